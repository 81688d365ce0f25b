"""NumPy restatement of metrpo_score_policy_actions (include/metrpo.h), float64 arithmetic on the fp32 inputs the device stores: per head k and candidate
b the cost sum of build_policy_graph (model_based_rl.py:122-141: model k fixed for the whole trajectory, the done mask updated AFTER the step's cost,
:134-137) with the action of every step formed from the head's own state,

    mean_t = policy_mean(s_t);   a_t = mean_t + noise_t   (noise_in_std: noise_t * exp(log_std) + mean_t, get_actions' arithmetic;  no noise: mean_t)
    u_t = clip(a_t, -1, 1);      s_t+1 = head k (s_t, u_t);   r_t = -cost_np_vec(s_t, u_t, s_t+1)

and score_actions_ref's return: gamma^t by repeated multiplication, the sum in step order, a step that is not counted adds nothing.
dtype=np.float32 restates the device's precision: parameters, states, actions and rewards in fp32 (the sum stays float64, as on the device).

The second half holds the cases the CPU test (tests/test_score_policy_ref.py) and the GPU test (tests/test_gpu_score_policy.py) share.
"""
import numpy as np

from oracle import metrpo_oracle as O
import helpers as Hh
from score_actions_ref import start_rows, bound          # noqa: F401  (re-exported: the GPU test takes them from here)

WRONG = ('noise_after_clip', 'mean_at_next', 'std_when_plain', 'mask_before_cost')


def score_policy_actions(dm, theta, pdims, env, init_obs, noise=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False, keep=False,
                         dtype=np.float64, wrong=None):
    """init_obs [S, ns]; noise [T, B, na] or None (then T= steps and B = S).  -> dict(ret [K, B] float64, len [K, B] int, mean [B], std [B]
    (population std over the heads); with keep: rew [K, T, B] the per-step rewards (unmasked), done [K, T, B], obs [K, T+1, B, ns], act [K, T, B, na]
    the UNCLIPPED actions).  wrong: one of WRONG, a deliberately wrong restatement (the CPU test shows that each misses a bound)."""
    assert wrong is None or wrong in WRONG
    init = np.atleast_2d(np.asarray(init_obs, np.float64))
    if noise is None:
        B, T = init.shape[0], int(T)
        nz = None
    else:
        nz = np.asarray(noise, dtype)
        T, B = nz.shape[:2]
    s0 = start_rows(init, B).astype(dtype)
    if dtype != np.float64:
        dm = dm.astype(dtype)
    theta = np.asarray(theta, dtype)
    sig = np.exp(O.policy_log_std(theta, pdims)).astype(dtype)
    K = dm.K
    ret = np.zeros((K, B)); length = np.zeros((K, B), np.int64)
    rews, dones, obss, acts = [], [], [], []

    def action(s, t):
        m = O.policy_mean(theta, pdims, s).astype(dtype)
        if nz is None:
            return m
        if noise_in_std or wrong == 'std_when_plain':
            return nz[t] * sig + m
        return m + nz[t]

    for k in range(K):
        s = s0.copy()
        alive = np.ones(B, bool)
        disc = 1.0
        rew_k, done_k, obs_k, act_k = [], [], [s], []
        for t in range(T):
            with np.errstate(all='ignore'):
                a = action(s, t)
                u = np.clip(a, -1.0, 1.0).astype(dtype)
                if wrong == 'noise_after_clip' and nz is not None:
                    u = (np.clip(O.policy_mean(theta, pdims, s), -1.0, 1.0) + (nz[t] * sig if noise_in_std else nz[t])).astype(dtype)
                nxt = np.asarray(O.dynamics_forward(dm, k, s, u), dtype)
                u_cost = np.clip(action(nxt, t), -1.0, 1.0).astype(dtype) if wrong == 'mean_at_next' else np.clip(u, -1.0, 1.0)   # (the oracle's cost refuses |u| > 1)
                r = np.asarray(-O.cost_np_vec(env, s, u_cost, nxt), dtype)
            dn = np.asarray(O.is_done(env, nxt, nxt), bool)
            if wrong == 'mask_before_cost' and stop_at_done:
                alive = alive & ~dn
            ret[k] = np.where(alive, ret[k] + disc * r.astype(np.float64), ret[k])
            length[k] += alive
            disc = disc * gamma
            if stop_at_done and wrong != 'mask_before_cost':
                alive = alive & ~dn
            rew_k.append(r); done_k.append(dn); obs_k.append(nxt); act_k.append(a)
            s = nxt
        rews.append(np.stack(rew_k)); dones.append(np.stack(done_k)); obss.append(np.stack(obs_k)); acts.append(np.stack(act_k))
    out = dict(ret=ret, len=length, mean=ret.sum(axis=0) / K, std=np.sqrt(((ret - ret.sum(axis=0) / K) ** 2).sum(axis=0) / K))
    if keep:
        out.update(rew=np.stack(rews).astype(np.float64), done=np.stack(dones), obs=np.stack(obss).astype(np.float64), act=np.stack(acts).astype(np.float64))
    return out


# ---- the cases the CPU and the GPU test share ---------------------------------------------------------------------------------------------------------
#           name             env            K  dynamics hidden  seed
SHAPES = {'swimmer':      ('swimmer',      5, (64, 64), 3),
          'half_cheetah': ('half_cheetah', 1, (64, 64), 4),     # one head: exact zeros in ret_std
          'ant':          ('ant',          8, (64, 64), 5),
          'hopper':       ('hopper',       5, (48, 48), 6),     # the zero-padded copy
          'snake':        ('snake',        8, (48, 48), 7),
          'swimmer9':     ('swimmer',      9, (64, 64), 8)}     # more heads than a workgroup has waves
# (B, T, S, gamma, stop_at_done, noise_in_std, with noise): every B of {1, 15, 16, 17, 33}, every T of {1, 2, 11}, S = 1, S = B and S = 3 at B = 33
# (the boundary between two start states inside a tile), both gammas, both masks, both noise units, and the deterministic policy (B = S)
GRID = [(1, 1, 1, 1.0, True, False, True), (15, 2, 15, 0.99, False, True, True), (16, 11, 1, 0.99, True, True, True), (17, 11, 17, 1.0, True, False, False),
        (33, 11, 3, 0.99, True, False, True), (33, 2, 1, 1.0, False, True, True), (16, 2, 16, 0.99, True, False, False)]
CASES = [(name,) + g for name in SHAPES for g in GRID]
NOISE_SCALE = 1.5          # noise = 1.5 * randn (tests/test_gpu_score_actions.py's actions): the clip to [-1, 1] acts on both sides
_problems = {}


def problem_data(name):
    """(dm, theta, pdims, pool, env), every array rounded to fp32 and held in float64: what the device stores"""
    if name not in _problems:
        env, K, hidden, seed = SHAPES[name]
        dm, theta, pdims, pool = Hh.problem_data(env, K, hidden, (32, 32), seed=seed, n_pool=64)
        dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
        _problems[name] = (dm, theta, pdims, pool.astype(np.float32).astype(np.float64), env)
    return _problems[name]


def inputs(name, B, T, S, with_noise=True, seed=0):
    """fp32 start states (pool rows; Ant with S >= 3: rows 1 and S - 1 planted outside 0.2 <= z <= 1.0, so the mask acts) and noise, or None"""
    dm, _, _, pool, env = problem_data(name)
    rng = np.random.RandomState(1000 * B + 10 * T + S + 7919 * seed)
    init = pool[rng.randint(len(pool), size=S)].astype(np.float32)
    if env == 'ant' and S >= 3:
        init[1, 2], init[S - 1, 2] = 1.2, 0.1
    noise = (NOISE_SCALE * rng.randn(T, B, dm.na)).astype(np.float32) if with_noise else None
    return init, noise


def z_clear(env, ref, margin=1e-4):
    """Ant: no predicted z of the restatement (any head) within `margin` of the thresholds 0.2 / 1.0, and nothing non-finite.  No env is left out."""
    if not np.isfinite(ref['obs']).all():
        return False
    if env != 'ant':
        return True
    z = ref['obs'][:, 1:, :, 2]
    return bool(np.all(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) > margin))


_refs = {}


def reference(name, B, T, S, gamma, stop, in_std, with_noise, seed=0, dtype=np.float64):
    key = (name, B, T, S, gamma, stop, in_std, with_noise, seed, np.dtype(dtype).name)
    if key not in _refs:
        dm, theta, pdims, _, env = problem_data(name)
        init, noise = inputs(name, B, T, S, with_noise, seed)
        _refs[key] = score_policy_actions(dm, theta, pdims, env, init, noise, T=T, gamma=gamma, stop_at_done=stop, noise_in_std=in_std, keep=True, dtype=dtype)
    return _refs[key]
