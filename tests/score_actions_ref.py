"""NumPy restatement of metrpo_score_actions (include/metrpo.h), float64 arithmetic on the fp32 inputs the device stores: per head k and candidate b the
cost sum of build_policy_graph (model_based_rl.py:122-141: model k fixed for the whole trajectory, the done mask updated AFTER the step's cost,
:134-137) under supplied actions (clipped once, env_helpers.py:216 / :599), negated and kept per candidate.

    alive_0 = 1;  ret = sum_t gamma^t alive_t r_t;  alive_t+1 = alive_t and not is_done(s_t+1)      (stop_at_done; else alive = 1 throughout)

gamma^t is formed by repeated multiplication and the sum is carried in step order, as the header says; a step that is not counted adds nothing.
"""
import numpy as np

from oracle import metrpo_oracle as O


def start_rows(init_obs, B):
    """init_obs [S, ns] or [ns] -> [B, ns]: candidate b starts from init_obs[b // (B // S)]"""
    init = np.atleast_2d(np.asarray(init_obs, np.float64))
    S = init.shape[0]
    assert S >= 1 and B % S == 0
    return init[np.arange(B) // (B // S)]


def score_actions(dm, env, init_obs, actions, gamma=1.0, stop_at_done=True, keep=False):
    """init_obs [S, ns], actions [T, B, na] unclipped.  -> dict(ret [K, B], len [K, B] int, mean [B], std [B] (population std over the heads);
    with keep: rew [K, T, B] the per-step rewards r_t (unmasked), done [K, T, B], obs [K, T+1, B, ns])."""
    a = np.clip(np.asarray(actions, np.float64), -1.0, 1.0)
    T, B = a.shape[:2]
    s0 = start_rows(init_obs, B)
    K = dm.K
    ret = np.zeros((K, B)); length = np.zeros((K, B), np.int64)
    rews, dones, obss = [], [], []
    for k in range(K):
        s = s0.copy()
        alive = np.ones(B, bool)
        disc = 1.0
        rew_k, done_k, obs_k = [], [], [s]
        for t in range(T):
            with np.errstate(all='ignore'):
                nxt = O.dynamics_forward(dm, k, s, a[t])
                r = -O.cost_np_vec(env, s, a[t], nxt)
            dn = np.asarray(O.is_done(env, nxt, nxt), bool)
            ret[k] = np.where(alive, ret[k] + disc * r, ret[k])
            length[k] += alive
            disc = disc * gamma
            if stop_at_done:
                alive = alive & ~dn
            rew_k.append(r); done_k.append(dn); obs_k.append(nxt)
            s = nxt
        rews.append(np.stack(rew_k)); dones.append(np.stack(done_k)); obss.append(np.stack(obs_k))
    out = dict(ret=ret, len=length, mean=ret.sum(axis=0) / K, std=np.sqrt(((ret - ret.sum(axis=0) / K) ** 2).sum(axis=0) / K))
    if keep:
        out.update(rew=np.stack(rews), done=np.stack(dones), obs=np.stack(obss))
    return out


def discount_and_sum(rew, done, gamma=1.0, stop_at_done=True):
    """The formula alone on one head's recorded rew / done [T, B] (float64 on whatever precision they come in) -> (ret [B] float64, len [B])."""
    rew = np.asarray(rew, np.float64)
    T, B = rew.shape
    ret = np.zeros(B); length = np.zeros(B, np.int64)
    alive = np.ones(B, bool)
    disc = 1.0
    for t in range(T):
        ret = np.where(alive, ret + disc * rew[t], ret)
        length += alive
        disc = disc * gamma
        if stop_at_done:
            alive = alive & ~np.asarray(done[t], bool)
    return ret, length


def bound(ref_rew, gamma, row_of_step):
    """The per-sample bound of a return: sum_t gamma^t (row(t).atol + row(t).rtol |r_t^ref|), row_of_step(t) with t = 1 .. T the step's number
    (tests/test_gpu_rollout_actions.py's rule).  ref_rew [..., T, B] -> [..., B]."""
    ref_rew = np.asarray(ref_rew, np.float64)
    T = ref_rew.shape[-2]
    out = np.zeros(ref_rew.shape[:-2] + ref_rew.shape[-1:])
    disc = 1.0
    for t in range(T):
        row = row_of_step(t + 1)
        out += abs(disc) * (row['atol'] + row['rtol'] * np.abs(ref_rew[..., t, :]))
        disc *= gamma
    return out
