"""GPU tests of metrpo_score_actions (csrc/score_actions.hip): the discounted return every head predicts for candidate action sequences, against the
float64 restatement tests/score_actions_ref.py, against the device's own one-head replay (Engine.rollout_actions) discounted in NumPy, between its two
paths, against the device's validation cost, and under the planner of metrpo_amd.planning.

Bounds, all from tests/tolerances.py, none new.  A return is a discounted sum of free-running rewards, so its bound is the sum of the rewards' bounds:
sum_t gamma^t (row(t).atol + row(t).rtol |r_t^ref|) with row = REWARD for steps t <= 10 and LONG_RUN beyond (the rule of
tests/test_gpu_rollout_actions.py), CROSS_KERNEL between the two device paths at T <= 10.  The mean over the heads errs by at most the heads' mean error
and the population std is 1-Lipschitz in the root-mean-square of the heads' errors: both are held to the largest head's bound of the candidate.
Actions are 1.5 * randn, so the clip to [-1, 1] acts on both sides.  Where `len` is compared the restatement's z is first shown to stay 1e-4 clear of
Ant's thresholds, on every case."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import score_actions_ref as SA

pytestmark = pytest.mark.gpu


def cpu(t):
    return t.detach().cpu().numpy()


def reward_row(t):
    """tests/tolerances.py: REWARD for step t <= 10, LONG_RUN beyond (tests/test_gpu_rollout_actions.py)."""
    return TOL.REWARD if t <= 10 else TOL.LONG_RUN


def cross_row(t):
    return TOL.CROSS_KERNEL


# ---- problems: one engine per (env, K, hidden), built once -----------------------------------------------------------------------------------------
#           name             env            K  dynamics hidden  seed
SHAPES = {'swimmer':      ('swimmer',      5, (64, 64), 3),
          'half_cheetah': ('half_cheetah', 1, (64, 64), 4),     # one head: exact zeros in ret_std
          'ant':          ('ant',          8, (64, 64), 5),
          'hopper':       ('hopper',       5, (48, 48), 6),     # the zero-padded copy
          'snake':        ('snake',        8, (48, 48), 7),
          'swimmer9':     ('swimmer',      9, (64, 64), 8)}     # K > 8: fused here, step loop in rollout_actions
_problems = {}


def problem(name):
    if name not in _problems:
        env, K, hidden, seed = SHAPES[name]
        dm, theta, pdims, pool = Hh.problem_data(env, K, hidden, (32, 32), seed=seed, n_pool=64)
        dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
        pool = pool.astype(np.float32).astype(np.float64)
        _problems[name] = (Hh.engine_of(env, K, hidden, (32, 32), dm, theta), dm, theta, pdims, pool, env)
    return _problems[name]


def inputs(name, B, T, S, seed=0):
    """fp32-rounded start states (pool rows) and 1.5 * randn actions"""
    _, dm, _, _, pool, _ = problem(name)
    rng = np.random.RandomState(1000 * B + 10 * T + S + 7919 * seed)
    init = pool[rng.randint(len(pool), size=S)].astype(np.float32)
    actions = (1.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    assert actions.size < 32 or ((actions > 1).any() and (actions < -1).any())      # the clip acts on both sides
    return init, actions


_refs = {}


def reference(name, B, T, S, gamma, stop=True, seed=0):
    key = (name, B, T, S, gamma, stop, seed)
    if key not in _refs:
        _, dm, _, _, _, env = problem(name)
        init, actions = inputs(name, B, T, S, seed)
        _refs[key] = SA.score_actions(dm, env, init, actions, gamma=gamma, stop_at_done=stop, keep=True)
    return _refs[key]


def z_clear(env, ref, margin=1e-4):
    """Ant: no predicted z of the restatement (any head) within `margin` of the thresholds 0.2 / 1.0, and nothing non-finite.  No env is left out."""
    if not np.isfinite(ref['obs']).all():
        return False
    if env != 'ant':
        return True
    z = ref['obs'][:, 1:, :, 2]
    return bool(np.all(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) > margin))


WANT = ('ret', 'len', 'ret_mean', 'ret_std')


def run(name, B, T, S, gamma, stop=True, force_generic=False, seed=0, init=None, actions=None):
    eng = problem(name)[0]
    if init is None:
        init, actions = inputs(name, B, T, S, seed)
    a_dev = torch.as_tensor(actions, device=eng.device)
    a_before = a_dev.clone()
    out = eng.score_actions(init, a_dev, gamma=gamma, stop_at_done=stop, want=WANT, force_generic=force_generic)
    kernel = eng.last_score_actions_kernel()
    assert torch.equal(a_dev, a_before)                                               # d_actions is never written
    K = problem(name)[1].K
    assert out['ret'].shape == (K, B) and out['len'].shape == (K, B) and out['ret_mean'].shape == (B,) and out['ret_std'].shape == (B,)
    return {k: cpu(v) for k, v in out.items()}, kernel


def assert_follows(tag, got, ref, gamma, row=reward_row, check_len=True):
    bnd = SA.bound(ref['rew'], gamma, row)                                            # [K, B]
    top = bnd.max(axis=0)
    shares = [float((np.abs(got['ret'] - ref['ret']) / bnd).max()), float((np.abs(got['ret_mean'] - ref['mean']) / top).max()),
              float((np.abs(got['ret_std'] - ref['std']) / top).max())]
    print("%s: ret %.3g, mean %.3g, std %.3g of their bounds" % ((tag,) + tuple(shares)))
    assert np.all(np.abs(got['ret'] - ref['ret']) <= bnd), "%s ret" % tag
    assert np.all(np.abs(got['ret_mean'] - ref['mean']) <= top), "%s ret_mean" % tag
    assert np.all(np.abs(got['ret_std'] - ref['std']) <= top), "%s ret_std" % tag
    if check_len:
        assert np.array_equal(got['len'], ref['len']), "%s len" % tag


def within_one_ulp(got32, ref64):
    return np.abs(got32.astype(np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def replay_identity(name, B, T, S, gamma, stop, got, force_step_loop, seed=0, init=None, actions=None):
    """d_ret against the device's own one-head replay: rollout_actions(eps_rand, model=k)'s rew / done, the formula applied in NumPy float64"""
    eng, dm = problem(name)[:2]
    if init is None:
        init, actions = inputs(name, B, T, S, seed)
    starts = SA.start_rows(init, B).astype(np.float32)
    for k in range(dm.K):
        _, rew, done = eng.rollout_actions(starts, actions, 'eps_rand', model=k, force_step_loop=force_step_loop)
        assert eng.last_rollout_actions_kernel() == ('step-loop' if force_step_loop else 'fused')
        ret, n = SA.discount_and_sum(cpu(rew), cpu(done), gamma, stop)
        assert np.all(within_one_ulp(got['ret'][k], ret)), "%s head %d: %g" % (name, k, np.abs(got['ret'][k] - ret).max())
        assert np.array_equal(got['len'][k], n)


# ---- 1. the fused kernel against the restatement, at the tile edges ------------------------------------------------------------------------------------
# per env: every B of {1, 15, 16, 17, 33}, every T of {1, 2, 11}, S = 1, S = B and S = 3 at B = 33 (the boundary between two start states at
# candidate 11 and 22, inside a tile), both gammas
GRID = [(1, 1, 1, 1.0), (15, 2, 15, 0.99), (16, 11, 1, 0.99), (17, 11, 17, 1.0), (33, 11, 3, 0.99), (33, 2, 1, 1.0)]
CASES = [(name,) + g for name in SHAPES for g in GRID]


@pytest.mark.parametrize('name,B,T,S,gamma', CASES)
def test_fused_against_the_restatement(name, B, T, S, gamma):
    env = problem(name)[5]
    ref = reference(name, B, T, S, gamma)
    assert z_clear(env, ref)
    got, kernel = run(name, B, T, S, gamma)
    assert kernel == 'fused'
    assert_follows("%s B=%d T=%d S=%d gamma=%g" % (name, B, T, S, gamma), got, ref, gamma)
    if problem(name)[1].K == 1:
        assert np.array_equal(got['ret_std'], np.zeros(B, np.float32)) and np.array_equal(got['ret_mean'], got['ret'][0])


# ---- 2. the fused kernel against the device's own one-head replay: the step arithmetic is shared ---------------------------------------------------------
@pytest.mark.parametrize('name,B,T,S,gamma', [c for c in CASES if c[0] != 'swimmer9'])
def test_fused_is_the_one_head_replay_discounted(name, B, T, S, gamma):
    got, kernel = run(name, B, T, S, gamma)
    assert kernel == 'fused'
    replay_identity(name, B, T, S, gamma, True, got, force_step_loop=False)


# ---- 3. the generic path -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B,T,S,gamma', CASES)
def test_generic_on_the_fused_shapes(name, B, T, S, gamma):
    env = problem(name)[5]
    ref = reference(name, B, T, S, gamma)
    assert z_clear(env, ref)
    got, kernel = run(name, B, T, S, gamma, force_generic=True)
    assert kernel == 'generic'
    assert_follows("%s B=%d T=%d S=%d gamma=%g generic" % (name, B, T, S, gamma), got, ref, gamma)
    replay_identity(name, B, T, S, gamma, True, got, force_step_loop=True)
    if T <= 10:
        fused, f_kernel = run(name, B, T, S, gamma)
        assert f_kernel == 'fused'
        bnd = SA.bound(ref['rew'], gamma, cross_row)
        print("%s fused vs generic: %.3g of the bound" % (name, float((np.abs(fused['ret'] - got['ret']) / bnd).max())))
        assert np.all(np.abs(fused['ret'] - got['ret']) <= bnd)
        assert np.array_equal(fused['len'], got['len'])


OFF_TABLE = [('wide', 'swimmer', 5, (128, 128), (32, 32)), ('humanoid', 'humanoid', 2, (256, 256), (100, 50, 25))]


@pytest.mark.parametrize('tag,env,K,dh,ph', OFF_TABLE, ids=[c[0] for c in OFF_TABLE])
def test_off_table_shapes_take_the_generic_path(tag, env, K, dh, ph):
    B, T, S, gamma = 17, 3, 17, 0.99
    eng, dm, _, _, pool = Hh.make_engine(env, K, dh, ph, seed=11, n_pool=32)
    rng = np.random.RandomState(5)
    init = pool[rng.randint(len(pool), size=S)].astype(np.float32)
    actions = (1.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    out = eng.score_actions(init, actions, gamma=gamma, want=WANT)
    assert eng.last_score_actions_kernel() == 'generic'
    ret, n = cpu(out['ret']), cpu(out['len'])
    assert np.isfinite(ret).all()
    for k in range(K):
        _, rew, done = eng.rollout_actions(init, actions, 'eps_rand', model=k)
        assert eng.last_rollout_actions_kernel() == 'step-loop'
        r, ln = SA.discount_and_sum(cpu(rew), cpu(done), gamma, True)
        assert np.all(within_one_ulp(ret[k], r)) and np.array_equal(n[k], ln)
    m = ret.sum(axis=0, dtype=np.float64) / K
    np.testing.assert_allclose(cpu(out['ret_mean']), m, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(cpu(out['ret_std']), np.sqrt(((ret - m) ** 2).sum(axis=0) / K), rtol=1e-5, atol=1e-6 * (1 + np.abs(m).max()))


# ---- 4. Ant's mask ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
def test_ant_mask(force):
    name, B, T, S, gamma = 'ant', 17, 11, 17, 0.99
    _, dm, _, _, _, env = problem(name)
    init, actions = inputs(name, B, T, S, seed=2)               # seed 2: the restatement also has candidates that end by themselves at step 10
    init[3, 2], init[16, 2] = 1.2, 0.1                          # outside 0.2 <= z <= 1.0; the model moves z by ~0.1 a step: done at their first step
    for stop in (True, False):
        ref = SA.score_actions(dm, env, init, actions, gamma=gamma, stop_at_done=stop, keep=True)
        assert ref['done'][:, 0, 3].all() and ref['done'][:, 0, 16].all()
        assert z_clear(env, ref)                                # no candidate excluded: every z of every head and step is clear of the thresholds
        got, kernel = run(name, B, T, S, gamma, stop=stop, force_generic=force, init=init, actions=actions)
        assert kernel == ('generic' if force else 'fused')
        assert_follows("ant planted stop=%d" % stop, got, ref, gamma)
        if stop:
            assert np.all(got['len'][:, [3, 16]] == 1)
            bnd0 = reward_row(1)['atol'] + reward_row(1)['rtol'] * np.abs(ref['rew'][:, 0][:, [3, 16]])
            assert np.all(np.abs(got['ret'][:, [3, 16]] - ref['rew'][:, 0][:, [3, 16]]) <= bnd0)       # the return is r_0 alone
        else:
            assert np.all(got['len'] == T)


# ---- 5. closing the loop on the device: the policy's own actions on head k give the validation cost --------------------------------------------------------
@pytest.mark.parametrize('name', ['swimmer', 'ant'])
def test_policy_actions_give_the_device_validation_cost(name):
    B, T, gamma = 33, 11, 0.97
    eng, dm, theta, pdims, pool, env = problem(name)
    s0 = pool[:B].astype(np.float32)
    want = cpu(eng.validation_cost(s0, T, gamma))
    for k in range(dm.K):
        x = s0.astype(np.float64)
        acts = []
        for t in range(T):                                      # O.validation_costs' own loop on head k
            u = np.clip(O.policy_mean(theta, pdims, x), -1.0, 1.0)
            acts.append(u)
            x = O.dynamics_forward(dm, k, x, u)
            assert z_clear(env, dict(obs=x[None, None].repeat(2, axis=1)))
        out = eng.score_actions(s0, np.stack(acts).astype(np.float32), gamma=gamma)
        got = -cpu(out['ret'])[k].astype(np.float64).mean()
        print("%s head %d: %.9g against validation_cost %.9g" % (name, k, got, want[k]))
        np.testing.assert_allclose(got, want[k], **TOL.VALIDATION_COST)


# ---- 6. guard cells ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('name', ['swimmer', 'ant'])
@pytest.mark.parametrize('B', [17, 1])
def test_no_write_beyond_B(name, B, force):
    """Each output is the front of a larger allocation whose tail -- guard cells behind [K][B] (or [B]) -- holds a sentinel."""
    eng, dm = problem(name)[:2]
    K, T, G = dm.K, 3, 5
    init, actions = inputs(name, B, T, 1)
    dev = eng.device
    a_dev = torch.as_tensor(actions, device=dev); a_before = a_dev.clone()
    g = {'ret': torch.full((K * B + G,), 777.0, dtype=torch.float32, device=dev), 'len': torch.full((K * B + G,), -77, dtype=torch.int32, device=dev),
         'ret_mean': torch.full((B + G,), 777.0, dtype=torch.float32, device=dev), 'ret_std': torch.full((B + G,), 777.0, dtype=torch.float32, device=dev)}
    n = {'ret': K * B, 'len': K * B, 'ret_mean': B, 'ret_std': B}
    out = eng.score_actions(init, a_dev, gamma=0.99, want=WANT, force_generic=force, out={w: g[w][:n[w]] for w in g})
    assert eng.last_score_actions_kernel() == ('generic' if force else 'fused')
    plain = eng.score_actions(init, a_dev, gamma=0.99, want=WANT, force_generic=force)
    torch.cuda.synchronize()
    for w in g:
        assert torch.all(g[w][n[w]:] == (-77 if w == 'len' else 777.0)), w            # nothing behind [K][B]
        assert not torch.any(g[w][:n[w]] == (-77 if w == 'len' else 777.0)), w        # every cell in front of it was written
        assert torch.equal(out[w].reshape(-1), plain[w].reshape(-1)), w                # and repeated calls are bit-identical
    assert torch.equal(a_dev, a_before)


# ---- 7. a call changes nothing else ----------------------------------------------------------------------------------------------------------------------------
def test_a_score_actions_call_changes_nothing_else():
    """The body of tests/test_gpu_rollout_actions.py::test_a_known_actions_call_changes_nothing_else, plus the reporters of the sibling entry points."""
    import test_gpu_model_error as TM
    _, dm, theta, pdims, pool, Os, As, Rs = TM.problem('swimmer')
    eng = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)
    rng = np.random.RandomState(0)
    x = rng.randn(5 * 16, dm.ns + dm.na).astype(np.float32); y = rng.randn(5 * 16, dm.ns).astype(np.float32)
    eng.train_step(x, y, 16, 1e-3)
    eng.policy_adam_step(torch.as_tensor(rng.randn(eng.P), dtype=torch.float64, device=eng.device), 1e-3)
    state = lambda: [eng.get_policy().clone(), eng.get_dynamics().clone()] + [t.clone() if torch.is_tensor(t) else t for t in eng.get_train_adam()] + \
        [t.clone() if torch.is_tensor(t) else t for t in eng.get_policy_adam()]
    before = state()
    roll = lambda: eng.rollout(128, 6, 4, 'step_rand', pool.astype(np.float32), seed=5)
    t1 = roll()
    o1, r1, a1 = t1.obs.clone(), t1.rew.clone(), t1.act.clone()
    kernel, note = eng.last_rollout_kernel(), eng.rollout_note()
    acts = (1.5 * rng.randn(5, 40, dm.na)).astype(np.float32)
    eng.rollout_actions(pool[:40].astype(np.float32), acts, 'model_mean')
    eng.ensemble_disagreement(pool[:40].astype(np.float32), acts[0], force_generic=True)
    assert eng.last_rollout_actions_kernel() == 'fused' and eng.last_disagreement_kernel() == 'generic' and eng.last_score_actions_kernel() is None
    for force in (False, True):
        eng.score_actions(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT, force_generic=force)
        assert eng.last_score_actions_kernel() == ('generic' if force else 'fused')
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note
    assert eng.last_rollout_actions_kernel() == 'fused' and eng.last_disagreement_kernel() == 'generic'
    t2 = roll()                                                                           # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


# ---- 8. the ABI's argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    eng, dm = problem('swimmer')[:2]
    dev = eng.device
    B, T, S, K, ns, na = 4, 2, 2, dm.K, dm.ns, dm.na
    init, act = torch.zeros(S, ns, device=dev), torch.zeros(T, B, na, device=dev)
    ret = torch.full((K, B), 555.0, dtype=torch.float32, device=dev)                       # outputs hold a sentinel
    ln = torch.full((K, B), -55, dtype=torch.int32, device=dev)
    mean, sd = torch.full((B,), 555.0, device=dev), torch.full((B,), 555.0, device=dev)

    def args(**kw):
        a = _lib.ScoreActionsArgs()
        a.B, a.T, a.S, a.stop_at_done, a.gamma = B, T, S, 1, 0.99
        a.d_init_obs, a.d_actions, a.d_ret, a.d_len, a.d_ret_mean, a.d_ret_std = (init.data_ptr(), act.data_ptr(), ret.data_ptr(), ln.data_ptr(),
                                                                                 mean.data_ptr(), sd.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.metrpo_score_actions(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_score_actions(None, C.byref(args()), eng._stream()) == -2 and lib.metrpo_last_score_actions_kernel(None) == -2
    assert lib.metrpo_score_actions(eng._ctx, None, eng._stream()) == -2 and b'args NULL' in err()
    for name in ('d_init_obs', 'd_actions', 'd_ret'):
        assert call(args(**{name: None})) == -2 and b'required pointer' in err()           # METRPO_ENULL
    assert call(args(B=-1)) == -1 and b'bad B/T' in err()                                  # METRPO_EINVAL
    assert call(args(T=-1)) == -1 and b'bad B/T' in err()
    for bad in (0, -1, 3):
        assert call(args(S=bad)) == -1 and b'must be at least 1 and divide B' in err()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(args(gamma=bad)) == -1 and b'gamma is not finite' in err()
    # B == 0 or T == 0: OK, nothing written -- not even with NULL pointers, which are not looked at
    for kw in (dict(B=0), dict(T=0), dict(B=0, d_ret=None)):
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert torch.all(ret == 555.0) and torch.all(ln == -55) and torch.all(mean == 555.0) and torch.all(sd == 555.0)
    # the optional outputs may be left out, each on its own
    for kw in (dict(d_len=None), dict(d_ret_mean=None), dict(d_ret_std=None), dict(d_len=None, d_ret_mean=None, d_ret_std=None), dict(force_generic=1, d_len=None)):
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert not torch.any(ret == 555.0) and not torch.any(ln == -55) and not torch.any(mean == 555.0) and not torch.any(sd == 555.0)
    # dynamics must be set, the policy need not be
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_score_actions(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_score_actions_kernel() is None
    bare.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    o2 = bare.score_actions(init, act, gamma=0.99, want=WANT)                              # no metrpo_set_policy: theta is never read
    o1 = eng.score_actions(init, act, gamma=0.99, want=WANT)
    for w in WANT:
        assert torch.equal(o1[w], o2[w])
    # the host method's own checks
    with pytest.raises(ValueError, match=r'init_obs: expected \[S, 10\]'):
        eng.score_actions(torch.zeros(S, ns + 1), act)
    with pytest.raises(ValueError, match=r'actions: expected \[T, B, 2\] with B a multiple of 3'):
        eng.score_actions(torch.zeros(3, ns), act)
    with pytest.raises(ValueError, match='want'):
        eng.score_actions(init, act, want=('ret', 'median'))
    one = eng.score_actions(torch.zeros(ns), act, want=WANT)                               # [ns]: one start state
    assert one['ret'].shape == (K, B)


# ---- 9. the planner on the device ---------------------------------------------------------------------------------------------------------------------------------
def test_plan_cem_on_the_device(monkeypatch):
    from metrpo_amd import planning as P
    eng, dm, _, _, pool, env = problem('swimmer')
    S, N, T, E, gamma = 2, 48, 5, 6, 0.99
    states = pool[[3, 17]].astype(np.float32)
    shown = []

    def restated(actions, init):                               # the float64 restatement wrapped for torch
        ref = SA.score_actions(dm, env, cpu(init), cpu(actions), gamma=gamma, keep=True)
        shown.append(ref)
        return torch.as_tensor(ref['ret'], dtype=torch.float32, device=actions.device)

    gen = lambda seed: torch.Generator(device=eng.device).manual_seed(seed)
    seed = None
    for s in range(8):                                          # a seed at which the restatement's elite set is decided by more than the bound
        del shown[:]
        want = P.plan_cem(eng, states, T, N, E, 1, gamma=gamma, generator=gen(s), scorer=restated)
        ref = shown[0]
        score = ref['ret'].mean(axis=0).reshape(S, N)
        bnd = SA.bound(ref['rew'], gamma, reward_row).max(axis=0).reshape(S, N)
        el = cpu(want['elites'])
        ok = True
        for i in range(S):
            rest = np.setdiff1d(np.arange(N), el[i])
            ok = ok and (score[i, el[i]] - bnd[i, el[i]]).min() > (score[i, rest] + bnd[i, rest]).max()
        if ok:
            seed = s
            break
    assert seed is not None
    got1 = P.plan_cem(eng, states, T, N, E, 1, gamma=gamma, generator=gen(seed))
    assert eng.last_score_actions_kernel() == 'fused'
    for i in range(S):
        assert set(cpu(got1['elites'])[i].tolist()) == set(el[i].tolist())
    np.testing.assert_allclose(cpu(got1['actions']), cpu(want['actions']), rtol=0, atol=1e-6)       # the same elites: the same refit
    # three iterations with nothing read back: one synchronize behind the call, none inside
    torch.cuda.synchronize()
    counts = dict(sync=0, item=0, cpu=0)
    real_sync, real_item, real_cpu = torch.cuda.synchronize, torch.Tensor.item, torch.Tensor.cpu

    def counted(key, fn):
        def wrapper(*a, **kw):
            counts[key] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(torch.cuda, 'synchronize', counted('sync', real_sync))
    monkeypatch.setattr(torch.Tensor, 'item', counted('item', real_item))
    monkeypatch.setattr(torch.Tensor, 'cpu', counted('cpu', real_cpu))
    got3 = P.plan_cem(eng, states, T, N, E, 3, gamma=gamma, generator=gen(seed))
    inside = dict(counts)
    torch.cuda.synchronize()
    assert inside == dict(sync=0, item=0, cpu=0) and counts['sync'] == 1
    monkeypatch.undo()
    assert got3['history'].shape == (3, S) and torch.isfinite(got3['history']).all() and torch.isfinite(got3['actions']).all()
    assert torch.all(got3['best_score'] >= got3['history'].max(dim=0).values)
    sc = P.score_action_sequences(eng, states, got3['best_actions'], gamma=gamma)
    torch.testing.assert_close(sc, got3['best_score'], rtol=1e-5, atol=1e-5)              # the best candidate scores what the planner recorded


# ---- 10. the controller as a data-collection policy ----------------------------------------------------------------------------------------------------------
def test_example_loop_collects_with_the_shooting_controller():
    """examples/me_trpo_loop.py --shooting: from the second outer iteration on the real data are collected by planning.ShootingController over the
    ensemble just trained (tests/test_gpu_api.py::test_end_to_end_outer_loop_example's sizes)."""
    import importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('me_trpo_loop', os.path.join(root, 'examples', 'me_trpo_loop.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    hist = mod.main(['--outer', '2', '--K', '3', '--T', '20', '--traj', '40', '--n-envs', '200', '--policy-iters', '6', '--model-passes', '6',
                     '--quiet', '--shooting'])
    assert len(hist) == 2 and hist[1]['n_data'] > hist[0]['n_data'] > 0
    assert all(np.isfinite([h['real_cost'], h['model_val'], h['est_cost']]).all() for h in hist)
