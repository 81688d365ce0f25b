"""GPU tests of metrpo_rollout_actions (csrc/rollout_actions.hip): the ensemble rolled forward under supplied actions, against the float64 restatement
tests/rollout_actions_ref.py, against Engine.step chained from Python, against the policy rollout whose actions it replays, and inside the model
diagnostic (metrpo_model_error with known_actions).

Bounds, all from tests/tolerances.py, none new: device and restatement each feed their own states back, so row t of obs is held to FREE_RUN for
t <= 10 and to LONG_RUN beyond (tolerances.py:28, :31; row_of_step of tests/test_gpu_model_error.py), the reward of step t to REWARD for t <= 10 and to
LONG_RUN beyond (the same rule), two device paths free-running on the same inputs to CROSS_KERNEL for t <= 10.  Actions are 1.5 * randn, so the clip to
[-1, 1] acts on both sides.  Where `done` is compared for equality the restatement's z is first shown to stay 1e-4 clear of Ant's thresholds."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import rollout_actions_ref as RA

pytestmark = pytest.mark.gpu


def cpu(t):
    return t.detach().cpu().numpy()


def row_of_step(t):
    """tests/tolerances.py: FREE_RUN for t <= 10 (line 28), LONG_RUN beyond (line 31)."""
    return TOL.FREE_RUN if t <= 10 else TOL.LONG_RUN


def reward_row(t):
    return TOL.REWARD if t <= 10 else TOL.LONG_RUN


# ---- problems: one engine per (env, K, hidden), built once -----------------------------------------------------------------------------------------
#          env            K  dynamics hidden   seed (Ant: the restatement's z stays clear of 0.2 / 1.0 on every case below, asserted there)
SHAPES = {'swimmer':      (5, (64, 64), 3),    # ns 10: one output block
          'half_cheetah': (1, (64, 64), 4),    # n_drop 1, ns 18: two output blocks
          'ant':          (8, (64, 64), 5),    # ns 29, the 8-wave workgroup, more than 64 KB of LDS
          'hopper':       (5, (48, 48), 6),    # n_drop 0; the zero-padded copy
          'snake':        (8, (48, 48), 7)}
MODES = ('mean', 'mixed', 'uniform', 'one')
_problems = {}


def problem(env):
    if env not in _problems:
        K, hidden, seed = SHAPES[env]
        dm, theta, pdims, pool = Hh.problem_data(env, K, hidden, (32, 32), seed=seed, n_pool=64)
        dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
        pool = pool.astype(np.float32).astype(np.float64)
        _problems[env] = (Hh.engine_of(env, K, hidden, (32, 32), dm, theta), dm, theta, pdims, pool)
    return _problems[env]


def inputs(env, B, T, seed=0):
    """fp32-rounded initial states (pool rows) and 1.5 * randn actions, plus a mixed head vector."""
    _, dm, _, _, pool = problem(env)
    rng = np.random.RandomState(1000 * B + 10 * T + seed)
    init = pool[rng.randint(len(pool), size=B)].astype(np.float32)
    actions = (1.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    heads = rng.randint(dm.K, size=B)
    if B > 1 and dm.K > 1:
        heads[0], heads[-1] = 0, dm.K - 1                 # mixed for sure, first and last head present
    assert actions.size < 32 or ((actions > 1).any() and (actions < -1).any())      # the clip acts on both sides
    return init, actions, heads


def mode_args(mode, dm, heads):
    """-> (Engine.rollout_actions keyword arguments, the restatement's `model`)"""
    if mode == 'mean':
        return dict(sam_mode='model_mean'), -1
    if mode == 'mixed':
        return dict(sam_mode='eps_rand', model=torch.as_tensor(heads, dtype=torch.int32)), heads
    if mode == 'uniform':
        return dict(sam_mode='eps_rand', model=dm.K - 1), dm.K - 1
    return dict(sam_mode='one_model'), 0                     # head 0 by definition (env_helpers.py:631-632)


def z_clear(env, ref, margin=1e-4):
    """Ant: no predicted z of the restatement within `margin` of the thresholds 0.2 / 1.0 (else fp32 and float64 may disagree on `done`, an error of
    neither), and nothing non-finite.  No env is left out."""
    if not np.isfinite(ref['obs']).all():
        return False
    if env != 'ant':
        return True
    z = ref['obs'][1:, :, 2]
    return bool(np.all(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) > margin))


def assert_follows(tag, got, ref):
    """obs / rew of a device result against the restatement, row by row with the row's bound; the worst share of a bound is printed first."""
    obs, rew = got
    T = rew.shape[0]
    worst_o = worst_r = 0.0
    for t in range(1, T + 1):
        ro, rr = row_of_step(t), reward_row(t)
        worst_o = max(worst_o, float((np.abs(obs[t] - ref['obs'][t]) / (ro['atol'] + ro['rtol'] * np.abs(ref['obs'][t]))).max()))
        worst_r = max(worst_r, float((np.abs(rew[t - 1] - ref['rew'][t - 1]) / (rr['atol'] + rr['rtol'] * np.abs(ref['rew'][t - 1]))).max()))
    print("%s: obs %.3g, rew %.3g of their bounds" % (tag, worst_o, worst_r))
    for t in range(1, T + 1):
        np.testing.assert_allclose(obs[t], ref['obs'][t], err_msg="%s obs row %d" % (tag, t), **row_of_step(t))
        np.testing.assert_allclose(rew[t - 1], ref['rew'][t - 1], err_msg="%s reward of step %d" % (tag, t), **reward_row(t))


def run(env, B, T, mode, force_step_loop=False, seed=0):
    eng, dm, _, _, _ = problem(env)
    init, actions, heads = inputs(env, B, T, seed)
    kw, model = mode_args(mode, dm, heads)
    a_dev = torch.as_tensor(actions, device=eng.device)
    a_before = a_dev.clone()
    obs, rew, done = eng.rollout_actions(init, a_dev, force_step_loop=force_step_loop, **kw)
    kernel = eng.last_rollout_actions_kernel()
    assert torch.equal(a_dev, a_before)                                               # d_actions is never written (unclipped in, unclipped after)
    assert np.array_equal(cpu(obs[0]).view(np.uint32), init.view(np.uint32))           # row 0 = d_init_obs, bit for bit
    return (cpu(obs), cpu(rew), cpu(done).astype(bool)), kernel, (dm, init, actions, model)


_refs = {}


def reference(env, B, T, mode, seed=0):
    key = (env, B, T, mode, seed)
    if key not in _refs:
        _, dm, _, _, _ = problem(env)
        init, actions, heads = inputs(env, B, T, seed)
        _refs[key] = RA.rollout_actions(dm, env, init, actions, model=mode_args(mode, dm, heads)[1])
    return _refs[key]


# ---- 1. the fused kernel against the restatement, at the tile edges ------------------------------------------------------------------------------------
# every env, every B of {1, 15, 16, 17, 33}, every T of {1, 2, 11} and every mode at least once; both one-head modes and both all-head modes on every env
CASES = [('swimmer', 1, 1, 'mean'), ('swimmer', 15, 2, 'mixed'), ('swimmer', 16, 11, 'uniform'), ('swimmer', 17, 11, 'one'), ('swimmer', 33, 11, 'mean'),
         ('swimmer', 17, 11, 'mixed'),
         ('half_cheetah', 17, 2, 'mean'), ('half_cheetah', 33, 11, 'mixed'), ('half_cheetah', 1, 11, 'uniform'), ('half_cheetah', 16, 1, 'one'),
         ('ant', 33, 11, 'mean'), ('ant', 17, 2, 'mixed'), ('ant', 15, 11, 'uniform'), ('ant', 1, 2, 'one'), ('ant', 16, 11, 'mixed'),
         ('hopper', 16, 11, 'mean'), ('hopper', 17, 11, 'mixed'), ('hopper', 33, 2, 'uniform'), ('hopper', 15, 1, 'one'),
         ('snake', 15, 11, 'mixed'), ('snake', 33, 11, 'mean'), ('snake', 17, 1, 'uniform'), ('snake', 1, 11, 'one')]


@pytest.mark.parametrize('env,B,T,mode', CASES)
def test_fused_against_the_restatement(env, B, T, mode):
    ref = reference(env, B, T, mode)
    assert z_clear(env, ref)
    (obs, rew, done), kernel, _ = run(env, B, T, mode)
    assert kernel == 'fused'
    assert obs.shape == (T + 1, B, ref['obs'].shape[2]) and rew.shape == (T, B) and done.shape == (T, B)
    assert_follows("%s B=%d T=%d %s" % (env, B, T, mode), (obs, rew), ref)
    assert np.array_equal(done, ref['done'])


# ---- 2. no write beyond B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'step-loop'])
@pytest.mark.parametrize('env,mode', [('swimmer', 'mean'), ('ant', 'uniform'), ('half_cheetah', 'mixed')])
@pytest.mark.parametrize('B', [17, 1])
def test_no_write_beyond_B(env, mode, B, force):
    """Each output is the front of a larger allocation whose tail -- one guard row behind [.., B, ..] of the last time step -- holds a sentinel."""
    eng, dm, _, _, _ = problem(env)
    T, ns = 3, dm.ns
    init, actions, heads = inputs(env, B, T)
    kw, _ = mode_args(mode, dm, heads)
    dev = eng.device
    g_obs = torch.full(((T + 1) * B * ns + ns,), 777.0, dtype=torch.float32, device=dev)
    g_rew = torch.full((T * B + 1,), 777.0, dtype=torch.float32, device=dev)
    g_done = torch.full((T * B + 1,), 0xAB, dtype=torch.uint8, device=dev)
    out = (g_obs[:(T + 1) * B * ns].view(T + 1, B, ns), g_rew[:T * B].view(T, B), g_done[:T * B].view(T, B))
    obs, rew, done = eng.rollout_actions(init, actions, force_step_loop=force, out=out, **kw)
    assert eng.last_rollout_actions_kernel() == ('step-loop' if force else 'fused')
    plain = eng.rollout_actions(init, actions, force_step_loop=force, **kw)
    torch.cuda.synchronize()
    assert torch.all(g_obs[(T + 1) * B * ns:] == 777.0) and g_rew[T * B].item() == 777.0 and g_done[T * B].item() == 0xAB
    assert not torch.any(obs == 777.0) and not torch.any(rew == 777.0) and torch.all(done <= 1)      # ... and every cell in front of it was written
    for a, b in zip((obs, rew, done), plain):
        assert torch.equal(a, b)


# ---- 3. a done neither stops nor resets (Ant) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['mean', 'uniform'])
def test_done_does_not_stop_or_reset(mode):
    env, B, T = 'ant', 17, 11
    eng, dm, _, _, _ = problem(env)
    init, actions, heads = inputs(env, B, T, seed=1)
    init[3, 2], init[16, 2] = 1.2, 0.1                          # outside 0.2 <= z <= 1.0; the model moves z by ~0.1 a step: done at their first step
    kw, model = mode_args(mode, dm, heads)
    ref = RA.rollout_actions(dm, env, init, actions, model=model)
    assert ref['done'][0, 3] and ref['done'][0, 16]
    z0 = ref['obs'][1, [3, 16], 2]
    assert np.all(np.minimum(np.abs(z0 - 0.2), np.abs(z0 - 1.0)) > 1e-4)
    assert z_clear(env, ref)                                    # no env excluded: every z of every step is clear of the thresholds
    obs, rew, done = eng.rollout_actions(init, actions, **kw)
    assert eng.last_rollout_actions_kernel() == 'fused'
    obs, rew, done = cpu(obs), cpu(rew), cpu(done).astype(bool)
    assert done[0, 3] and done[0, 16]
    assert_follows("ant planted %s" % mode, (obs, rew), ref)    # rows behind the done included: the env was neither stopped nor reset
    assert np.array_equal(done, ref['done'])
    assert not np.array_equal(obs[2, 3], obs[1, 3])


# ---- 4. the step loop against the restatement and against the fused path ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('env', list(SHAPES))
def test_step_loop_against_restatement_and_fused(env, mode):
    B, T = 17, 11
    ref = reference(env, B, T, mode)
    assert z_clear(env, ref)
    (obs, rew, done), kernel, _ = run(env, B, T, mode, force_step_loop=True)
    assert kernel == 'step-loop'
    assert_follows("%s %s step loop" % (env, mode), (obs, rew), ref)
    assert np.array_equal(done, ref['done'])
    (f_obs, f_rew, f_done), f_kernel, _ = run(env, B, T, mode)
    assert f_kernel == 'fused'
    print("%s %s fused vs step loop: obs %.3g rew %.3g absolute" % (env, mode, np.abs(f_obs[:11] - obs[:11]).max(), np.abs(f_rew[:10] - rew[:10]).max()))
    np.testing.assert_allclose(f_obs[:11], obs[:11], **TOL.CROSS_KERNEL)             # rows t <= 10
    np.testing.assert_allclose(f_rew[:10], rew[:10], **TOL.CROSS_KERNEL)             # rewards of steps 1 .. 10
    assert np.array_equal(f_done, done)


# ---- 5. off-table shapes take the step loop and are Engine.step chained, bit for bit ------------------------------------------------------------------------
OFF_TABLE = [('wide', 'swimmer', 5, (128, 128), (32, 32), 'model_mean'), ('K9', 'swimmer', 9, (64, 64), (32, 32), 'model_mean'),
             ('humanoid', 'humanoid', 5, (1024, 1024), (100, 50, 25), 'eps_rand'),
             ('step_rand', 'swimmer', 5, (64, 64), (32, 32), 'step_rand'), ('model_mean_std', 'swimmer', 5, (64, 64), (32, 32), 'model_mean_std'),
             ('model_med', 'swimmer', 5, (64, 64), (32, 32), 'model_med')]


@pytest.mark.parametrize('name,env,K,dh,ph,sam', OFF_TABLE, ids=[c[0] for c in OFF_TABLE])
def test_off_table_shapes_are_the_chained_step(name, env, K, dh, ph, sam):
    B, T = 17, 3
    if (env, K, dh) == ('swimmer',) + SHAPES['swimmer'][:2]:
        eng, dm = problem('swimmer')[:2]
        pool = problem('swimmer')[4]
    else:
        eng, dm, _, _, pool = Hh.make_engine(env, K, dh, ph, seed=11, n_pool=32)
    rng = np.random.RandomState(5)
    init = pool[rng.randint(len(pool), size=B)].astype(np.float32)
    actions = (1.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    heads = rng.randint(K, size=B)
    model_idx = rng.randint(K, size=(T, B)) if sam == 'step_rand' else None
    noise = rng.randn(T, B, dm.ns).astype(np.float32) if sam == 'model_mean_std' else None
    obs, rew, done = eng.rollout_actions(init, actions, sam_mode=sam, model=(torch.as_tensor(heads, dtype=torch.int32) if sam == 'eps_rand' else None),
                                         model_idx=model_idx, noise=noise)
    assert eng.last_rollout_actions_kernel() == 'step-loop'
    s = torch.as_tensor(init, device=eng.device)
    assert torch.equal(obs[0], s)
    for t in range(T):
        idx = model_idx[t] if sam == 'step_rand' else (heads if sam == 'eps_rand' else None)
        s, r, d = eng.step(s, actions[t], sam, model_idx=idx, noise=(noise[t] if noise is not None else None))
        assert torch.equal(obs[t + 1], s) and torch.equal(rew[t], r) and torch.equal(done[t], d), "%s: step %d differs from Engine.step" % (name, t)
    assert torch.isfinite(obs).all()
    if name == 'humanoid':                                      # uniform_model on the step loop: the ctx-owned head vector
        u_obs, u_rew, _ = eng.rollout_actions(init, actions, sam_mode='eps_rand', model=K - 1)
        s = torch.as_tensor(init, device=eng.device)
        for t in range(T):
            s, r, d = eng.step(s, actions[t], 'eps_rand', model_idx=np.full(B, K - 1))
            assert torch.equal(u_obs[t + 1], s) and torch.equal(u_rew[t], r)


# ---- 6. teacher forcing closes the loop: the policy rollout's own actions replayed -------------------------------------------------------------------------
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_replaying_a_policy_rollout_reproduces_it(env):
    B, T = 33, 10
    eng, dm, theta, pdims, pool = problem(env)
    init = pool[:B].astype(np.float32)
    # the float64 restatement of that rollout: no done (Ant would be reset from the pool, the replay would not) and z clear of the thresholds
    s = init.astype(np.float64)
    for t in range(T):
        s = np.mean(O.dynamics_forward_all(dm, s, np.clip(O.policy_mean(theta, pdims, s), -1, 1)), axis=0)
        assert not np.any(O.is_done(env, s, s)) and z_clear(env, dict(obs=np.stack([s, s])))
    dev = eng.device
    resume = (torch.as_tensor(init, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    tr = eng.rollout(B, T, T + 1, 'model_mean', init, determ=True, resume=resume)
    obs, rew, done = eng.rollout_actions(init, tr.act, 'model_mean')
    assert eng.last_rollout_actions_kernel() == 'fused'
    r_obs = np.concatenate([cpu(tr.obs), cpu(tr.last_obs)[None]], axis=0)
    print("%s replay vs rollout (%s): obs %.3g rew %.3g absolute" % (env, eng.last_rollout_kernel(), np.abs(cpu(obs) - r_obs).max(),
                                                                     np.abs(cpu(rew) - cpu(tr.rew)).max()))
    np.testing.assert_allclose(cpu(obs), r_obs, **TOL.CROSS_KERNEL)
    np.testing.assert_allclose(cpu(rew), cpu(tr.rew), **TOL.CROSS_KERNEL)
    assert np.array_equal(cpu(done), cpu(tr.done)) and not cpu(done).any()


# ---- 7. the model diagnostic runs on it ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', [-1, 4])
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_model_error_known_actions_is_open_loop_predictions(env, model):
    """metrpo_model_error(known_actions) = one gather + the body of metrpo_rollout_actions + k_pred_error.  open_loop_predictions from the same window
    starts with the same gathered actions is the same kernel on the same inputs at the same batch positions, and k_pred_error's arithmetic is
    pred_error_np's (tests/test_gpu_model_error.py, held bit for bit there): the diagnostic's outputs follow bit for bit."""
    import test_gpu_model_error as TM
    from metrpo_amd import model_error as M
    eng, dm, theta, pdims, pool, Os, As, Rs = TM.problem(env)
    n, T, hs = TM.N_TRAJ, TM.T_REC, list(TM.TIMESTEPS)
    hmax = hs[-1]
    eng.rollout(64, 2, 3, 'step_rand', pool.astype(np.float32), seed=1)
    kernel_before, note_before = eng.last_rollout_kernel(), eng.rollout_note()
    r = M.model_error(eng, Os, As, Rs, hs, model=model, known_actions=True)
    assert eng.last_rollout_actions_kernel() == 'fused'
    assert eng.last_rollout_kernel() == kernel_before and eng.rollout_note() == note_before
    i, t = np.divmod(np.arange(n * T), T)
    starts = Os[i, t]
    acts = np.stack([As[i, np.minimum(t + s, T - 1)] for s in range(hmax)], axis=1)       # [W, hmax, na]
    states, costs, done = M.open_loop_predictions(eng, starts, acts, model=model)
    assert states.shape == (n * T, hmax + 1, dm.ns) and costs.shape == (n * T, hmax) and done.shape == (n * T, hmax)
    obs = np.ascontiguousarray(cpu(states).transpose(1, 0, 2)); rew = np.ascontiguousarray(-cpu(costs).T); dn = np.ascontiguousarray(cpu(done).T)
    sd, cd, va = TM.pred_error_np(obs[:hmax], rew, dn, obs[hmax], Os, Rs, hs, n, T)
    assert np.array_equal(cpu(r['valid']).astype(bool), va)
    assert np.array_equal(cpu(r['state_diff']).view(np.uint32), sd.view(np.uint32))
    assert np.array_equal(cpu(r['cost_diff']).view(np.uint32), cd.view(np.uint32))
    if env == 'ant':
        assert dn.any() and not va[:, 1 * T + 3].any()                                     # the planted window (trajectory 1, t = 3) is done at once


def test_a_known_actions_call_changes_nothing_else():
    """tests/test_gpu_model_error.py::test_a_call_changes_nothing_else for the new path and for the entry point itself, plus metrpo_last_rollout_kernel."""
    import test_gpu_model_error as TM
    from metrpo_amd import model_error as M
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
    assert eng.last_rollout_actions_kernel() is None
    M.model_error(eng, Os, As, Rs, list(TM.TIMESTEPS), model=0, known_actions=True)
    acts = (1.5 * rng.randn(5, 40, dm.na)).astype(np.float32)
    for force in (False, True):
        eng.rollout_actions(pool[:40].astype(np.float32), acts, 'model_mean', force_step_loop=force)
        eng.rollout_actions(pool[:40].astype(np.float32), acts, 'eps_rand', model=2, force_step_loop=force)
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note
    t2 = roll()                                                                           # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


# ---- 8. host function and the ABI's argument checks -------------------------------------------------------------------------------------------------------------
def test_open_loop_predictions_host():
    import metrpo_amd
    eng, dm, _, _, pool = problem('swimmer')
    init, actions, _ = inputs('swimmer', 17, 11)
    states, costs, done = metrpo_amd.open_loop_predictions(eng, init, actions.transpose(1, 0, 2), model=-1)      # trajectory-major in and out
    ref = reference('swimmer', 17, 11, 'mean')
    assert_follows("open_loop_predictions", (cpu(states).transpose(1, 0, 2), -cpu(costs).T), ref)
    assert not cpu(done).any()
    with pytest.raises(ValueError, match=r'initial_states: expected \[n, 10\]'):
        metrpo_amd.open_loop_predictions(eng, init[:, :9], actions.transpose(1, 0, 2))
    with pytest.raises(ValueError, match=r'actions: expected \[17, T, 2\]'):
        metrpo_amd.open_loop_predictions(eng, init, actions)                                                      # time-major by mistake
    with pytest.raises(ValueError, match='model = 5'):
        metrpo_amd.open_loop_predictions(eng, init, actions.transpose(1, 0, 2), model=5)


def test_abi_argument_errors():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    eng, dm, _, _, pool = problem('swimmer')
    dev = eng.device
    B, T, ns, na = 4, 2, dm.ns, dm.na
    f = lambda *s: torch.full(s, 555.0, dtype=torch.float32, device=dev)
    init, act, obs, rew = torch.zeros(B, ns, device=dev), torch.zeros(T, B, na, device=dev), f(T + 1, B, ns), f(T, B)      # outputs hold a sentinel
    done = torch.full((T, B), 0xCD, dtype=torch.uint8, device=dev)
    idx = torch.zeros(T, B, dtype=torch.int32, device=dev)

    def args(**kw):
        a = _lib.RolloutActionsArgs()
        a.B, a.T, a.sam_mode, a.uniform_model = B, T, _lib.SAM_MODES['model_mean'], -1
        a.d_init_obs, a.d_actions, a.d_obs, a.d_rew, a.d_done = init.data_ptr(), act.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.metrpo_rollout_actions(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_rollout_actions(None, C.byref(args()), eng._stream()) == -2 and lib.metrpo_last_rollout_actions_kernel(None) == -2
    assert lib.metrpo_rollout_actions(eng._ctx, None, eng._stream()) == -2 and b'args NULL' in err()
    for name in ('d_init_obs', 'd_actions', 'd_obs', 'd_rew', 'd_done'):
        assert call(args(**{name: None})) == -2 and b'required pointer' in err()           # METRPO_ENULL
    assert call(args(B=-1)) == -1 and b'bad B/T' in err()                                  # METRPO_EINVAL
    assert call(args(T=-1)) == -1 and b'bad B/T' in err()
    for bad in (-1, 6):
        assert call(args(sam_mode=bad)) == -1 and b'sam mode is not defined' in err()
    assert call(args(sam_mode=_lib.SAM_MODES['eps_rand'])) == -2 and b'eps_rand needs d_model' in err()
    assert call(args(sam_mode=_lib.SAM_MODES['eps_rand'], uniform_model=5)) == -1 and b'uniform_model = 5' in err()
    assert call(args(uniform_model=-2)) == -1 and b'uniform_model = -2' in err()
    assert call(args(sam_mode=_lib.SAM_MODES['step_rand'])) == -2 and b'd_model_idx required' in err()
    assert call(args(sam_mode=_lib.SAM_MODES['model_mean_std'])) == -2 and b'd_sel_noise required' in err()
    # B == 0 or T == 0: OK, nothing written -- not even with NULL pointers, which are not looked at
    for kw in (dict(B=0), dict(T=0), dict(B=0, d_obs=None)):
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert torch.all(obs == 555.0) and torch.all(rew == 555.0) and torch.all(done == 0xCD)
    # per-mode inputs present: accepted (eps_rand with either form; step_rand goes to the step loop)
    assert call(args(sam_mode=_lib.SAM_MODES['eps_rand'], uniform_model=4)) == 0 and eng.last_rollout_actions_kernel() == 'fused'
    assert call(args(sam_mode=_lib.SAM_MODES['eps_rand'], d_model=idx.data_ptr())) == 0 and eng.last_rollout_actions_kernel() == 'fused'
    assert call(args(sam_mode=_lib.SAM_MODES['step_rand'], d_model_idx=idx.data_ptr())) == 0 and eng.last_rollout_actions_kernel() == 'step-loop'
    torch.cuda.synchronize()
    assert not torch.any(obs == 555.0)
    # dynamics must be set, the policy need not be
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_rollout_actions(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_rollout_actions_kernel() is None
    bare.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    o2, r2, d2 = bare.rollout_actions(init, act, 'model_mean')                             # no metrpo_set_policy: theta is never read
    o1, r1, d1 = eng.rollout_actions(init, act, 'model_mean')
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
