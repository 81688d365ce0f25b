"""GPU tests of the model diagnostics: metrpo_model_error / metrpo_model_error_windows (csrc/model_error.hip) and the host functions
metrpo_amd.evaluate_model_predictions / get_error_distribution (env_helpers.py:96-172, :175-269) against tests/model_error_ref.py.

Bounds.  States and costs of the end-to-end cases are held to the rows DESIGN.md section 6 / tests/tolerances.py grant a free-running rollout of
the same kernel family: FREE_RUN (rtol 1e-5, atol 1e-6; tolerances.py:28, "t <= 10 ... keeps the single-step figure") for the state after h <= 10
steps and the reward of a step t <= 10, LONG_RUN (rtol 1e-4, atol 1e-5; tolerances.py:31, "beyond t = 10 ... 10x the single-step figure") beyond.
The diagnostic's outputs are functions of those: state_diff = |real - pred| carries pred's bound plus the subtraction's rounding
2^-24 |state_diff|; cost_diff = |costs + rewards| carries the sum of the per-step reward bounds, plus the two sequential fp32 sums of h terms
((h - 1) 2^-24 (sum |c_s| + sum |R_s|)), plus the last addition's rounding 2^-24 |costs + rewards|.  Nothing is measured on the new code."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import model_error_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
SHAPES = [(9, 7), (5, 13), (1, 257)]                    # W = n T = 63, 65, 257: one short of a wave, one over a wave, one over a workgroup
ENVS_NS = [('swimmer', 10), ('ant', 29)]


def cpu(t):
    return t.detach().cpu().numpy()


_engines = {}


def bare_engine(env):
    """An engine for the entry points that read neither the dynamics nor the policy (window gather, caller-made trajectory)."""
    import metrpo_amd
    if env not in _engines:
        _engines[env] = metrpo_amd.Engine(env, 2, (16, 16), (8, 8))
    return _engines[env]


# ---- 1. the comparison kernel alone, bit for bit ---------------------------------------------------------------------------------------------------------
def pred_error_np(obs, rew, done, last, Os, Rs, hs, n, T):
    """k_pred_error in NumPy fp32 on the same arrays: every output is one fp32 subtraction or an in-order fp32 sum."""
    W, ns, hmax = n * T, Os.shape[2], hs[-1]
    i, t = np.divmod(np.arange(W), T)
    costs, rewards, dead = np.zeros(W, np.float32), np.zeros(W, np.float32), np.zeros(W, bool)
    sd, cd, va = [], [], []
    for s in range(hmax):
        costs = (costs - rew[s]).astype(np.float32)
        m = t + s < T
        rewards[m] = (rewards[m] + Rs[i[m], t[m] + s]).astype(np.float32)
        dead |= done[s] != 0
        h = s + 1
        if h in hs:
            v = (t + h <= T) & ~dead
            pred = obs[h] if h < hmax else last
            real = Os[i, np.minimum(t + h, T)]
            sd.append(np.where(v[:, None], np.abs(real - pred), np.float32(0)).astype(np.float32))
            cd.append(np.where(v, np.abs(costs + rewards), np.float32(0)).astype(np.float32))
            va.append(v)
    return np.stack(sd), np.stack(cd), np.stack(va)


@pytest.mark.parametrize('n,T', SHAPES)
@pytest.mark.parametrize('env,ns', ENVS_NS)
def test_comparison_kernel_is_exact(env, ns, n, T):
    """Random fp32 trajectory through the caller-made-trajectory path of metrpo_model_error.  hs holds 1, an inner horizon and T itself (= hmax: the
    last row comes from d_last_obs).  Planted: a done at step h - 1 drops the window from h on, a done at step h does not drop it from h.
    d_sums: float64 sums of non-negative addends in a fixed order against the exactly rounded sum (math.fsum).  Adding a zero is exact, so the
    summation tree pruned of zeros has n_add leaves and no addend passes through more than n_add - 1 inexact additions, each of relative error
    <= 2^-53 of a partial sum that never exceeds the total: |got - exact| <= (n_add - 1) 2^-53 total, plus half an ulp for fsum's own rounding:
    <= n_add 2^-53 relative.  n_add = count for the cost and last-column sums: the bound asserted, count 2^-53.  The state sum adds count * ns
    values, so what the argument proves for it is count * ns * 2^-53; it is held to the tighter count 2^-53 all the same (the kernel's order is
    fixed, so a pass is not luck of the run).  The count itself is exact."""
    from metrpo_amd import model_error as M
    eng = bare_engine(env)
    assert eng.ns == ns
    W = n * T
    hin = 3 if T < 100 else 100
    hs = [1, hin, T]
    rng = np.random.RandomState(1000 * ns + W)
    f = lambda *s: rng.randn(*s).astype(np.float32)
    Os, Rs = f(n, T + 1, ns), f(n, T)
    obs, rew, last = f(T, W, ns), f(T, W), f(W, ns)
    done = (rng.rand(T, W) < 0.02).astype(np.uint8)
    done[:, ::T] = 0                                    # the t = 0 windows, the only ones that serve h = T, stay alive
    w_a, w_b = 1, (n - 1) * T + 2                       # t = 1 of the first trajectory, t = 2 of the last: both serve 1 and hin
    done[:, [w_a, w_b]] = 0
    done[hin - 1, w_a] = 1                              # step h - 1: dropped from h = hin on
    done[hin, w_b] = 1                                  # step h: still serves h = hin, dropped above
    r = M.model_error(eng, Os, None, Rs, hs, trajectory=(obs, rew, done, last))
    sd, cd, va = pred_error_np(obs, rew, done, last, Os, Rs, hs, n, T)
    g_sd, g_cd, g_va, g_sums = cpu(r['state_diff']), cpu(r['cost_diff']), cpu(r['valid']), cpu(r['sums'])
    assert va[0, w_a] and not va[1, w_a] and not va[2, w_a]
    assert va[0, w_b] and va[1, w_b] and not va[2, w_b]
    assert np.array_equal(g_va.astype(bool), va)
    assert np.array_equal(g_sd.view(np.uint32), sd.view(np.uint32))
    assert np.array_equal(g_cd.view(np.uint32), cd.view(np.uint32))
    # hmax < T: the same two first horizons from a trajectory that ends at hin, whose row hin is d_last_obs
    r2 = M.model_error(eng, Os, None, Rs, hs[:2], trajectory=(obs[:hin], rew[:hin], done[:hin], obs[hin]))
    assert np.array_equal(cpu(r2['state_diff']).view(np.uint32), sd[:2].view(np.uint32)) and np.array_equal(cpu(r2['cost_diff']).view(np.uint32), cd[:2].view(np.uint32))
    assert np.array_equal(cpu(r2['valid']).astype(bool), va[:2]) and np.array_equal(cpu(r2['sums']), g_sums[:2])
    for p, h in enumerate(hs):
        count = int(va[p].sum())
        assert count > 0 and g_sums[p, 0] == count
        assert count <= n * (T + 1 - h)
        for col, (vals, n_add) in enumerate([(sd[p][va[p]].ravel(), count), (sd[p][va[p]][:, -1], count), (cd[p][va[p]], count)], start=1):
            exact = math.fsum(float(x) for x in vals)
            err = abs(g_sums[p, col] - exact)
            print("sums[%d][%d] h=%d: rel err %.3g of bound %.3g" % (p, col, h, err / exact, n_add * U64))
            assert err <= n_add * U64 * exact


# ---- 2. the window gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,T', SHAPES)
@pytest.mark.parametrize('env,ns', ENVS_NS)
def test_window_gather(env, ns, n, T):
    from metrpo_amd import model_error as M
    eng = bare_engine(env)
    Os = np.random.RandomState(n * T + ns).randn(n, T + 1, ns).astype(np.float32)
    got = cpu(M.model_error_windows(eng, Os))
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(Os[:, :-1]).reshape(-1, ns).view(np.uint32))


# ---- 3. end to end against the restatement -----------------------------------------------------------------------------------------------------------------
N_TRAJ, T_REC, TIMESTEPS = 3, 12, (1, 3, 5, 12)
SEEDS = {'swimmer': 1, 'ant': 1}             # ant: the restatement keeps every t = 0 window at h = 12 and every z stays 0.09 clear of the thresholds
_problems = {}


def problem(env):
    """Engine (K = 5, 2x64 dynamics, 2x32 policy), the fp32-rounded float64 problem and the recorded trajectories, built once per env."""
    if env not in _problems:
        dm, theta, pdims, pool = Hh.problem_data(env, 5, (64, 64), (32, 32), seed=SEEDS[env], n_pool=64)
        dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
        pool = pool.astype(np.float32).astype(np.float64)
        eng = Hh.engine_of(env, 5, (64, 64), (32, 32), dm, theta)
        Os, As, Rs = R.recorded_trajectories(dm, theta, pdims, env, pool, N_TRAJ, T_REC, seed=SEEDS[env])
        if env == 'ant':                                 # two window starts outside the healthy range 0.2 <= z <= 1.0: done at their first step
            Os[1, 3, 2] = 1.2; Os[2, 7, 2] = 0.1
        _problems[env] = (eng, dm, theta, pdims, pool, Os, As, Rs)
    return _problems[env]


_refs = {}


def reference(env, model, known):
    key = (env, model, known)
    if key not in _refs:
        eng, dm, theta, pdims, pool, Os, As, Rs = problem(env)
        _refs[key] = R.evaluate_model_predictions(dm, theta, pdims, env, Os, Rs, timesteps=TIMESTEPS, model=model, As=As, known_actions=known)
    return _refs[key]


def row_of_step(t):
    """tests/tolerances.py: FREE_RUN for t <= 10 (line 28), LONG_RUN beyond (line 31)."""
    return TOL.FREE_RUN if t <= 10 else TOL.LONG_RUN


def bounds(e, h):
    """Element bounds on state_diff [N, ns] and cost_diff [N] of one horizon from the restatement's own arrays (module docstring)."""
    row = row_of_step(h)
    b_state = row['atol'] + row['rtol'] * np.abs(e['pred']) + U32 * e['state_diff']
    c, r = np.abs(e['step_costs']), np.abs(e['step_rewards'])
    b_cost = sum(row_of_step(s + 1)['atol'] + row_of_step(s + 1)['rtol'] * c[s] for s in range(h))
    b_cost = b_cost + (h - 1) * U32 * (c.sum(axis=0) + r.sum(axis=0)) + U32 * e['cost_diff']
    return b_state, b_cost


def z_margin_ok(env, dm, theta, pdims, Os, Rs, As, model, known, margin=1e-4):
    """Ant: no kept window's predicted z comes within `margin` of the 0.2 / 1.0 thresholds at a step that decides a horizon -- else a float32 and a
    float64 rollout may disagree on `done`, which is no error of either."""
    if env != 'ant':
        return True
    n, T = Rs.shape
    s = np.reshape(Os[:, :-1].astype(np.float64), (-1, dm.ns))
    alive = np.ones(len(s), bool)
    i, t = np.divmod(np.arange(len(s)), T)
    ok = True
    for step in range(T):
        a = np.reshape(As.astype(np.float64)[i, np.minimum(t + step, T - 1)], (-1, dm.na)) if known else O.policy_mean(theta, pdims, s)
        with np.errstate(all='ignore'):
            s = R.forward(dm, model, s, np.clip(a, -1, 1))
        serving = alive & (t + step + 1 <= T)
        z = s[serving, 2]
        ok = ok and bool(np.all(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) > margin))
        alive &= ~np.asarray(O.is_done(env, s, s), bool)
    return ok


@pytest.mark.parametrize('known', [False, True], ids=['policy', 'known_actions'])
@pytest.mark.parametrize('model', [-1, 0, 4])
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_end_to_end_against_the_restatement(env, model, known):
    from metrpo_amd import model_error as M
    eng, dm, theta, pdims, pool, Os, As, Rs = problem(env)
    ref = reference(env, model, known)
    assert z_margin_ok(env, dm, theta, pdims, Os, Rs, As, model, known)
    r = M.model_error(eng, Os, As, Rs, list(TIMESTEPS), model=model, known_actions=known)
    g_sd, g_cd, g_va, g_sums = cpu(r['state_diff']), cpu(r['cost_diff']), cpu(r['valid']).astype(bool), cpu(r['sums'])
    if not known:
        assert eng.last_rollout_kernel() == 'mfma-cooperative'          # the rollout went through metrpo_rollout's dispatch: K = 5, 2x64 + 2x32
    for p, h in enumerate(TIMESTEPS):
        e = ref['per_h'][p]
        w = e['i'] * T_REC + e['t']                                       # the restatement's windows in the device's numbering
        serves = np.zeros(N_TRAJ * T_REC, bool); serves[w[e['keep']]] = True
        assert np.array_equal(g_va[p], serves)
        if env == 'ant' and h == 12:                                      # a kernel that drops everything cannot pass
            assert e['keep'].sum() >= 0.75 * len(e['keep']) and g_va[p].sum() == e['keep'].sum()
        if env == 'ant' and h <= 5:
            assert ref['dropped'][p] >= 2                                 # ... and the two planted windows (t = 3 and t = 7) are dropped where they would serve
        k = e['keep']
        b_state, b_cost = bounds(e, h)
        d_state = np.abs(g_sd[p][w[k]].astype(np.float64) - e['state_diff'][k])
        d_cost = np.abs(g_cd[p][w[k]].astype(np.float64) - e['cost_diff'][k])
        print("%s model %d %s h=%d: state %.3g, cost %.3g of their bounds" % (env, model, 'known' if known else 'policy', h,
                                                                            (d_state / b_state[k]).max(), (d_cost / b_cost[k]).max()))
        assert np.all(d_state <= b_state[k]) and np.all(d_cost <= b_cost[k])
        assert not g_sd[p][~serves].any() and not g_cd[p][~serves].any()  # zero where the window does not serve
        cnt = int(k.sum())
        assert g_sums[p, 0] == cnt
        # the sums are the device's own arrays added in float64 (test 1 holds the order's rounding)
        np.testing.assert_allclose(g_sums[p, 1:], [g_sd[p].astype(np.float64).sum(), g_sd[p][:, -1].astype(np.float64).sum(),
                                                   g_cd[p].astype(np.float64).sum()], rtol=cnt * dm.ns * U64 * 2, atol=0)


# ---- 4. host functions ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_evaluate_model_predictions_host(env, tmp_path):
    import metrpo_amd
    eng, dm, theta, pdims, pool, Os, As, Rs = problem(env)
    ref = reference(env, -1, False)
    with pytest.warns(UserWarning, match=r'horizons \[15, 100\] exceed the recorded length T = 12'):
        err = metrpo_amd.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(1, 3, 5, 12, 15, 100), model=-1, log_dir=str(tmp_path), count=7)
    assert set(err) == {'timesteps', 'l2_sum', 'l1_sum', 'l1_state_cost', 'state_diff', 'cost_diff', 'dropped'}
    assert err['timesteps'] == TIMESTEPS and err['dropped'] == ref['dropped']
    for key in ('l2_sum', 'l1_sum', 'l1_state_cost', 'dropped'):
        assert len(err[key]) == len(TIMESTEPS)
    assert err['l2_sum'] == err['l1_sum']                                  # env_helpers.py:163
    for which in ('state_diff', 'cost_diff'):
        assert set(err[which]) == set(R.STAT_KEYS)
        assert all(len(v) == len(TIMESTEPS) for v in err[which].values())
        assert err[which]['batch_size'] == ref[which]['batch_size']
    for p, h in enumerate(TIMESTEPS):
        e = ref['per_h'][p]
        b_state, b_cost = bounds(e, h)
        bs, bc = b_state[e['keep']].max(axis=0), b_cost[e['keep']].max()   # an order statistic or a mean moves by at most the largest element error
        for key in ('0%', '25%', '50%', '75%', '100%', 'avg'):
            assert err['state_diff'][key][p].shape == (dm.ns,)
            assert np.all(np.abs(err['state_diff'][key][p] - ref['state_diff'][key][p]) <= bs)
            assert abs(err['cost_diff'][key][p] - ref['cost_diff'][key][p]) <= bc
        assert abs(err['l1_sum'][p] - ref['l1_sum'][p]) <= bs.sum()
        assert abs(err['l1_state_cost'][p] - ref['l1_state_cost'][p]) <= bs[-1]
    for which in ('state_diff', 'cost_diff'):                              # write_to_csv's format (env_helpers.py:71-81) parses back
        with open(os.path.join(str(tmp_path), '%s_7.csv' % which), newline='') as fh:
            rows = list(csv.reader(fh))
        assert rows[0] == ['timesteps'] + sorted(R.STAT_KEYS) and [r[0] for r in rows[1:]] == [str(h) for h in TIMESTEPS]
        col = rows[0].index('batch_size')
        assert [int(r[col]) for r in rows[1:]] == err[which]['batch_size']
        col = rows[0].index('avg')
        for p, r in enumerate(rows[1:]):
            back = np.array(r[col].strip('[]').split(), np.float64)
            np.testing.assert_allclose(back, np.ravel(err[which]['avg'][p]), rtol=5.1e-9, atol=5.1e-9)     # str() of an array keeps 8 digits


@pytest.mark.parametrize('known', [False, True], ids=['policy', 'known_actions'])
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_get_error_distribution_is_the_t0_rows(env, known):
    """At horizon = T the function's windows are the t = 0 windows of the T-step pass of case 3: |e_state| and |e_cost| are that pass's rows
    (within twice the rows' bounds: two runs of the same arithmetic at different batch positions), and the signed values the restatement's."""
    import metrpo_amd
    from metrpo_amd import model_error as M
    eng, dm, theta, pdims, pool, Os, As, Rs = problem(env)
    model, T = 4, T_REC
    real_costs = (-Rs.astype(np.float64).sum(axis=1)).astype(np.float32)
    e_cost, e_state = metrpo_amd.get_error_distribution(eng, Os[:, 0], As, real_costs, Os[:, T], T, model=model, known_actions=known)
    assert e_cost.shape == (N_TRAJ,) and e_state.shape == (N_TRAJ, dm.ns)
    rc, rs, keep = R.get_error_distribution(dm, theta, pdims, env, Os[:, 0], As, real_costs, Os[:, T], T, model=model, known_actions=known)
    e = reference(env, model, known)['per_h'][len(TIMESTEPS) - 1]           # h = 12 = T: one window per trajectory, t = 0
    assert np.array_equal(e['t'], np.zeros(N_TRAJ)) and np.array_equal(keep, e['keep']) and keep.any()
    assert np.array_equal(np.isnan(e_cost), ~keep) and np.array_equal(np.isnan(e_state).all(axis=1), ~keep)
    b_state, b_cost = bounds(e, T)
    b_cost = b_cost + U32 * np.abs(real_costs)                              # the real total enters as one fp32 value here
    assert np.all(np.abs(e_state[keep] - rs[keep]) <= b_state[keep]) and np.all(np.abs(e_cost[keep] - rc[keep]) <= b_cost[keep])
    full = M.model_error(eng, Os, As, Rs, list(TIMESTEPS), model=model, known_actions=known)
    sd, cd = cpu(full['state_diff'])[-1][::T], cpu(full['cost_diff'])[-1][::T]
    assert np.all(np.abs(np.abs(e_state[keep]) - sd[keep]) <= 2 * b_state[keep]) and np.all(np.abs(np.abs(e_cost[keep]) - cd[keep]) <= 2 * b_cost[keep])


# ---- 5. no side effects ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_else():
    from metrpo_amd import model_error as M
    _, dm, theta, pdims, pool, Os, As, Rs = problem('swimmer')
    eng = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)         # its own context: the optimizer steps below change the weights
    rng = np.random.RandomState(0)
    x = rng.randn(5 * 16, dm.ns + dm.na).astype(np.float32); y = rng.randn(5 * 16, dm.ns).astype(np.float32)
    eng.train_step(x, y, 16, 1e-3)                                          # non-zero moments and step counts in both optimizers
    eng.policy_adam_step(torch.as_tensor(rng.randn(eng.P), dtype=torch.float64, device=eng.device), 1e-3)
    state = lambda: [eng.get_policy().clone(), eng.get_dynamics().clone()] + [t.clone() if torch.is_tensor(t) else t for t in eng.get_train_adam()] + \
        [t.clone() if torch.is_tensor(t) else t for t in eng.get_policy_adam()]
    before = state()
    roll = lambda: eng.rollout(128, 6, 4, 'step_rand', pool.astype(np.float32), seed=5)
    t1 = roll()
    o1, r1, a1 = t1.obs.clone(), t1.rew.clone(), t1.act.clone()
    for known in (False, True):
        M.model_error(eng, Os, As, Rs, list(TIMESTEPS), model=0, known_actions=known)
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    t2 = roll()
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


# ---- 6. the ABI's argument checks --------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors():
    import ctypes as C
    from metrpo_amd import model_error as M, _lib
    eng, dm, theta, pdims, pool, Os, As, Rs = problem('swimmer')
    E = _lib.MetrpoError
    with pytest.raises(E, match='not sorted'):
        M.model_error(eng, Os, As, Rs, [3, 1])
    with pytest.raises(E, match='not sorted'):
        M.model_error(eng, Os, As, Rs, [1, 3, 3])
    with pytest.raises(E, match='h = 13 > T = 12'):
        M.model_error(eng, Os, As, Rs, [1, 13])
    with pytest.raises(E, match='horizons start at 1'):
        M.model_error(eng, Os, As, Rs, [0, 3])
    with pytest.raises(E, match='model = 5'):
        M.model_error(eng, Os, As, Rs, [1, 3], model=5)
    a = _lib.ModelErrorArgs()
    t = torch.zeros(16, device=eng.device)
    a.d_Os, a.d_Rs, a.n, a.T = t.data_ptr(), t.data_ptr(), 1, 1
    hs = (C.c_int32 * 1)(1)
    a.hs, a.n_h, a.model = hs, 1, -1
    assert _lib.lib.metrpo_model_error(eng._ctx, C.byref(a), eng._stream()) == -2      # NULL outputs: METRPO_ENULL
    assert b'NULL output' in _lib.lib.metrpo_last_error(eng._ctx)
    a.d_state_diff = a.d_cost_diff = a.d_valid = a.d_sums = t.data_ptr()
    for bad in (0, 33):
        a.n_h = bad
        assert _lib.lib.metrpo_model_error(eng._ctx, C.byref(a), eng._stream()) == -1  # no horizon / more than METRPO_MODEL_ERROR_MAX_HORIZONS
        assert b'n_h must be' in _lib.lib.metrpo_last_error(eng._ctx)
    a.n_h = 1
    a.d_dbg_obs = t.data_ptr()
    assert _lib.lib.metrpo_model_error(eng._ctx, C.byref(a), eng._stream()) == -1      # half a debug trajectory: METRPO_EINVAL
    a.d_dbg_obs = None; a.known_actions = 1
    assert _lib.lib.metrpo_model_error(eng._ctx, C.byref(a), eng._stream()) == -2      # known_actions without d_As
    assert _lib.lib.metrpo_model_error_windows(eng._ctx, None, 1, 1, None, eng._stream()) == -2
    assert _lib.lib.metrpo_model_error_windows(eng._ctx, C.c_void_p(t.data_ptr()), 0, 1, C.c_void_p(t.data_ptr()), eng._stream()) == -1
