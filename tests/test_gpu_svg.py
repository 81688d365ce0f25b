"""The 'svg' policy update on the device (metrpo_svg_grad, metrpo_svg_update, metrpo_last_svg_path; csrc/svg.hip) against the float64 restatement
tests/svg_ref.py on the cases of tests/svg_cases.py (checked on the CPU by tests/test_svg_cases.py): avg_grads['theta'] held to GRAD_REL_L2 on the
whole vector and to tolerances.block_bound on every variable, avg_grads['state'] to the same row, F_t and Pi_t per sample to 1e-5 of the sample
matrix's Frobenius norm against float64 Jacobians; the path every case ran on; the two Jacobian paths against each other; and the entry
points' contract: padding rows (NaN included) change no bit, repeated calls are bit-identical, a small call after a large one equals a fresh
context's, svg_grad leaves the context's state alone, svg_update is theta + float32(-lr) * float32(g) bit for bit, Ant and bad arguments are refused."""
import ctypes as C

import numpy as np
import pytest
import torch

import svg_cases as U
import svg_ref as R
import tolerances as TOL
from helpers import engine_of, problem_data

pytestmark = pytest.mark.gpu
_ENGINES, _OUT = {}, {}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def engine_for(case, fresh=False):
    key = (case.env, case.K, case.dh, case.ph, case.act, case.seed)
    if fresh or key not in _ENGINES:
        dm, theta, _, _ = U.problem(*key)
        eng = engine_of(case.env, case.K, case.dh, case.ph, dm, theta, dyn_act=case.act)
        if fresh:
            return eng
        _ENGINES[key] = eng
    return _ENGINES[key]


def run(eng, case, d, jacobians=True, obs=None, act=None):
    out = eng.svg_grad((d['obs'] if obs is None else obs).astype(np.float32), (d['act'] if act is None else act).astype(np.float32), d['lengths'],
                       model=case.model, gamma=case.gamma, path=case.path, chunk=case.chunk, jacobians=jacobians)
    return {k: cpu(v) for k, v in out.items()}


def device_result(case):
    if case.id not in _OUT:
        eng = engine_for(case)
        eng.set_policy(U.case_data(case)['theta'])
        _OUT[case.id] = (run(eng, case, U.case_data(case)), eng.last_svg_path())
    return _OUT[case.id]


@pytest.mark.parametrize('case', U.CASES, ids=[c.id for c in U.CASES])
def test_svg_matches_float64_per_variable(case):
    d = U.case_data(case)
    ref = U.reference(case)
    got, path = device_result(case)
    assert path == U.want_path(case), (case.id, path)
    na, lens, fails = d['pdims'][-1], d['lengths'], []

    def hold(name, share):
        print('%s %s: %.3g of the bound' % (case.id, name, share))
        if not share <= 1.0:
            fails.append((name, share))

    assert all(np.all(np.isfinite(v)) for v in got.values()), case.id
    assert np.all(got['theta'][-na:] == 0.0), case.id                            # log_std slots exactly 0
    whole, worst, where = U.vector_use(got['theta'], ref['theta'], d['pdims'])
    hold('GRAD_REL_L2', whole)
    hold('GRAD_REL_L2 per block (%s)' % where, worst)
    hold('GRAD_REL_L2 state', U.state_use(got['state'], ref['state']))
    hold('F per sample', U.jac_use(got['dyn_jac'], ref['dyn_jac'], lens))
    hold('Pi per sample', U.jac_use(got['pol_jac'], ref['pol_jac'], lens))
    for r in range(case.n):
        assert np.all(got['mean_adj'][r, lens[r]:] == 0.0), case.id             # rows at or behind len
    hold('mean adjoint', float(np.linalg.norm(got['mean_adj'] - ref['mean_adj']) / np.linalg.norm(ref['mean_adj'])) / TOL.GRAD_REL_L2)
    assert not fails, (case.id, fails)


PAIRS = [(c, U.BY_ID[c.id.replace('-generic-', '-gemm-')]) for c in U.CASES if c.path == 'generic']


@pytest.mark.parametrize('gen,gem', PAIRS, ids=[a.id for a, _ in PAIRS])
def test_the_two_paths_agree_within_the_row(gen, gem):
    d, ref = U.case_data(gen), U.reference(gen)
    (a, pa), (b, pb) = device_result(gen), device_result(gem)
    assert (pa, pb) == ('generic', 'gemm')
    assert np.linalg.norm(a['theta'] - b['theta']) <= TOL.GRAD_REL_L2 * np.linalg.norm(ref['theta'])
    for name, sl in U.blocks(d['pdims'])[:-1]:
        assert np.linalg.norm(a['theta'][sl] - b['theta'][sl]) <= TOL.block_bound(TOL.GRAD_REL_L2, ref['theta'][sl], ref['theta']), (gen.id, name)
    assert np.linalg.norm(a['state'] - b['state']) <= TOL.GRAD_REL_L2 * np.linalg.norm(ref['state'])
    assert np.array_equal(a['pol_jac'], b['pol_jac'])                            # Pi_t comes from one kernel on both paths


@pytest.mark.parametrize('path', ['generic', 'gemm'])
def test_reference_fixture_through_the_device(path):
    """tests/golden/svg_swimmer.npz: the reference's own svg_gradient (tests/golden/make_golden_svg.py), 2 x 16 head, 2 x 8 policy"""
    from conftest import load_golden, dm_from_golden
    d = load_golden('svg_swimmer')
    dm, pdims = dm_from_golden(d, 'swimmer'), [int(x) for x in d['pdims']]
    eng = engine_of('swimmer', int(d['K']), tuple(int(x) for x in d['dyn_hidden']), tuple(int(x) for x in d['pol_hidden']), dm, d['theta'])
    for j, gamma in enumerate(d['gammas']):
        g = eng.svg_grad(d['obs'].astype(np.float32), d['act'].astype(np.float32), d['lengths'], model=0, gamma=float(gamma), path=path)
        assert eng.last_svg_path() == path
        ref_t, ref_s = d['grad_theta_%d' % j], d['grad_state_%d' % j]
        whole, worst, where = U.vector_use(cpu(g['theta']), ref_t, pdims)
        print('fixture %s gamma %g: %.3g of GRAD_REL_L2, %.3g of the block bound (%s), state %.3g' % (path, gamma, whole, worst, where, U.state_use(cpu(g['state']), ref_s)))
        assert whole <= 1.0 and worst <= 1.0 and U.state_use(cpu(g['state']), ref_s) <= 1.0


RAGGED = 'swimmer-64x64-32x32-relu-n3T11-g0.97-m1-%s-c16'


@pytest.mark.parametrize('path', ['generic', 'gemm'])
def test_padding_rows_change_no_bit_and_repeated_calls_are_identical(path):
    case = U.BY_ID[RAGGED % path]
    d = U.case_data(case)
    eng = engine_for(case)
    eng.set_policy(d['theta'])
    a, b = run(eng, case, d), run(eng, case, d)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, 'repeated call')
    obs, act = d['obs'].copy(), d['act'].copy()
    for r, L in enumerate(d['lengths']):
        obs[r, L:], act[r, L:] = np.nan, np.nan
    assert np.isnan(obs).any()
    c = run(eng, case, d, obs=obs, act=act)
    for k in ('theta', 'state', 'mean_adj'):
        assert np.array_equal(a[k], c[k]), (k, 'NaN behind the lengths')
    for r, L in enumerate(d['lengths']):
        assert np.array_equal(a['dyn_jac'][r, :L], c['dyn_jac'][r, :L]) and np.array_equal(a['pol_jac'][r, :L], c['pol_jac'][r, :L])
    assert all(np.all(np.isfinite(v)) for v in c.values())


@pytest.mark.parametrize('path', ['generic', 'gemm'])
def test_small_call_after_large_equals_a_fresh_context(path):
    small = U.BY_ID['swimmer-64x64-32x32-relu-n3T2-g0.97-m2-%s-c0' % path]
    large = U.BY_ID['swimmer-64x64-32x32-relu-n5T11-g0.97-m0-%s-c0' % path]
    ds = U.case_data(small)
    used = engine_for(small, fresh=True)
    run(used, large, U.case_data(large))
    after = run(used, small, ds)
    fresh = run(engine_for(small, fresh=True), small, ds)
    for k in after:
        assert np.array_equal(after[k], fresh[k]), k


def test_svg_grad_leaves_the_context_state_alone():
    case = U.BY_ID[RAGGED % 'gemm']
    d = U.case_data(case)
    dm, theta, pdims, pool = U.problem(case.env, case.K, case.dh, case.ph, case.act, case.seed)
    eng = engine_for(case, fresh=True)
    eng.policy_adam_step(np.linspace(-1, 1, eng.P), 1e-3)                       # non-trivial Adam states on both sides
    x = np.random.RandomState(0).randn(64, dm.ns + dm.na).astype(np.float32)
    eng.train_step(x, x[:, :dm.ns] * 0.1, 32, 1e-3)
    traj = eng.rollout(16, 4, 3, 'eps_rand', pool.astype(np.float32), seed=5)
    before = [cpu(traj.obs), cpu(traj.act)]

    def state():
        pm, pv, pt = eng.get_policy_adam()
        dm_, dv, dt = eng.get_train_adam()
        return [cpu(eng.get_policy()), cpu(pm), cpu(pv), pt, cpu(dm_), cpu(dv), dt, cpu(eng.get_dynamics()), eng.last_rollout_kernel(), eng.rollout_note()]
    s0 = state()
    run(eng, case, d)
    s1 = state()
    for p, q in zip(s0, s1):
        assert np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q
    again = eng.rollout(16, 4, 3, 'eps_rand', pool.astype(np.float32), seed=5)  # the same Philox draws as before the call
    assert np.array_equal(before[0], cpu(again.obs)) and np.array_equal(before[1], cpu(again.act))


@pytest.mark.parametrize('path', ['generic', 'gemm'])
def test_svg_update_is_the_float32_sgd_step_bit_for_bit(path):
    case = U.BY_ID[RAGGED % path]
    d = U.case_data(case)
    eng = engine_for(case, fresh=True)
    th0 = eng.get_policy().cpu().numpy()
    g = run(eng, case, d, jacobians=False)['theta']
    lr = 0.037
    out = eng.svg_update(d['obs'].astype(np.float32), d['act'].astype(np.float32), lr, d['lengths'], model=case.model, gamma=case.gamma, path=case.path,
                         chunk=case.chunk)
    assert np.array_equal(cpu(out['theta']), g)                                  # the gradient the step used = svg_grad's
    th1 = eng.get_policy().cpu().numpy()
    want = R.svg_update(th0, g, lr)
    assert th1.dtype == np.float32 and np.array_equal(th1.view(np.uint32), want.view(np.uint32))
    na = d['pdims'][-1]
    assert np.array_equal(th1[-na:].view(np.uint32), th0[-na:].view(np.uint32)) and not np.array_equal(th1[:-na], th0[:-na])
    assert eng.last_svg_path() == path


def test_svg_class_and_early_stop_loop_move_the_policy():
    """SVG.svg_gradient = Engine.svg_grad on the packed triplets; early_stop.optimize_policy on an SVG object keeps an improving policy."""
    from metrpo_amd import SVG, rollout_triplets, early_stop
    case = U.BY_ID[RAGGED % 'gemm']
    d = U.case_data(case)
    eng = engine_for(case, fresh=True)
    data = rollout_triplets([d['Os'][r, :L + 1] for r, L in enumerate(d['lengths'])], [d['act'][r] for r in range(case.n)])
    assert [len(r) for r in data] == list(d['lengths'])
    svg = SVG(eng, learning_rate=1e-3, model=case.model, gamma=case.gamma)
    g = svg.svg_gradient(data)
    want = eng.svg_grad(d['obs'].astype(np.float32), d['act'].astype(np.float32), d['lengths'], model=case.model, gamma=case.gamma)
    assert np.array_equal(cpu(g['theta']), cpu(want['theta'])) and np.array_equal(cpu(g['state']), cpu(want['state']))
    th0 = cpu(eng.get_policy())
    res = early_stop.optimize_policy(svg, d['obs'][:, 0].astype(np.float32), 3, 1.0, mode='no_early', log_every=1, max_iters=2, init_pool=data)
    assert res['training_costs'] == [0.0, 0.0] and res['best_index'] == 2 and not np.array_equal(th0, cpu(eng.get_policy()))


def test_ant_and_bad_arguments_are_refused():
    from metrpo_amd import _lib
    lib = _lib.lib
    dm, theta, pdims, pool = problem_data('ant', 2, (64, 64), (32, 32), seed=1)
    ant = engine_of('ant', 2, (64, 64), (32, 32), dm, theta)
    with pytest.raises(_lib.MetrpoError, match='Ant'):
        ant.svg_grad(np.zeros((1, 2, dm.ns), np.float32), np.zeros((1, 2, dm.na), np.float32))
    case = U.BY_ID[RAGGED % 'gemm']
    eng = engine_for(case)
    dev = eng.device
    obs = torch.zeros(2, 3, eng.ns, device=dev); act = torch.zeros(2, 3, eng.na, device=dev); grad = torch.zeros(eng.P, dtype=torch.float64, device=dev)

    def call(**kw):
        a = _lib.SvgArgs()
        a.d_obs, a.d_act, a.d_grad, a.n, a.T, a.model, a.gamma = obs.data_ptr(), act.data_ptr(), grad.data_ptr(), 2, 3, 0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return (lib.metrpo_svg_grad(eng._ctx, C.byref(a), eng._stream()), lib.metrpo_svg_update(eng._ctx, C.byref(a), 0.1, eng._stream()))
    assert call() == (0, 0)
    for kw in (dict(n=0), dict(T=0), dict(model=-1), dict(model=eng.K), dict(path=3), dict(chunk=-1)):
        assert call(**kw) == (-1, -1), kw                                       # METRPO_EINVAL
    for kw in (dict(d_obs=None), dict(d_act=None), dict(d_grad=None)):
        assert call(**kw) == (-2, -2), kw                                       # METRPO_ENULL
    assert lib.metrpo_svg_grad(eng._ctx, None, eng._stream()) == -2
    tanh = U.BY_ID['hopper-32x32-32x32-tanh-n3T11-g0.97-m0-auto-c0']
    e2 = engine_for(tanh)
    with pytest.raises(_lib.MetrpoError, match='GEMM'):                          # a forced path the shape does not have is an error, not a fall-back
        e2.svg_grad(np.zeros((1, 2, e2.ns), np.float32), np.zeros((1, 2, e2.na), np.float32), path='gemm')
    torch.cuda.synchronize()
