"""The BPTT policy gradient (metrpo_bptt_grad, metrpo_bptt_grad_stochastic, metrpo_validation_cost on the same forward sweeps) per variable at the
tile edges of every sweep family: the fused MFMA sweeps on the exact and the zero-padded layout (bptt_mfma.hip), the GEMM-path sweeps
(det_gemm.hip), the generic sweeps at bs = 64 and bs = 32 (bptt.hip); B = 1 ... 129 around every 16 / 32 / 64 edge, T = 1, 2, 3, K = 1; with the
policy VJP on the fused 2 x 32, the generic and the GEMM-path gradient kernels.  All calls go through the C ABI.  Case table, kink guard and
references: tests/bptt_cases.py (checked on the CPU by tests/test_bptt_cases.py).  Bounds: the rows BPTT_COST and BPTT_GRAD_REL_L2 of
tests/tolerances.py on the whole vector, and tolerances.block_bound on every variable W_l, b_l, log_std.
That a case runs on the kernels it names is asserted from Engine.set_det_path's return value and from what the library notes of the VJP's launch
(Engine.last_update_launch), here and in test_cases_reach_every_instantiation.

Observed on an MI355X (worst share of each bound over the file, per sweep family): profiles/r11_bptt_edges.txt."""
import json
import os

import numpy as np
import pytest
import torch
import tolerances as TOL
import bptt_cases as U
from helpers import engine_of

pytestmark = pytest.mark.gpu
_ENGINES, _RAN, _WORST = {}, {}, {}
UPDATE_PATH = {'mfma': True, 'generic': False, 'gemm': 'gemm'}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def fresh_engine(case):
    dm, theta, _, _ = U.problem(case)
    return engine_of(case.env, case.K, case.dh, case.ph, dm, theta)


def engine_for(case):
    """One engine per (env, K, widths): the cases of a shape share it, select their sweep and VJP family and set their own theta."""
    key = (case.env, case.K, case.dh, case.ph)
    if key not in _ENGINES:
        _ENGINES[key] = fresh_engine(case)
    return _ENGINES[key]


def select(eng, case):
    assert eng.set_det_path(case.sweep != 'generic') == U.DET_PATH[case.sweep], case.id
    arg = UPDATE_PATH[case.vjp] if case.force else True
    # (not forced: True where the shape has fused update kernels -- the 100-50-25 ones included, which the VJP does not use -- else False)
    assert eng.set_update_path(arg) == (arg if case.force else (case.vjp == 'mfma' or case.ph == (100, 50, 25))), case.id


def run(eng, case, d):
    """The case's call -> (costs, grad, n_saturates or None, the VJP's noted launch), host float64."""
    eng.set_policy(d['th'])
    x0 = d['x0'].astype(np.float32)
    if case.stoch:
        c, g, n = eng.bptt_grad_stochastic(x0, case.T, case.gamma, noise=d['eps'].astype(np.float32), n_saturates=True)
        rep = eng.last_update_launch()
        return cpu(c), cpu(g), n.cpu().numpy(), rep
    c, g = eng.bptt_grad(x0, case.T, case.gamma)
    rep = eng.last_update_launch()
    return cpu(c), cpu(g), None, rep


def check_report(case, rep):
    assert rep['family'] == case.vjp and rep['op'] == 0, (case.id, rep)
    if case.vjp == 'mfma':
        assert rep['table'] == U.FUSED_ENVS.index(case.env), (case.id, rep)


def _note(family, row, share):
    _WORST.setdefault(family, {})
    _WORST[family][row] = max(_WORST[family].get(row, 0.0), float(share))
    if os.environ.get('METRPO_TOL_REPORT'):
        json.dump(_WORST, open(os.environ['METRPO_TOL_REPORT'] + '.bptt_edges', 'w'), indent=1, sort_keys=True)


@pytest.mark.parametrize('case', U.CASES, ids=[c.id for c in U.CASES])
def test_bptt_matches_float64_per_variable(case):
    d = U.case_data(case)
    assert d['accepted'] == case.B and d['replaced'] <= U.MAX_REPLACED * case.B and d['margin'] >= U.KINK_FACTOR
    rc, rg, rn = U.reference(d)
    eng = engine_for(case)
    select(eng, case)
    costs, g, nsat, rep = run(eng, case, d)
    check_report(case, rep)
    _RAN[case.id] = (U.DET_PATH[case.sweep], rep)
    na, fails = d['pdims'][-1], []

    def hold(name, share, what=''):
        _note(case.sweep, name, share)
        print('%s %s%s: %.3g of the bound' % (case.id, name, what, share))
        if not share <= 1.0:
            fails.append((name, what, share))

    assert np.all(np.isfinite(costs)) and np.all(np.isfinite(g)), case.id          # nothing non-finite from skipped steps or idle lanes
    hold('BPTT_COST', U.cost_use(costs, rc))
    if not case.stoch:                                          # the same forward sweep without the tape
        v = cpu(eng.validation_cost(d['x0'].astype(np.float32), case.T, case.gamma))
        if case.sweep == 'generic':
            np.testing.assert_allclose(v, costs, rtol=1e-6, atol=1e-7)
        else:
            np.testing.assert_allclose(v, costs, rtol=1e-12)
        assert np.all(g[-na:] == 0.0), case.id
    if case.variant == 'clipped':                               # the clip gate kills every mean adjoint
        assert not np.any(rg) and np.all(g == 0.0), (case.id, np.abs(g).max())
    else:
        whole, worst, where, ls = U.vector_use(g, rg, d['pdims'])
        hold('BPTT_GRAD_REL_L2', whole)
        hold('BPTT_GRAD_REL_L2 per block', worst, ' ' + str(where))
        if case.stoch:
            hold('BPTT_GRAD_REL_L2 log_std', ls)
            assert np.array_equal(nsat, rn), (case.id, np.abs(nsat - rn).sum())     # every saturating draw is clear of the clip (kink guard)
    if case.variant == 'ant_all' and case.T >= 2 and case.gamma == 1.0:           # only the t = 0 term, weight gamma^0, survives
        other = next(o for o in U.CASES if o.variant == 'ant_all' and (o.sweep, o.B, o.T, o.gamma) == (case.sweep, case.B, case.T, 0.97))
        c2 = cpu(eng.bptt_grad(d['x0'].astype(np.float32), case.T, other.gamma)[0])
        assert np.array_equal(c2, costs), (case.id, c2, costs)
    assert not fails, (case.id, fails)


def test_cases_reach_every_instantiation():
    """From the sweep path and the VJP launch each case of the table reported (those test_bptt_matches_float64_per_variable already ran in this
    process; the others are run here, without their references): every (sweep family, VJP family) pair of the table ran."""
    for case in U.CASES:
        if case.id not in _RAN:
            eng = engine_for(case)
            select(eng, case)
            rep = run(eng, case, U.case_data(case))[3]
            check_report(case, rep)
            _RAN[case.id] = (U.DET_PATH[case.sweep], rep)
    torch.cuda.synchronize()
    seen = {(c.sweep, _RAN[c.id][1]['family']) for c in U.CASES}
    assert seen == {(c.sweep, c.vjp) for c in U.CASES}, sorted(seen)
    assert {(p, r['family']) for p, r in _RAN.values()} == {(p, f) for p in (0, 1, 2) for f in ('mfma', 'generic', 'gemm')}
    assert {r['table'] for p, r in _RAN.values() if p == 1 and r['family'] == 'mfma'} == set(range(len(U.FUSED_ENVS)))
    assert any(r['family'] == 'gemm' for (p, r), c in ((_RAN[c.id], c) for c in U.CASES) if c.ph == (100, 50, 25))       # f3_active excludes the VJP
    rows = {r['nrows'] for p, r in _RAN.values() if r['family'] != 'gemm'}
    assert 1 in rows and max(rows) >= 2, sorted(rows)
    print('reached:', sorted({(c.sweep, r['family'], r['table'], r['pt'], r['nrows'], r['splits']) for c in U.CASES for p, r in [_RAN[c.id]]}))


# ---- whole-suite properties -------------------------------------------------------------------------------------------------------------------
def _case(sweep, B, T, stoch=False, variant='plain'):
    return next(c for c in U.CASES if (c.sweep, c.B, c.T, c.stoch, c.variant) == (sweep, B, T, stoch, variant) and not c.force and c.K == 2
                and c.gamma == 0.97 and (c.sweep, c.env, c.dh, c.ph, c.vjp) == U.LEAD[sweep])


@pytest.mark.parametrize('sweep', sorted(U.DET_PATH))
def test_workspace_reuse_is_bitwise(sweep):
    """launch_bptt_grad re-carves XS | WT | GM | out on every call and zeroes exactly nGM floats: a (17, 1) call after a (129, 3) one on the same
    context, and a (129, 3) call after a (17, 1) one (the second grows the workspace), give the bits of a fresh engine's call; so does the
    stochastic form after a deterministic call."""
    big, small, st = _case(sweep, 129, 3), _case(sweep, 17, 1), _case(sweep, 17, 1, stoch=True)
    alone = {}
    for c in (big, small, st):
        eng = fresh_engine(c); select(eng, c)
        alone[c.id] = run(eng, c, U.case_data(c))[:3]
    for first, second in ((big, small), (small, big), (big, st)):
        eng = fresh_engine(first); select(eng, first)
        run(eng, first, U.case_data(first))
        got = run(eng, second, U.case_data(second))[:3]
        for a, b in zip(got, alone[second.id]):
            assert (a is None and b is None) or np.array_equal(a, b), (first.id, second.id)


@pytest.mark.parametrize('sweep', sorted(U.DET_PATH))
@pytest.mark.parametrize('B', [17, 65])
def test_bitwise_repeatability(sweep, B):
    for c in (_case(sweep, B, 3), _case(sweep, B, 3, stoch=True)):
        eng = engine_for(c); select(eng, c)
        a, b = run(eng, c, U.case_data(c)), run(eng, c, U.case_data(c))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[2] is None or np.array_equal(a[2], b[2])), c.id


@pytest.mark.parametrize('shape', [s for s in U.SHAPES if s[0] != 'generic'], ids=lambda s: '%s-%s-%s' % (s[0], s[1], 'x'.join(map(str, s[2]))))
@pytest.mark.parametrize('B', [17, 65])
def test_fast_sweeps_agree_with_the_generic_sweeps(shape, B):
    """The MFMA and the GEMM-path sweeps against the generic sweeps on the same inputs, within the rows (tests/test_gpu_bptt.py: only B = 77)."""
    c = next(c for c in U.CASES if (c.sweep, c.env, c.dh, c.ph, c.vjp) == shape and (c.B, c.T, c.variant, c.K, c.gamma) == (B, 3, 'plain', 2, 0.97)
             and not c.stoch and not c.force)
    d = U.case_data(c)
    eng = engine_for(c); select(eng, c)
    cf, gf = run(eng, c, d)[:2]
    assert eng.set_det_path(False) == 0
    cg, gg = run(eng, c, d)[:2]
    assert U.cost_use(cf, cg) <= 1.0
    whole, worst, where, _ = U.vector_use(gf, gg, d['pdims'])
    assert whole <= 1.0 and worst <= 1.0, (c.id, whole, worst, where)
