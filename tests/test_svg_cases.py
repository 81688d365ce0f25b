"""CPU checks of the 'svg' case table (tests/svg_cases.py) that tests/test_gpu_svg.py runs on the device: every case's rollouts are clear of the
relu and cost kinks with no redraw beyond the cap, the float32-Jacobian / float64-scan restatement -- the form the device computes -- stays far
inside the bounds the GPU test holds (its share is printed), and deliberately wrong restatements miss those bounds by at least 10 x."""
import numpy as np
import pytest

import svg_cases as U
import svg_ref as R


@pytest.mark.parametrize('case', U.CASES, ids=[c.id for c in U.CASES])
def test_case_is_clear_of_kinks_and_float32_restatement_is_inside_the_bounds(case):
    d = U.case_data(case)
    assert d['replaced'] <= U.MAX_REPLACED * case.n, (case.id, d['replaced'])
    assert d['margin'] >= U.KINK_FACTOR
    assert U.want_path(case) in ('generic', 'gemm')
    r64, r32 = U.reference(case), U.reference(case, np.float32)
    assert np.all(np.isfinite(r64['theta'])) and np.linalg.norm(r64['theta']) > 0 and np.all(r64['theta'][-d['pdims'][-1]:] == 0.0)
    whole, worst, where = U.vector_use(r32['theta'], r64['theta'], d['pdims'])
    st = U.state_use(r32['state'], r64['state'])
    jf = U.jac_use(r32['dyn_jac'], r64['dyn_jac'], d['lengths'])
    jp = U.jac_use(r32['pol_jac'], r64['pol_jac'], d['lengths'])
    print('%s float32 share: grad %.3g, per block %.3g (%s), state %.3g, F %.3g, Pi %.3g' % (case.id, whole, worst, where, st, jf, jp))
    assert max(whole, worst, st, jf, jp) <= 0.5


def test_case_table_covers_what_the_gpu_test_claims():
    cs = U.CASES
    assert {c.env for c in cs} == {'swimmer', 'half_cheetah', 'hopper', 'snake', 'humanoid'}
    assert {c.n for c in cs} >= {1, 3, 5} and {c.T for c in cs} >= {1, 2, 11} and {c.gamma for c in cs} == {1.0, 0.97}
    assert any(c.model == 0 for c in cs) and any(c.model == c.K - 1 and c.K > 1 for c in cs)
    for dh in ((64, 64), (128, 128), (24, 16), (48, 48, 32)):
        assert {c.path for c in cs if c.dh == dh} >= {'generic', 'gemm'}, dh
    auto = {(c.dh, c.act, c.ph): U.want_path(c) for c in cs if c.path == 'auto'}
    assert auto[((8, 8), 'relu', (32, 32))] == 'generic' and auto[((32, 32), 'tanh', (32, 32))] == 'generic'
    assert auto[((8, 8), 'relu', (100, 50, 25))] == 'generic' and 'gemm' in auto.values()
    assert {c.n * c.T for c in cs if c.path == 'gemm'} >= {63, 64, 65, 129}
    assert {c.chunk - c.n * c.T for c in cs if c.chunk and c.path == 'gemm'} >= {1, 0, -1}
    assert any(c.chunk and 0 < c.chunk < c.n * c.T and c.T % c.chunk and c.chunk % c.T for c in cs)      # a rollout straddles a chunk boundary
    assert all(list(U.lengths_of(c.n, c.T)) == [max(1, (c.T, c.T - 1, 1)[r % 3]) for r in range(c.n)] for c in cs)


WRONG_ON = {'cost_at_next': 'humanoid-64x64-100x50x25-relu-n3T2-g0.97-m1-generic-c0',
            'clip_gate': 'swimmer-64x64-32x32-relu-n5T11-g0.97-m0-generic-c0',
            'gamma_t_plus_1': 'swimmer-64x64-32x32-relu-n5T11-g0.97-m0-generic-c0',
            'drop_last': 'swimmer-64x64-32x32-relu-n5T11-g0.97-m0-generic-c0',
            'divide_by_N': 'swimmer-64x64-32x32-relu-n5T11-g0.97-m0-generic-c0'}


@pytest.mark.parametrize('wrong', R.WRONG)
def test_wrong_restatements_miss_the_bound_by_ten(wrong):
    case = U.BY_ID[WRONG_ON[wrong]]
    d = U.case_data(case)
    ref, bad = U.reference(case), U.reference(case, np.float64, wrong)
    whole, worst, _ = U.vector_use(bad['theta'], ref['theta'], d['pdims'])
    print('%s on %s: %.3g x the whole-vector bound, %.3g x the worst block bound' % (wrong, case.id, whole, worst))
    assert whole >= 10.0 and worst >= 10.0
