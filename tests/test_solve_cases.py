"""The case table of tests/test_gpu_trpo_solve.py, on the CPU and without the library (tests/solve_cases.py): it is well-formed; (a) every bound is
a small share of what it bounds; (b) every line-search decision of the float64 solve is clear of its thresholds; (c) the bounds discriminate."""
import json

import numpy as np
import pytest
import tolerances as TOL
import solve_cases as S
import update_cases as U

_CACHE = {}


def solved(c):
    """(data, reference solve, bounds) of a case, computed once for the module."""
    if c.id not in _CACHE:
        d = U.case_data(c.ucase)
        _CACHE[c.id] = (d,) + S.solve_and_bounds(d, c.k, draws=c.draws)
    return _CACHE[c.id]


def test_case_table_is_well_formed():
    ids = [c.id for c in S.CASES]
    assert len(ids) == len(set(ids)) and 300 <= len(ids) <= 400
    assert TOL.SOLVE_DRAWS == 4 and TOL.SOLVE_MARGIN == 2.0 and all(c.draws == 4 for c in S.CASES)         # (no case needed fewer draws: the whole float64 side takes ~30 s)
    base = [c for c in S.CASES if not c.lead]
    # every case of update_cases runs a solve of k = 2, the GEMM path on the widths the issue keeps
    want = [u.id for u in U.CASES if u.family != 'gemm' or (u.env == 'swimmer' and u.ph in S.GEMM_WIDTHS)]
    assert [c.ucase.id for c in base] == want and all(c.k == S.K_ALL for c in base) and not S.RUNS_SHORT
    assert {c.ucase.env for c in base if c.ucase.family == 'mfma'} == set(U.FUSED_ENVS)
    assert {c.ucase.ph for c in base if c.ucase.family == 'gemm'} == set(S.GEMM_WIDTHS)
    assert {(c.ucase.env, c.ucase.ph) for c in base if c.ucase.family == 'generic'} == {('swimmer', (32, 32)), ('humanoid', (100, 50, 25)), ('swimmer', (256, 128))}
    for c in base:                                         # the seed of a case is update_cases' unless (b) moved it
        assert c.ucase.seed == S.SEEDS.get(c.id, next(u for u in U.CASES if u.id == c.ucase.id).seed)
    # one lead per (family, env, policy shape), at k = 0, 1, 3, 10
    shapes = {(c.ucase.family, c.ucase.env, c.ucase.ph) for c in base}
    for key in shapes:
        lead = [c for c in S.CASES if c.lead and (c.ucase.family, c.ucase.env, c.ucase.ph) == key]
        assert sorted(c.k for c in lead) == [0, 1, 3, 10], key
        assert {c.ucase.nspec for c in lead} == {S.lead_n(lead[0].ucase)} and {c.ucase.mask for c in lead} == {'none'}
    # a P in each of the four ranges of the CG step (cg_device.h: 2 x 1024, 4 x 1024, 13 x 1024, the loop form), and one below a block
    P = {O_P(c) for c in base}
    assert any(p < 1024 for p in P) and any(1024 < p <= 2048 for p in P) and any(2048 < p <= 4096 for p in P)
    assert any(4096 < p <= 13312 for p in P) and any(p > 13312 for p in P), sorted(P)


def O_P(c):
    from oracle import metrpo_oracle as O
    ns, na, _ = O.ENV_SPECS[c.ucase.env]
    return O.policy_num_params(O.policy_dims(ns, c.ucase.ph, na))


def test_bounds_are_a_small_share_of_what_they_bound():
    """(a): every per-block bound (d and step), the whole-vector ones and the bound on beta are at most 0.1 of the reference's norm of what they bound,
    at every case and k.  At k <= 3 the rule itself stays far below (largest share printed); at k = 10 it gives more for seven lead cases (ten CG
    iterations on N <= 129 samples amplify what the FVP row admits: up to 3.0 of a block), and solve_cases cuts those bounds to 0.1."""
    worst, capped = (0.0, None), {}
    for c in S.CASES:
        d, ref, b = solved(c)
        share = b['beta'] / abs(ref['beta'])
        for key in ('d', 'step'):
            for nm, bound in b[key].items():
                n = ref['norms'][key][nm]
                assert n > 0.0 or c.k == 0, (c.id, key, nm)
                share = max(share, bound / n if n > 0.0 else 0.0)
        assert share <= S.CAP * (1.0 + 1e-12), (c.id, share)
        if ref['capped']:
            capped[c.id] = ref['capped']
        else:
            worst = max(worst, (share, c.id))
    print('largest bound / norm where the rule alone decides: %.3g (%s); cut to %g: %s' % (worst + (S.CAP, json.dumps(capped))))
    assert all(i.endswith('-k10') for i in capped) and len(capped) == 7, capped


def test_line_search_decisions_are_clear():
    """(b): every trial of the float64 search is clear of loss_before and max_kl by the LOSS_RTOL / KL_ATOL / KL_RTOL rows, and the search accepts a
    trial.  k = 0 is left out: its step is exactly zero, every trial theta is theta bit for bit and the loss equals loss_before, so the decision
    is rounding and changes nothing (the GPU test holds the policy to its bits there)."""
    depth = []
    for c in S.CASES:
        if c.k == 0:
            continue
        d, ref, b = solved(c)
        ls = S.line_search(d, ref['beta'], ref['d'])
        assert all(clear for _, _, _, _, clear in ls), (c.id, ls)
        assert ls[-1][3], (c.id, 'no trial accepted')
        depth.append(len(ls) - 1)
    assert min(depth) == 0 and max(depth) >= 1              # both a first-trial accept and a backtrack occur


@pytest.mark.parametrize('name', S.CORRUPTIONS)
def test_the_bounds_discriminate(name):
    """(c): at every N <= 129, the float64 solve with one seeded defect exceeds a bound (d, beta or step; whole or per block; either form of the
    step scale).  Smallest margins seen (x the bound): block scaled 21, tile left out 7.8e2, invalid included 4.9e3, stale vector 2.8e7,
    reg left out 2.1, reg left out of d.(H d) 2.0.  `invalid_included` has no meaning without a mask: those cases are counted, not run."""
    worst, n_run, n_identity = (np.inf, None), 0, 0
    for c in S.CASES:
        if c.lead or U.nominal_n(c.ucase.nspec) > 129:
            continue
        d, ref, b = solved(c)
        bad = S.corrupted(d, c.k, name, ref['g'], ref)
        if bad is None:
            assert name == 'invalid_included' and c.ucase.mask == 'none'
            n_identity += 1
            continue
        share = S.corruption_share(bad, ref, b, d['pdims'])
        assert share > 1.0, (c.id, name, share)
        worst = min(worst, (share, c.id)); n_run += 1
    print('%s: smallest margin %.3g x (%s), %d cases, %d without a mask' % (name, worst[0], worst[1], n_run, n_identity))
    assert n_run >= 140


def test_shares_of_the_reference_and_of_a_perturbed_solve():
    """The measuring functions themselves: the reference uses 0 of its bounds, a solve perturbed as the bounds' own draws uses at most 1 / SOLVE_MARGIN."""
    c = next(c for c in S.CASES if c.id == 'mfma-ant-32x32-N17-seven-k2')
    d, ref, b = solved(c)
    assert S.worst_share(S.shares(ref['d'], ref['beta'], ref, b, d['pdims'])) == 0.0
    F = S.fisher(S.problem(d))
    rng = np.random.RandomState((c.ucase.seed * 131 + 17 * c.k + 0) % (2 ** 31))
    got = S.run_solve(ref['g'], c.k, lambda i, v: (lambda z: z + S.admitted_error(z, d['pdims'], rng))(F(v)))
    use = S.worst_share(S.shares(got['d'], got['beta'], ref, b, d['pdims']))
    assert 0.0 < use <= 1.0 / TOL.SOLVE_MARGIN + 1e-9, use
