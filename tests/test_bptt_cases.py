"""The case table of tests/test_gpu_bptt_edges.py, on the CPU and without the library (tests/bptt_cases.py): it is well formed and holds every
(sweep family, VJP family, instantiation) at every size; the restatement the kink guard and the mutations run on reproduces both references; the
kink guard's conditions hold; and the bounds the GPU test asserts would catch a wrong kernel."""
import numpy as np
import bptt_cases as U


def _sizes(cases):
    return {(c.B, c.T) for c in cases}


def test_case_table_is_well_formed():
    ids = [c.id for c in U.CASES]
    assert len(ids) == len(set(ids)) and 300 <= len(ids) <= 500
    main = {(B, 3) for B in U.SIZES_B} | {(B, T) for B in U.SHORT_B for T in (1, 2)}
    plain = [c for c in U.CASES if c.variant == 'plain' and not c.stoch and not c.force and c.K == 2 and c.gamma == 0.97]
    for sweep, env, dh, ph, vjp in U.SHAPES:                   # every shape the sweep families are asked on, at every size
        assert _sizes(c for c in plain if (c.sweep, c.env, c.dh, c.ph, c.vjp) == (sweep, env, dh, ph, vjp)) == main, (sweep, env, dh)
    shapes = {(s[0], s[1], s[2]) for s in U.SHAPES}
    assert {('mfma', e, (64, 64)) for e in U.FUSED_ENVS} <= shapes and sum(s[0] == 'mfma_pad' for s in shapes) == 2
    assert {s[2] for s in shapes if s[0] == 'gemm'} == {(128, 128), (128, 160, 128), (24, 16)}
    assert {U.generic_bs(s[1], s[2], s[3]) for s in U.SHAPES if s[0] == 'generic'} == {64, 32}
    assert U.bptt_floats('humanoid', (48, 48, 32), (100, 50, 25)) == 786 and 786 * 64 * 4 > U.LDS_MAX >= 786 * 32 * 4
    # k_dg_pre_mfma<ENV, STOCH> beyond swimmer: the four other envs on the GEMM path behind a 2 x 32 policy, appended behind everything else
    extra = [c for c in U.CASES if c.sweep == 'gemm' and (c.dh, c.ph) == ((128, 128), (32, 32)) and c.env != 'swimmer']
    assert U.CASES[-len(extra):] == extra and all(c.seed == 4000 + U.CASES.index(c) or c.id in U.SEEDS for c in U.CASES)
    for env in U.FUSED_ENVS[1:]:
        assert sorted((c.B, c.T, c.stoch) for c in extra if c.env == env) == [(1, 2, False), (17, 2, False), (17, 2, True), (65, 2, False)], env
    for fam in U.DET_PATH:
        mine = [c for c in U.CASES if c.sweep == fam and c not in extra]
        assert any(c.K == 1 and (c.B, c.T) == (1, 1) for c in mine) and any(c.K == 1 and c.B == 65 for c in mine)
        assert any(c.gamma == 1.0 and c.variant == 'plain' for c in mine)
        assert _sizes(c for c in mine if c.stoch) == {(B, T) for B in U.STOCH_B for T in (1, 3)}
        assert {c.B for c in mine if c.variant == 'clipped'} == {17, 65}
        assert {(c.B, c.T) for c in mine if c.variant == 'ant_tile'} >= {(17, 3), (65, 3), (129, 3), (17, 2)}
        for B in U.SHORT_B:
            assert {(c.T, c.gamma) for c in mine if c.variant == 'ant_all' and c.B == B} == {(1, 0.97), (2, 0.97), (2, 1.0), (3, 0.97), (3, 1.0)}
        forced = {c.vjp for c in mine if c.force}
        assert forced == {'generic', 'gemm'}, (fam, forced)
        for v in forced:
            assert _sizes(c for c in mine if c.force and c.vjp == v) >= {(1, 1), (17, 3), (65, 3), (129, 3)}
    pairs = {(c.sweep, c.vjp) for c in U.CASES}
    assert pairs == {('mfma', 'mfma'), ('mfma', 'generic'), ('mfma', 'gemm'), ('mfma_pad', 'mfma'), ('mfma_pad', 'generic'), ('mfma_pad', 'gemm'), ('gemm', 'mfma'), ('gemm', 'generic'),
                     ('gemm', 'gemm'), ('generic', 'mfma'), ('generic', 'generic'), ('generic', 'gemm')}
    assert any(c.ph == (100, 50, 25) and c.vjp == 'gemm' and not c.force for c in U.CASES)      # (f3_active excludes the VJP)
    for c in U.CASES:
        assert c.variant in ('plain', 'clipped', 'ant_tile', 'ant_all') and (c.env == 'ant' or not c.variant.startswith('ant'))
        assert not c.force or (c.ph == (32, 32) and c.env in U.FUSED_ENVS)


def test_restatement_reproduces_both_references():
    """walk() in float64 is oracle.bptt_oracle.policy_costs_and_grad without noise and tests/bptt_stochastic_ref.py with it."""
    worst = 0.0
    for c in U.CASES[::5] + [c for c in U.CASES if c.stoch][::3]:
        d = U.case_data(c)
        rc, rg, rn = U.reference(d)
        w = U.restated(d)
        worst = max(worst, float(np.max(np.abs(w['costs'] - rc) / np.maximum(1.0, np.abs(rc)))),
                    float(np.linalg.norm(w['grad'] - rg) / max(np.linalg.norm(rg), 1e-300)) if np.any(rg) else float(np.abs(w['grad']).max()))
        if c.stoch:
            assert np.array_equal(w['nsat'], rn), c.id
    print('restatement vs references: worst relative difference %.3g' % worst)
    assert worst < 1e-11


def test_kink_guard_conditions_hold():
    """Conditions, not measurements: at most a quarter of a case's envs replaced, no case short of its B; every accepted env takes the same branch
    in float32 and float64 at every relu, clip, cost and done site with the float64 argument >= 16 x the float32 - float64 difference away.
    The deliberate variants sit on their side of the kink by the same margin.  Figures seen (printed): largest replaced share 0.031, smallest
    margin 16.4 x."""
    share, margin, sat = 0.0, np.inf, 0
    for c in U.CASES:
        d = U.case_data(c)
        assert d['accepted'] == c.B and d['replaced'] <= U.MAX_REPLACED * c.B, (c.id, d['replaced'], d['accepted'])
        assert d['margin'] >= U.KINK_FACTOR, (c.id, d['margin'])
        share, margin = max(share, d['replaced'] / float(c.B)), min(margin, d['margin'])
        if c.variant != 'plain' or c.stoch:
            s = U.walk(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma, d['eps'], grad=False)
            if c.variant == 'clipped':
                assert np.all(s['sites']['clip'] > 1.0)
            if c.variant.startswith('ant'):                     # column 0 of ant_lo: the step-0 transition of model 0; every model's has the same sign
                n = 16 if c.variant == 'ant_tile' else c.B
                lo = s['sites']['ant_lo'].reshape(c.B, c.K, c.T)
                assert np.all(lo[:n, :, 0] < 0) and np.all(lo[n:] > 0) and np.all(s['sites']['ant_hi'][n:] > 0), c.id
            if c.stoch and c.B >= 17:
                assert s['nsat'].sum() > 0, c.id
                sat += 1
    print('kink guard: largest replaced share %.3g, smallest margin %.3g x' % (share, margin))
    assert sat >= 24


def test_done_from_step_0_at_T_1_is_the_case_without_dones():
    """is_done marks an env at the step-0 transition and `dones` is updated after the cost: at T = 1 no mask has taken effect."""
    for c in U.CASES:
        if c.variant == 'ant_all' and c.T == 1:
            d = U.case_data(c)
            a, b = U.restated(d), U.restated(d, mut=('done', None))
            assert np.array_equal(a['costs'], b['costs']) and np.array_equal(a['grad'], b['grad']) and np.any(a['grad'])
        if c.variant == 'ant_all' and c.T > 1 and c.gamma == 1.0:       # only the t = 0 term, weight gamma^0, survives
            other = next(o for o in U.CASES if o.variant == 'ant_all' and (o.sweep, o.B, o.T) == (c.sweep, c.B, c.T) and o.gamma == 0.97)
            d, e = U.case_data(c), U.case_data(other)
            g1 = U.walk(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, 1.0)
            g2 = U.walk(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, 0.97)
            assert np.array_equal(g1['costs'], g2['costs']) and np.array_equal(g1['grad'], g2['grad'])


def test_the_bounds_discriminate():
    """Each wrong result, made on the reference alone, misses the bounds of tests/test_gpu_bptt_edges.py (TOL.BPTT_COST on the costs,
    TOL.BPTT_GRAD_REL_L2 on the whole gradient, tolerances.block_bound on every variable) by at least 10 x, at every size it applies to.
    The all-clipped cases have an exactly zero reference and an exact check: any non-zero slot misses it.  Smallest miss factors seen (printed)."""
    worst, low = {}, []

    def miss(name, c, bad, ref):
        whole, blk, _, _ = U.vector_use(bad['grad'], ref['grad'], U.case_data(c)['pdims'])
        m = max(whole, blk, U.cost_use(bad['costs'], ref['costs']))
        if m < worst.get(name, (np.inf, None))[0]:
            worst[name] = (m, c.id)
        if m < 10.0:
            low.append((name, c.id, m))

    for c in U.CASES:
        if c.variant == 'clipped':
            continue
        d = U.case_data(c)
        ref = U.restated(d)
        pd, na = d['pdims'], d['pdims'][-1]
        g = ref['grad'].copy()
        b_last = dict(U.blocks(pd))['b%d' % (len(pd) - 2)]
        g[b_last] *= 1.01
        miss('b_last x 1.01', c, dict(costs=ref['costs'], grad=g), ref)
        if c.B >= 15:
            miss('last env dropped', c, U.restated(d, mut=('drop', c.B - 1)), ref)
        if c.gamma == 0.97 and c.T >= 2 and c.variant != 'ant_all':
            miss('gamma^(t+1)', c, U.restated(d, mut=('gamma',)), ref)
        miss('terminal row', c, U.restated(d, mut=('terminal',)), ref)
        if c.variant == 'ant_tile' or (c.variant == 'ant_all' and c.T >= 2):
            miss('one done flag ignored', c, U.restated(d, mut=('done', min(7, c.B - 1))), ref)
        if c.stoch:
            g = ref['grad'].copy()
            g[len(g) - na + int(np.argmax(np.abs(g[-na:])))] *= 1.01
            miss('log_std slot x 1.01', c, dict(costs=ref['costs'], grad=g), ref)
    print('smallest miss factors (x the bound):', {k: '%.3g (%s)' % v for k, v in sorted(worst.items())})
    assert len(worst) == 6 and not low, low


def test_float32_restatement_meets_the_rows():
    """The float32 NumPy restatement against the float64 one, on a sample of the table: float32 arithmetic alone stays inside every bound the GPU
    test asserts, so no block needs a measured exception.  Largest shares seen (printed)."""
    use = {'cost': 0.0, 'whole': 0.0, 'block': 0.0}
    for c in U.CASES[::4]:
        if c.variant == 'clipped':
            continue
        d = U.case_data(c)
        a, b = U.restated(d, np.float32), U.restated(d)
        whole, blk, _, _ = U.vector_use(a['grad'], b['grad'], d['pdims'])
        use = {'cost': max(use['cost'], U.cost_use(a['costs'], b['costs'])), 'whole': max(use['whole'], whole), 'block': max(use['block'], blk)}
    print('float32 restatement, share of each bound:', {k: '%.3g' % v for k, v in use.items()})
    assert all(v <= 1.0 for v in use.values()), use
