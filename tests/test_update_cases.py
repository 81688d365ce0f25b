"""The case table of tests/test_gpu_update_kernels.py, on the CPU and without the library: it is well-formed, the PPO near-bound masking stays
under its cap on the float64 reference alone, and the bounds the GPU test asserts would catch a wrong kernel (tests/update_cases.py)."""
import numpy as np
import tolerances as TOL
import update_cases as U


def test_case_table_is_well_formed():
    ids = [c.id for c in U.CASES]
    assert len(ids) == len(set(ids)) and 250 <= len(ids) <= 400
    for c in U.CASES:
        assert len(c.ph) <= U.METRPO_MAX_LAYERS and all(h >= 1 for h in c.ph) and c.family in U.PATHS and c.mask in U.MASKS
        n = U.nominal_n(c.nspec)
        assert 1 <= n <= 70000
        valid = U.make_mask(c.mask, n)
        assert valid is None or (valid.shape == (n,) and valid.sum() >= 1 and valid.sum() < n), c.id
        if c.mask == 'one':
            assert valid.sum() == 1
        if c.mask == 'edges':                               # first, last and every sample of one 16-sample tile
            assert valid[0] == 0 and valid[-1] == 0 and any(not valid[16 * t:16 * t + 16].any() for t in range(n // 16))
    # what the issue lists is there
    fam = lambda f: [c for c in U.CASES if c.family == f]
    assert {c.env for c in fam('mfma')} == set(U.FUSED_ENVS)
    for env in U.FUSED_ENVS:
        assert {c.nspec for c in fam('mfma') if c.env == env} == {1, 15, 16, 17, 129, ('two_blocks', 0), ('deal', 1), ('deal', 2)}
    assert {c.nspec for c in fam('fused3')} == {1, 15, 17, 129}
    assert {c.ph for c in fam('gemm') if c.env == 'swimmer'} == {(), (3,), (17,), (30, 21, 10), (65, 33), (128, 64), (24, 24, 24, 24)}
    assert {(c.env, c.ph) for c in fam('gemm') if c.env != 'swimmer'} == {('hopper', (17,))}
    for key in {(c.env, c.ph) for c in fam('gemm')}:
        assert {c.nspec for c in fam('gemm') if (c.env, c.ph) == key} == {1, 15, 17, 63, 65, 4099}
    for env, ph, pt in (('swimmer', (32, 32), 128), ('humanoid', (100, 50, 25), 64), ('swimmer', (256, 128), 32)):
        assert {c.nspec for c in fam('generic') if (c.env, c.ph) == (env, ph)} == {1, pt - 1, pt, pt + 1, ('full', pt)}
    for key in {(c.family, c.env, c.ph, c.nspec) for c in U.CASES}:
        n = U.nominal_n(key[3])
        want = {'none'} | ({'seven'} if n >= 2 else set()) | ({'edges'} if n >= 33 else set()) | ({'one'} if n >= 17 else set())
        assert {c.mask for c in U.CASES if (c.family, c.env, c.ph, c.nspec) == key} == want, key


def test_ppo_near_bound_cap():
    """On the float64 reference alone: the samples whose ratio lies within BAND of 1 +- CLIP_LR are at most CAP of a case's valid samples, and
    none at all in a case with N <= 129; the masked case keeps a valid sample.  Over the table the gate is exercised on both sides."""
    outside = []
    for c in U.CASES:
        d = U.case_data(c)
        assert d['removed'] <= U.CAP * d['n_valid'], (c.id, d['removed'], d['n_valid'])
        if d['N'] <= 129:
            assert d['removed'] == 0, (c.id, d['removed'])
        assert d['n_valid'] - d['removed'] >= 1
        r = d['ratio'][d['keep']]
        outside.append(float(((r < 1 - U.CLIP_LR) | (r > 1 + U.CLIP_LR)).mean()))
    assert 0.02 <= np.median(outside) <= 0.5, np.median(outside)


def _representatives():
    """One case per (family, env, policy shape) at N = 17 and N = 129 (the GEMM table's largest N below 129 is 65; the generic table's 127 - 129)."""
    out, done = [], set()
    for c in U.CASES:
        n = U.nominal_n(c.nspec)
        slot = 17 if n in (16, 17) else (129 if n in (63, 65, 127, 128, 129) else None)
        if c.mask in ('none', 'seven') and slot and (c.family, c.env, c.ph, slot, c.mask) not in done:
            done.add((c.family, c.env, c.ph, slot, c.mask))
            out.append(c)
    return out


def test_the_bounds_discriminate():
    """A result that is the float64 reference of the same case with ONE sample's valid bit flipped, or with the largest log_std gradient entry
    scaled by 1.01, misses the whole-vector or the per-block bound by at least 100 x.  Smallest margins seen (printed): flipped bit 7.9e2 x
    (gradient), 1.3e3 x (FVP); scaled log_std entry 3.6e2 x."""
    worst = {'flip grad': np.inf, 'flip fvp': np.inf, 'scale log_std': np.inf}
    for c in _representatives():
        d = U.case_data(c)
        ref = U.references(d)
        flipped = d['keep'].astype(np.uint8)
        k = int(np.flatnonzero(flipped)[len(np.flatnonzero(flipped)) // 2])
        flipped[k] = 0
        bad = U.references(d, valid=flipped)
        pd, na = d['pdims'], d['pdims'][-1]
        for op in ('loss_grad', 'vpg', 'ppo1'):
            worst['flip grad'] = min(worst['flip grad'], U.vector_use(bad[op][1], ref[op][1], TOL.GRAD_REL_L2, pd)[0])
            g = ref[op][1].copy()
            i = len(g) - na + int(np.argmax(np.abs(g[-na:])))
            g[i] *= 1.01
            worst['scale log_std'] = min(worst['scale log_std'], U.vector_use(g, ref[op][1], TOL.GRAD_REL_L2, pd)[0])
        worst['flip fvp'] = min(worst['flip fvp'], U.vector_use(bad['fvp'], ref['fvp'], TOL.FVP_REL_L2, pd)[0])
    print('smallest margins (x the bound):', {k: '%.3g' % v for k, v in worst.items()})
    assert all(v >= 100.0 for v in worst.values()), worst
