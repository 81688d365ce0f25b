"""The shared MFMA GEMM (csrc/gemm_mfma.h) on its own, through the diagnostics hook Engine.debug_gemm: every k_gemm_mfma instantiation the
library's callers make -- the ten (EPI, TA, TB) combinations of gemm_auto / gemm_mfma_launch on all four tiles, aligned and unaligned
loaders, prefetch distance 1 and 4 -- plus gemm_skinny_bias and gemm_relu_fused_out in all their argument forms, at tile-edge extents,
layout quirks, split-K corner forms and workgroup counts that are no multiple of 8 (gemm_cases.py holds the table and the float64 side;
test_gemm_cases.py checks both on the CPU).

Per case: the form the library reports equals the form the table expects; on dyadic operands (every product and partial sum exact in
fp32) the output equals the float64 result exactly -- only tanh (the project's allowance for one tanh layer, TOL.STEP['atol'], after the
BIAS_ID form gave the exact pre-activation on the same operands) and Adam (adam_bounds, the gradient itself being exact) have a bound;
on fp32 normals |got - ref| <= (n + 2) u (|A| @ |W| + |bias|) per cell; no cell outside the stated output is written, every cell inside
is; a second call returns the same bits.  The worst share of the float bound is printed per form (pytest -s)."""
import numpy as np
import pytest
import torch
import helpers as Hh
import tolerances as TOL
import gemm_cases as G

pytestmark = pytest.mark.gpu

BY_FORM = G.cases_by_form()
OUTPUTS = ('C', 'part', 'am', 'av', 'bvec', 'bam', 'bav')


@pytest.fixture(scope='module')
def eng():
    return Hh.make_engine('swimmer', 3, (64, 64), (32, 32), seed=3)[0]


def run(eng, c, p):
    """one call on fresh device copies of p.bufs -> (reported form, {output buffer: float32 array})"""
    dev = dict((n, torch.from_numpy(b).to(eng.device)) for n, b in p.bufs.items())
    assert all(t.data_ptr() % 16 == 0 for t in dev.values())
    fields = G.device_fields(c, p)
    for n in G.pointer_names(c, p):
        fields[n] = (dev[n], {'A': c.a_off, 'W': c.w_off}.get(n, 0))
    form = eng.debug_gemm(c.op, c.epi if c.op == 'auto' else 0, **fields)
    torch.cuda.synchronize()
    return form, dict((n, dev[n].cpu().numpy()) for n in OUTPUTS if n in dev)


def bits(a):
    return a.view(np.int32)


def check(eng, c):
    """-> worst share of a float bound used (0 for exact cases)"""
    what = G.case_id(c)
    p = G.build(c)
    ref = G.expect(c, p)
    form, got = run(eng, c, p)
    assert form == p.want, what
    share = 0.0
    for name, g in got.items():
        untouched = np.ones(g.size, bool)
        if name in ref:
            idx, r, bound = ref[name]
            untouched[idx] = False
            x = g[idx].astype(np.float64)
            miss = idx[~np.isfinite(x) | (g[idx] == G.SENTINEL)]
            assert miss.size == 0, '%s %s: %d of %d cells not written, flat indices %s ..' % (what, name, miss.size, idx.size, miss[:8])
            if bound is None:
                assert np.array_equal(x, r), '%s %s: %d of %d cells differ from the exact result, worst %g' % (
                    what, name, (x != r).sum(), x.size, np.abs(x - r).max())
            elif isinstance(bound, str):
                print('    %s %s: worst tanh error %.2e of %.0e' % (what, name, np.abs(x - r).max(), TOL.STEP['atol']))
                np.testing.assert_allclose(x, r, rtol=0, atol=TOL.STEP['atol'], err_msg='%s %s (tanh)' % (what, name))
            else:
                s = float((np.abs(x - r) / bound).max())
                print('    %s %s: worst share of the bound %.3f' % (what, name, s))
                assert s <= 1.0, '%s %s: %d cells beyond the bound, worst share %g' % (what, name, (np.abs(x - r) > bound).sum(), s)
                if c.kind == 'float':
                    share = max(share, s)
        assert np.array_equal(bits(g[untouched]), bits(p.bufs[name][untouched])), '%s %s: written outside the output' % (what, name)
    form2, again = run(eng, c, p)
    assert form2 == form and all(np.array_equal(bits(again[n]), bits(got[n])) for n in got), what + ': a second call differs'
    return share


@pytest.mark.parametrize('form', sorted(BY_FORM), ids=G.form_id)
def test_form_against_float64(eng, form):
    worst = 0.0
    for c in BY_FORM[form]:
        tanh = c.epi == 'BIAS_TANH' if c.op == 'auto' else (c.op == 'skinny' and c.act == 2)
        if tanh:        # the exact pre-activation first, on the same operands and the same tile
            check(eng, c._replace(epi='BIAS_ID') if c.op == 'auto' else c._replace(act=0))
        worst = max(worst, check(eng, c))
    print('%s: %d cases, worst share of the float bound %.3f' % (G.form_id(form), len(BY_FORM[form]), worst))


def test_rejects_what_the_library_does_not_ship(eng):
    from metrpo_amd._lib import MetrpoError
    a = torch.zeros(64, device=eng.device)
    base = dict(M=4, N=4, Kd=4, heads=1, lda=4, ldw=4, ldc=4, A=a, W=a, C=a, bias=a, mask=a, ldm=4)
    for kw in (dict(epi='BIAS_ID', ta=1), dict(epi='PLAIN'), dict(epi='ADAM', tb=1), dict(epi='RELU_MASK', ta=1, tb=1), dict(epi='BIAS_ID', tm=1),
               dict(epi='BIAS_ID', tm=3, tn=1), dict(epi='BIAS_ID', M=0)):
        f = dict(base); f.update(kw)
        with pytest.raises(MetrpoError):
            eng.debug_gemm('auto', **f)
    with pytest.raises(MetrpoError):
        eng.debug_gemm('auto', 'PARTIAL', ta=1, part=a, stridePart=20, splits=2, kchunk=4, **base)      # an empty second split
    with pytest.raises(MetrpoError):
        eng.debug_gemm('fused_out', tm=1, tn=1, w2=a, part=a, no=8, **base)                               # N no multiple of 64
    with pytest.raises(MetrpoError):
        eng.debug_gemm('skinny', tm=1, tn=1, **base)


def test_hook_leaves_the_context_alone():
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 3, (64, 64), (32, 32), seed=3)
    gen = torch.Generator(device=eng.device).manual_seed(7)
    rnd = lambda *s: torch.rand(*s, generator=gen, device=eng.device)
    eng.set_train_adam(rnd(eng.K, eng.dyn_param_count) - 0.5, rnd(eng.K, eng.dyn_param_count), 5)
    eng.set_policy_adam(rnd(eng.P) - 0.5, rnd(eng.P), 9)
    rng = np.random.RandomState(1)
    B, T, H = 32, 2, 2
    eng.rollout(B, T, H, 'step_rand', pool, eps=rng.randn(T, B, dm.na), model_idx=rng.randint(eng.K, size=(T, B)),
                reset_idx=rng.randint(len(pool), size=(T + 1, B)), reset_model=rng.randint(eng.K, size=(T + 1, B)))
    assert eng.last_rollout_kernel() is not None

    def state():
        m, v, t = eng.get_train_adam()
        pm, pv, pt = eng.get_policy_adam()
        return [eng.get_policy(), eng.get_dynamics(), m, v, pm, pv], (t, pt, eng.last_rollout_kernel(), eng.rollout_note())
    before, scalars = state()
    for c in (G.case('auto', 'ADAM', 65, 65, 17, ta=True, heads=3, seed=1), G.case('skinny', 'BIAS_ID', 65, 18, 257, heads=3, use_part=True, seed=2),
              G.case('fused_out', 'BIAS_RELU', 65, 128, 17, tm=1, tn=1, no=18, amp=4, seed=3)):
        run(eng, c, G.build(c))
    after, scalars2 = state()
    assert scalars2 == scalars
    assert all(torch.equal(x, y) for x, y in zip(before, after))
