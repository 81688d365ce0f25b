"""CPU checks of the direct GEMM tests' case table (gemm_cases.py): the table reaches every form the library ships, its dyadic data is
exact in fp32 with headroom, and the comparison test_gpu_gemm.py makes would see each restatement mistake.  No library is loaded."""
import numpy as np
import pytest
import gemm_cases as G

BY_FORM = G.cases_by_form()


def _auto_forms(variant, ta, tb, tiles=((1, 1), (1, 2), (2, 1), (2, 2))):
    out = []
    for tm, tn in tiles:
        out += [G.Form('auto', variant, ta, tb, tm, tn, al, 1) for al in (0, 1)]
        if tm * tn == 1:
            out += [G.Form('auto', variant, ta, tb, 1, 1, al, 4) for al in (0, 1)]
    return out


# every k_gemm_mfma<TM, TN, EPI, TA, TB, AL, PD> the library's callers instantiate, and every argument form of the two composite entries
EXPECTED_FORMS = ([f for epi, ta, tb in G.AUTO_COMBOS for f in _auto_forms(epi, ta, tb)] +
                  _auto_forms('PARTIAL', False, False, tiles=((1, 1),)) +
                  [G.Form('fused_out', v, False, False, t, t, al, 1) for v in ('RELU_OUT', 'RELU_OUT48', 'RELU_OUT64') for t in (1, 2) for al in (0, 1)] +
                  [G.Form('fused_out', v, False, False, 1, 1, al, 4) for v in ('RELU_OUT', 'RELU_OUT48', 'RELU_OUT64') for al in (0, 1)] +
                  [G.Form('skinny', 'act%d%s%s' % (a, d, p), False, False, 0, 0, 0, 0) for a in (0, 1, 2) for d in ('', '-defer') for p in ('', '-part')])


def test_the_table_reaches_every_shipped_form_and_no_other():
    assert len(EXPECTED_FORMS) == 90 + 4 + 18 + 12
    assert sorted(BY_FORM) == sorted(EXPECTED_FORMS)


def test_table_covers_the_listed_corners():
    cs = G.CASES
    auto = [c for c in cs if c.op == 'auto']
    for M in (1, 63, 64, 65, 127, 128, 129):
        assert any(c.M == M for c in auto) and any(c.N == M for c in auto), M
    for Kd in (1, 2, 3, 15, 16, 17, 33, 255, 256, 257):
        assert any(c.Kd == Kd for c in auto), Kd
    assert {c.heads for c in auto} >= {1, 3}
    # layout quirks on every loader form: A strided (!ta) / direct (ta), B direct (!tb) / strided (tb)
    for quirk in ('lda_pad', 'ldw_pad', 'a_off', 'w_off', 'sa_pad', 'sw_pad', 'ldc_pad'):
        for ta, tb in ((False, False), (False, True), (True, False)):
            assert any(getattr(c, quirk) and c.ta == ta and c.tb == tb for c in auto), (quirk, ta, tb)
    # split-K under PD 4 with nk = 1, 2, 3 k-tiles per split, a shorter last split, a last split of one row, <T, F> with M % 4 != 0
    sk = [(c, G.want_form(c)) for c in auto if c.epi == 'PARTIAL' and c.splits > 1]
    for kc in (16, 32, 48):
        assert any(c.kchunk == kc and w['pd'] == 4 for c, w in sk), kc
    assert any(0 < c.Kd - (c.splits - 1) * c.kchunk < c.kchunk for c, w in sk)
    assert any(c.Kd - (c.splits - 1) * c.kchunk == 1 for c, w in sk)
    assert any(c.ta and c.M % 4 for c, w in sk)
    # workgroup counts under the XCD remap
    counts = {w['gx'] * w['gy'] * w['gz'] for w in (G.want_form(c) for c in cs)}
    assert counts >= {1, 2, 3, 7, 9, 15}
    # gemm_auto's own rule on both sides of its threshold, for each tile
    for (M, N, heads), tile in G.RULE_WANT.items():
        hit = [c for c in auto if (c.M, c.N, c.heads, c.tm) == (M, N, heads, 0)]
        assert hit and all((G.want_form(c)['tm'], G.want_form(c)['tn']) == tile for c in hit), (M, N, heads)
    assert {t for t in G.RULE_WANT.values()} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    # the composite entries: split and unsplit, reduced and deferred; all three classes of the fused output layer on both tiles
    sw = [(c, G.want_form(c)) for c in cs if c.op == 'skinny']
    assert any(w['splits'] > 1 and w['reduced'] for c, w in sw) and any(w['splits'] > 1 and not w['reduced'] for c, w in sw)
    assert any(w['splits'] == 0 and c.use_part for c, w in sw)
    assert any(c.op == 'fused_out' and c.tm == 0 for c in cs)


def _small(c):
    return c.heads <= 3


@pytest.mark.parametrize('form', sorted(BY_FORM), ids=G.form_id)
def test_dyadic_cases_are_exact_and_mutations_show(form):
    seen = {}
    for c in BY_FORM[form]:
        p = G.build(c)
        ref = G.expect(c, p)
        for name, (idx, r, bound) in ref.items():
            assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < p.bufs[name].size, (G.case_id(c), name)
        if c.kind != 'float':
            assert G.headroom(c, p) < 2.0 ** 24, G.case_id(c)
            for name, (idx, r, bound) in ref.items():
                if bound is None:
                    assert np.array_equal(r.astype(np.float32).astype(np.float64), r), (G.case_id(c), name)
            if c.epi == 'BIAS_TANH' or (c.op == 'skinny' and c.act == 2 and 'C' in ref):
                assert p.pre_max <= 2.0
        if not _small(c):
            continue
        for mut in G.MUTATIONS:
            if not G.applies(mut, c):
                continue
            seen.setdefault(mut, False)
            bad = G.expect(c, G.build(c), mut)
            for name, (idx, r, bound) in ref.items():
                d = np.abs(bad[name][1] - r)
                if bound is None:
                    seen[mut] |= bool(d.max() >= G.quantum(c))
                elif isinstance(bound, str):                  # tanh: neighbouring pre-activations differ by 1/64 within [-2, 2]
                    seen[mut] |= bool(d.max() > 1e-3)
                else:
                    seen[mut] |= bool((d > 10.0 * bound).any())
    assert seen and all(seen.values()), 'mutations the checks of this form would not see: %s' % [m for m, s in seen.items() if not s]
