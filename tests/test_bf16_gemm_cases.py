"""CPU checks of the direct bf16-GEMM tests' case table (bf16_gemm_cases.py): the dyadic data is exact in f32 with headroom and really exercises the
output rounding (a good share of cells is changed by it, exact ties of both parities occur in every bf16-output case that can hold them), every one of
the six k_gemm_bf16 instantiations and every activation has row, column and k edges of its own, the pick rule is restated on both sides of its
threshold, and the comparison test_gpu_bf16_gemm.py makes would reject each restatement mistake on every case it applies to.  No library is loaded."""
import numpy as np
import pytest
import bf16_gemm_cases as G
from dyn_bf16_ref import bf16_round

BY_GROUP = G.cases_by_group()
INSTANCES = ['%s-%s-bn%d' % (at, ct, bn) for at, ct in G.PAIRS for bn in (64, 128)]


def test_dyadic_operands_are_bf16_values():
    v = np.arange(-16, 17) / 8.0
    assert len(v) == 33 and np.array_equal(bf16_round(v.astype(np.float32)).astype(np.float64), v)


def test_table_size_and_groups():
    assert 150 <= len(G.CASES) <= 250, len(G.CASES)
    assert set(BY_GROUP) == set(INSTANCES) | {'f32-bf16-rule64', 'bf16-f32-rule64', 'image'}
    assert len(set(G.CASES)) == len(G.CASES)


def test_table_covers_the_listed_values():
    gm = G.GEMM_CASES
    assert {c.M for c in gm} >= set(G.MS) and {c.N for c in gm} >= set(G.NS)
    assert {c.lda for c in gm if c.at == 'f32'} == set(G.LDAS) and {c.Kp for c in gm if c.at == 'f32'} == {64, 128, 192}
    assert {c.Kp for c in gm if c.at == 'bf16'} == {64, 128, 192, 256} and any(c.K < c.Kp for c in gm if c.at == 'bf16')
    assert sum(c.at == 'bf16' and c.lda > c.Kp for c in gm) >= 4
    assert {c.heads for c in gm} == {1, 3}
    assert {c.sa0 for c in gm if c.at == 'f32' and c.heads == 3} == {True, False}           # one X for all heads, and an X per head
    assert {c.K for c in G.IMAGE_CASES} == set(G.IMG_KD) and {c.N for c in G.IMAGE_CASES} == set(G.IMG_N) and {c.heads for c in G.IMAGE_CASES} == {1, 3}
    # the 128-column tile's own corners: the col >= ldc skip (N = 136 -> ldc 192 under a 256-column grid), pad columns, the TM = 2 row map off the tile edge
    for at, ct in G.PAIRS:
        c128 = [c for c in gm if (c.at, c.ct, c.bn) == (at, ct, 128)]
        assert any(c.N == 136 for c in c128) and any(c.N % 128 not in (0, ) and c.N > 128 for c in c128)
        assert any(c.M % 128 not in (0, 1) for c in c128) and any(c.M > 128 for c in c128)


def _edges(cs):
    return (any(c.M % 128 != 0 for c in cs), any(c.N % G.want_form(c, 256)['bn'] != 0 for c in cs), any(c.K % 64 != 0 for c in cs))


def test_every_instantiation_and_activation_has_its_edges():
    gm = G.GEMM_CASES
    for at, ct in G.PAIRS:
        for bn in (64, 128):
            cs = [c for c in gm if (c.at, c.ct, c.bn) == (at, ct, bn)]
            assert all(_edges(cs)), (at, ct, bn)
            assert {c.act for c in cs} == {0, 1, 2} and {c.kind for c in cs} == {'dyadic', 'dyadic_small', 'float'}
            assert any(c.M > 128 for c in cs) and any(c.N > bn for c in cs)                    # more than one block either way
    for act in (0, 1, 2):
        for ct in ('bf16', 'f32'):
            for bn in (64, 128):
                assert all(_edges([c for c in gm if (c.act, c.ct, c.bn) == (act, ct, bn)])), (act, ct, bn)


def test_pick_rule_restated():
    mk = lambda M, N, heads: G.gemm_case('f32', 'bf16', 0, M, N, K=4, heads=heads)
    for n_cu in (64, 256, 304):
        lo, hi = G.threshold_cases(n_cu)
        assert G.want_form(lo, n_cu) == dict(bn=64, gx=2, gy=n_cu - 1, gz=1, n_cu=n_cu)
        assert G.want_form(hi, n_cu) == dict(bn=128, gx=1, gy=n_cu, gz=1, n_cu=n_cu)
        assert G.want_form(mk(128 * n_cu, 64, 3), n_cu)['bn'] == 64                           # N <= 64: never the wide tile
    assert G.want_form(mk(4097, 512, 3), 256) == dict(bn=128, gx=4, gy=33, gz=3, n_cu=256)      # the one shape the random-net test reaches it with
    assert G.want_form(mk(129, 144, 5), 256)['bn'] == 64
    for c in BY_GROUP['f32-bf16-rule64'] + BY_GROUP['bf16-f32-rule64']:
        assert c.bn == 0 and c.N in (64, 65)
    assert {c.N for c in BY_GROUP['f32-bf16-rule64']} == {64, 65}


def test_rounding_really_rounds_and_ties_of_both_parities_occur():
    even = odd = 0
    for c in G.GEMM_CASES:
        if not (c.kind == 'dyadic' and c.ct == 'bf16'):
            continue
        p = G.build(c)
        y = G.expect(c, p, 'out_unrounded')
        e = G.expect(c, p)
        real = ~e.pad
        changed = (y.val != e.val)[real]
        assert changed.mean() >= 0.05, (G.case_id(c), changed.mean())
        u = y.val[real].astype(np.float32).view(np.uint32)
        tie = (u & 0xffff) == 0x8000
        kept_odd = ((u >> 16) & 1) == 1
        assert (tie & ~kept_odd).any(), G.case_id(c)
        assert c.N == 1 or (tie & kept_odd).any(), G.case_id(c)
        even += int((tie & ~kept_odd).sum()); odd += int((tie & kept_odd).sum())
    assert even > 1000 and odd > 1000, (even, odd)                  # not the planted ones alone: dense sums in [4, 8) land on ties by themselves


def _mutations(c):
    return [m for m in (G.IMAGE_MUTATIONS if c.op == 'image' else G.GEMM_MUTATIONS) if G.applies(m, c)]


@pytest.mark.parametrize('group', sorted(BY_GROUP))
def test_cases_are_exact_and_every_mutation_shows(group):
    seen = set()
    for c in BY_GROUP[group]:
        what = G.case_id(c)
        p = G.build(c)
        good = G.expect(c, p)
        assert len(np.unique(good.idx)) == len(good.idx) and good.idx.min() >= 0 and good.idx.max() < p.bufs['C'].size, what
        assert not G.differs(c, good, good), what
        if c.op == 'gemm':
            if c.kind != 'float':
                assert G.headroom(c, p) < 2.0 ** 24, what
                assert np.abs(p.A).max() <= 2 and np.abs(p.W).max() <= 2 and np.array_equal(p.A * 8, np.round(p.A * 8)) and np.array_equal(p.W * 8, np.round(p.W * 8))
                assert np.array_equal(p.bias * 64, np.round(p.bias * 64)), what
            if c.kind == 'dyadic':
                assert good.exact and np.array_equal(good.val.astype(np.float32).astype(np.float64), good.val), what
            else:
                assert not good.exact and np.all(good.lo <= good.hi) and np.all(np.isfinite(good.lo)) and np.all(np.isfinite(good.hi)), what
            if c.kind == 'float' and c.ct == 'f32':
                assert np.all(good.bound > 0) and good.bound.max() <= (c.K + 2) * G.U * (c.K * 16.0 + 4.0), what      # |a|, |w|, |b| <= 4
            if c.kind == 'dyadic_small':
                assert np.abs(np.arctanh(np.clip(good.centre, -0.9999999, 0.9999999))).max() <= 3.5, what
            assert np.all(good.val[good.pad] == 0) and np.all(good.lo[good.pad] == 0) and np.all(good.hi[good.pad] == 0), what
        for mut in _mutations(c):
            assert G.differs(c, good, G.expect(c, p, mut)), '%s: the check would not see %s' % (what, mut)
            seen.add(mut)
    if group == 'image':
        assert seen == set(G.IMAGE_MUTATIONS)
    elif 'rule' not in group:
        want = set(G.GEMM_MUTATIONS)
        if group.endswith('-f32-bn64') or group.endswith('-f32-bn128'):
            want -= {'pad_nonzero', 'out_unrounded', 'out_trunc', 'out_half_up'}          # an f32 output has no pad columns and no rounding
        if not group.startswith('f32-'):
            want -= {'op_trunc'}                                                            # bf16 A arrives rounded
        assert seen == want, (sorted(want - seen), sorted(seen - want))
