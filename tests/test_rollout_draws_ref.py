"""CPU checks of tests/rollout_draws_ref.py, the NumPy restatement of the rollout's Philox stream (csrc/device_common.h) that
tests/test_gpu_rollout_draws.py holds every rollout kernel family against."""
import os
import re
import numpy as np
from conftest import REPO
import rollout_draws_ref as R

HEADER = os.path.join(REPO, 'me-trpo_amd', 'csrc', 'device_common.h')


def test_purpose_numbers_equal_the_header():
    txt = open(HEADER).read()
    m = re.search(r'enum\s*\{([^}]*RNG_STEP[^}]*)\}', txt)
    vals = {k: int(v) for k, v in re.findall(r'(RNG_\w+)\s*=\s*(\d+)', m.group(1))}
    assert vals['RNG_STEP'] == R.RNG_STEP and vals['RNG_SELNOISE'] == R.RNG_SELNOISE and vals['RNG_RESET'] == R.RNG_RESET
    from bptt_stochastic_ref import RNG_BPTT
    assert vals['RNG_BPTT'] == RNG_BPTT and len(set(vals.values())) == len(vals) == 4


def test_philox_known_answer():
    """Random123's known-answer vectors of philox4x32-10 (kat_vectors): the one copy in bptt_stochastic_ref.py that this restatement imports."""
    from bptt_stochastic_ref import philox4x32_10
    one = lambda c, k: [int(v[0]) for v in philox4x32_10([np.array([x], dtype=np.uint64) for x in c], k)]
    assert one((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert one((0xffffffff,) * 4, (0xffffffff, 0xffffffff)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert one((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_counter_tuples_of_one_call_are_distinct():
    for (off, t0, B, T, ns, na) in ((0, 0, 7, 5, 10, 2), (2 ** 32 - 3, 4, 6, 3, 29, 8), (5, 0, 3, 4, 11, 3), (0, 2, 4, 3, 55, 21)):
        tup = []
        for name, genv, t, purpose, c in R.counters(off, t0, B, T, ns, na):
            tup += [(int(g) & 0xFFFFFFFF, int(g) >> 32, int(s), (purpose << 16) | c) for g, s in zip(genv, t)]
        assert len(set(tup)) == len(tup)
        assert len(tup) == T * B * ((na + 1) // 2 + (ns + 3) // 4) + B
        assert all(0 <= w < 2 ** 32 for tu in tup for w in tu)


def test_index_rules_on_hand_computed_words():
    w = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x55555555, 0x55555556], dtype=np.uint64)
    assert R.index32(w, 3).tolist() == [0, 0, 1, 1, 2, 0, 1]               # floor(3 w / 2^32): 0x55555556 is the first word of the second third
    assert R.index32(w, 1000).tolist() == [0, 0, 499, 500, 999, 333, 333]
    assert R.index32(w, 1).tolist() == [0] * 7
    w16 = np.array([0, 0xFFFF, 0xABCD0000, 0x1234FFFF, 0xFFFF8000, 0x00015555, 0x00015556], dtype=np.uint64)
    assert R.index16(w16, 5).tolist() == [0, 4, 0, 4, 2, 1, 1]             # only the low 16 bits count: 0x5555 * 5 >> 16 = 1
    assert R.index16(w16, 3).tolist() == [0, 2, 0, 2, 1, 0, 1]             # 0x5555 * 3 = 0xFFFF -> 0; 0x5556 * 3 = 0x10002 -> 1
    # the two rules read different bits of the same word
    assert int(R.index32(np.uint64(0xFFFF0000), 5)) == 4 and int(R.index16(np.uint64(0xFFFF0000), 5)) == 0


def test_uniform_rounding_edge_gives_radius_zero_and_no_nan():
    # float32(word) + 0.5 rounds to 2^32 from word = 2^32 - 128 on (float32 spacing below 2^32 is 256: the tie at 2^32 - 128 goes to the even 2^32)
    edge = 2 ** 32 - 128
    w = np.array([0, 1, edge - 1, edge, 0xFFFFFFFF], dtype=np.uint64)
    u = R.uniform32(w)
    assert u[0] == 0.5 * 2.0 ** -32 and u[1] == 1.5 * 2.0 ** -32
    assert u[2] == 1.0 - 2.0 ** -24 and u[3] == 1.0 and u[4] == 1.0 and (u > 0).all()
    r = R.radius(w)
    assert r[3] == 0.0 and r[4] == 0.0 and not np.signbit(r).any() and np.isfinite(r).all()
    assert abs(r[0] - np.sqrt(2 * 33 * np.log(2.0))) < 1e-12                # u = 2^-33: the largest radius, 6.76
    n0, n1, rr = R.normal2(w, w[::-1].copy())
    assert np.isfinite(n0).all() and np.isfinite(n1).all() and n0[3] == 0.0 and n1[4] == 0.0


def test_integer_draws_in_range_and_uniform_at_a_million():
    def chi2_ok(v, n):
        cnt = np.bincount(v.ravel(), minlength=n)
        assert cnt.size == n and v.min() >= 0
        e = v.size / n
        return ((cnt - e) ** 2 / e).sum() < (n - 1) + 5.0 * np.sqrt(2.0 * (n - 1))      # 5 sigma of chi^2 with n - 1 degrees of freedom
    B, T = 10000, 100
    for K, n_pool in ((3, 1000), (5, 777), (10, 1000)):
        dr, _ = R.rollout_draws(seed=(K << 40) + 17, stream_offset=0, t0=0, B=B, T=T, K=K, n_pool=n_pool, ns=1, na=1)
        assert dr['model_idx'].shape == (T, B) and dr['reset_idx'].shape == (T + 1, B) == dr['reset_model'].shape
        assert chi2_ok(dr['model_idx'], K) and chi2_ok(dr['reset_model'][1:], K) and chi2_ok(dr['reset_idx'][1:], n_pool)
        assert dr['reset_idx'][0].max() < n_pool and dr['reset_model'][0].max() < K and dr['reset_idx'][0].min() >= 0
        # the step head (high bits of .z) and the reset model (low 16 bits) are independent: their joint table is uniform too
        assert chi2_ok(dr['model_idx'] * K + dr['reset_model'][1:], K * K)


def test_normal_moments_at_a_million():
    dr, rad = R.rollout_draws(seed=(77 << 32) | 5, stream_offset=0, t0=0, B=5000, T=50, K=5, n_pool=100, ns=4, na=4)
    for z in (dr['eps'], dr['sel_noise']):
        assert z.size == 10 ** 6 and np.isfinite(z).all()
        # standard errors at N = 1e6: mean 1e-3, variance 1.4e-3, third moment 3.9e-3, fourth 9.8e-3 -- five of each
        assert abs(z.mean()) < 5e-3 and abs(z.var() - 1.0) < 7e-3 and abs(np.mean(z ** 3)) < 2e-2 and abs(np.mean(z ** 4) - 3.0) < 5e-2
        # the members of a Box-Muller pair, and neighbouring pairs, are uncorrelated
        assert abs(np.mean(z[..., 0] * z[..., 1])) < 1e-2 and abs(np.mean(z[..., 1] * z[..., 2])) < 1e-2
    for k in ('eps', 'sel_noise'):
        assert np.array_equal(rad[k][..., 0], rad[k][..., 1]) and not np.array_equal(rad[k][..., 1], rad[k][..., 2])
        np.testing.assert_allclose(dr[k][..., 0] ** 2 + dr[k][..., 1] ** 2, rad[k][..., 0] ** 2, rtol=1e-12, atol=1e-14)
    assert abs((rad['eps'] < 2.0 ** -6).mean() - 1.2e-4) < 1e-4               # the share the GPU test may leave out of its normals check


def _all_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_chunk_equals_slice_of_one_long_call():
    kw = dict(seed=(9 << 32) | 3, stream_offset=11, B=13, K=5, n_pool=1000, ns=11, na=3)
    whole, wr = R.rollout_draws(t0=0, T=10, **kw)
    for t0, T in ((0, 4), (4, 6), (5, 5), (9, 1)):
        part, pr = R.rollout_draws(t0=t0, T=T, **kw)
        for k in ('eps', 'model_idx', 'sel_noise'):
            assert np.array_equal(part[k], whole[k][t0:t0 + T]), k
        for k in ('reset_idx', 'reset_model'):
            assert np.array_equal(part[k], whole[k][t0:t0 + T + 1]), k
        assert all(np.array_equal(pr[k], wr[k][t0:t0 + T]) for k in pr)
    other, _ = R.rollout_draws(t0=1, T=10, **kw)
    assert not np.array_equal(other['eps'][0], whole['eps'][0]) and np.array_equal(other['eps'][0], whole['eps'][1])


def test_stream_offset_equals_columns_of_a_wider_call():
    for base in (0, 2 ** 32 - 40, 2 ** 40 + 5):
        kw = dict(seed=(0xC0FFEE << 32) | 0xABCDEF, t0=0, T=4, K=3, n_pool=1000, ns=10, na=8)
        wide, wr = R.rollout_draws(stream_offset=base, B=77, **kw)
        for o, B in ((0, 5), (30, 20), (40, 37)):                            # base = 2^32 - 40, o = 30: the env counter carries inside the block
            part, pr = R.rollout_draws(stream_offset=base + o, B=B, **kw)
            assert all(np.array_equal(part[k], wide[k][:, o:o + B]) for k in part)
            assert all(np.array_equal(pr[k], wr[k][:, o:o + B]) for k in pr)
    # the high counter word and the high key word both count
    a, _ = R.rollout_draws(stream_offset=7, B=4, **kw)
    b, _ = R.rollout_draws(stream_offset=7 + 2 ** 32, B=4, **kw)
    c, _ = R.rollout_draws(stream_offset=7, B=4, **dict(kw, seed=0xABCDEF))
    assert not np.array_equal(a['eps'], b['eps']) and not np.array_equal(a['eps'], c['eps'])
    assert not np.array_equal(a['reset_idx'], b['reset_idx']) and not np.array_equal(a['reset_idx'], c['reset_idx'])


def test_restatement_equals_the_bptt_restatement_of_normal4():
    """normal4 here (two normal2 pairs) and in bptt_stochastic_ref.bptt_noise are written independently: same four normals from the same block."""
    import bptt_stochastic_ref as Bs
    seed, K, T, B = (5 << 32) | 9, 2, 3, 6
    ref = Bs.bptt_noise(seed, K, T, B, 4)                                     # counter (b, i, t, RNG_BPTT << 16 | 0)
    for i in range(K):
        for t in range(T):
            genv = (np.uint64(i) << np.uint64(32)) | np.arange(B, dtype=np.uint64)
            x, y, z, w = R.draw_block(seed, genv, np.full(B, t), Bs.RNG_BPTT, 0)
            a0, a1, _ = R.normal2(x, y); b0, b1, _ = R.normal2(z, w)
            np.testing.assert_allclose(np.stack([a0, a1, b0, b1], -1), ref[i, t], rtol=1e-13, atol=1e-15)
