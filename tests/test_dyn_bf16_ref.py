"""CPU checks of tests/dyn_bf16_ref.py, the restatement behind tests/test_gpu_dyn_bf16.py (bf16-operand dynamics forward of metrpo_rollout,
include/metrpo.h metrpo_set_dyn_precision; reference model: training.py:218-269).  The rounding helper is pinned against torch, one case is checked
by hand, the 'exact' case generator is shown to produce order-independent arithmetic, and the random-net bound is shown to discriminate."""
import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import dyn_bf16_ref as R


def _torch_bf16(x):
    return torch.tensor(x).to(torch.bfloat16).to(torch.float32).numpy()


def test_rne_helper_matches_torch_on_random_values():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.randn(20000), rng.randn(20000) * 1e-3, rng.randn(20000) * 1e4, -np.abs(rng.randn(2000))]).astype(np.float32)
    assert np.array_equal(R.bf16_round(x).view(np.uint32), _torch_bf16(x).view(np.uint32))


def test_rne_helper_on_exact_ties_of_both_parities_and_negatives():
    # 1 + 2^-7 m are the bf16 values in [1, 2); a tie sits half way between two of them
    even_tie = np.float32(1.0 + 2.0 ** -8)                     # between 1 (even mantissa) and 1 + 2^-7 (odd): goes DOWN to the even one
    odd_tie = np.float32(1.0 + 2.0 ** -7 + 2.0 ** -8)          # between 1 + 2^-7 (odd) and 1 + 2^-6 (even): goes UP
    x = np.array([even_tie, odd_tie, -even_tie, -odd_tie, np.float32(4.0) * even_tie, np.float32(-0.25) * odd_tie], np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 4.0, -0.25 * (1.0 + 2.0 ** -6)], np.float32)
    assert np.array_equal(R.bf16_round(x), want)
    assert np.array_equal(R.bf16_round(x).view(np.uint32), _torch_bf16(x).view(np.uint32))
    # the other two modes differ exactly where they should
    assert np.array_equal(R.bf16_round(x[:2], 'trunc'), np.array([1.0, 1.0 + 2.0 ** -7], np.float32))
    assert np.array_equal(R.bf16_round(x[:2], 'half_up'), np.array([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6], np.float32))
    just = np.array([np.nextafter(even_tie, np.float32(2)), np.nextafter(even_tie, np.float32(0))], np.float32)
    assert np.array_equal(R.bf16_round(just), np.array([1.0 + 2.0 ** -7, 1.0], np.float32))


def test_hand_computed_step():
    """ns = 10 swimmer, one head, hidden (2,): x = [s2 .. s9, a0, a1] (two columns dropped).  W0 routes x0 to unit 0 and x8 - x1 to unit 1,
    W1 sends unit 0 to dim 0 (x 2) and unit 1 to dim 5 (x -2); diff_std = 1/2.
      s2 = 1 + 2^-8 (an even tie: rounds to 1), s3 = 0.25, a0 = 0.75:  h = relu([1 + 0.5, 0.75 - 0.25 - 1]) = [1.5, 0]
      out0 = 2 * 1.5 + 1 = 4 -> s'0 = s0 + 2;  out5 = -2 * 0 = 0 -> s'5 = s5;  every other dim keeps its state."""
    ns, na = 10, 2
    W0 = np.zeros((1, 10, 2)); W0[0, 0, 0] = 1; W0[0, 8, 1] = 1; W0[0, 1, 1] = -1
    b0 = np.array([[0.5, -1.0]])
    W1 = np.zeros((1, 2, ns)); W1[0, 0, 0] = 2; W1[0, 1, 5] = -2
    b1 = np.zeros((1, ns)); b1[0, 0] = 1
    dm = O.DynamicsEnsemble([W0, W1], [b0, b1], ['relu'], np.zeros(ns + na), np.ones(ns + na), np.zeros(ns), np.full(ns, 0.5), 2, ns, na)
    s = np.zeros((1, ns), np.float32); s[0, 0] = 7; s[0, 2] = 1 + 2.0 ** -8; s[0, 3] = 0.25; s[0, 5] = -3
    ac = np.array([[0.75, -1.0]], np.float32)
    nxt = R.step_all(dm, s, ac)[0, 0]
    want = s[0].astype(np.float64).copy(); want[0] = 9.0
    assert np.array_equal(nxt, want)
    assert R.step_all(dm, s, ac, 'half_up')[0, 0, 0] == 7 + 0.5 * (2 * (1 + 2.0 ** -7 + 0.5) + 1)      # the tie rounded the other way shows up


EXACT = [('swimmer', 1, (128, 128), 17, 'step_rand'), ('half_cheetah', 5, (144, 136), 64, 'step_rand'), ('ant', 5, (100, 72), 129, 'model_med'),
         ('humanoid', 5, (128, 64, 128), 17, 'model_mean'), ('ant', 1, (128, 128), 1, 'model_mean')]


@pytest.mark.parametrize('env,K,hidden,B,sam_mode', EXACT)
def test_exact_generator_is_order_independent(env, K, hidden, B, sam_mode):
    """exact_rollout only returns cases that pass check_exact (nothing changed by the rounding; every partial sum a multiple of the grid below 2^24
    grids).  Shown here independently: float32 accumulation in two very different orders reproduces the float64 sums bit for bit on the recorded layers."""
    dm, theta, pdims, pool, dr, ref = R.exact_rollout(env, K, hidden, B, 3, 2, sam_mode, seed=3)
    rec = []
    again = R.rollout_ref(dm, theta, pdims, env, pool, B, 3, 2, sam_mode, dr['model_idx'], dr['reset_idx'], dr['reset_model'], record=rec)
    R.check_exact(rec)
    assert np.array_equal(again['obs'], ref['obs'])
    assert np.any(ref['obs'][2] != ref['obs'][0])                      # the states move
    for h, W, hr, Wr, b in rec[:2 * len(dm.Ws)]:
        z64 = b + hr @ Wr
        fwd = b.astype(np.float32).copy(); bwd = np.zeros_like(fwd)
        h32, W32 = hr.astype(np.float32), Wr.astype(np.float32)
        acc_f = np.zeros((h32.shape[0], W32.shape[1]), np.float32); acc_b = acc_f.copy()
        for i in range(h32.shape[1]):
            acc_f = acc_f + h32[:, i:i + 1] * W32[i:i + 1]
            j = h32.shape[1] - 1 - i
            acc_b = acc_b + h32[:, j:j + 1] * W32[j:j + 1]
        assert np.array_equal((acc_f + fwd).astype(np.float64), z64) and np.array_equal((fwd + acc_b).astype(np.float64), z64)
    with pytest.raises(AssertionError):                                # a non-representable input is caught
        bad = [(rec[0][0] + np.float32(2.0 ** -12), rec[0][1], R.bf16_round(rec[0][0] + np.float32(2.0 ** -12)).astype(np.float64), rec[0][3], rec[0][4])]
        R.check_exact(bad)


@pytest.mark.parametrize('hidden', R.RANDOM_HIDDEN)
def test_random_net_bound_discriminates(hidden):
    """The random-net GPU test holds the device to 8 x the distance between a float32-accumulating emulation and the restatement.  That bound must tell
    the rounding mode and the presence of rounding apart: truncation and the unrounded float64 model each lie at least 10 bounds away."""
    bound, fig, (dm, s, ac), ref = R.random_bound(hidden)
    print('hidden %s: emulation rel-L2 %.3e, bound %.3e' % (hidden, fig, bound))
    assert 0 < fig < 1e-3
    d_trunc = R.rel_l2_per_head(R.ref_delta(dm, s, ac, 'trunc'), ref)
    d_none = R.rel_l2_per_head(R.ref_delta(dm, s, ac, 'none'), ref)
    print('  truncation %.3e, unrounded %.3e' % (d_trunc.min(), d_none.min()))
    assert d_trunc.min() >= 10 * bound and d_none.min() >= 10 * bound


def test_emulation_reproduces_the_restatement_on_an_exact_case():
    """The emulation is the same arithmetic: on exact data it has nothing to round and equals the restatement."""
    dm, theta, pdims, pool, dr, ref = R.exact_rollout('half_cheetah', 2, (100, 72), 17, 1, 5, 'step_rand', seed=11)
    s = pool.astype(np.float32)[:17]
    ac = np.full((17, dm.na), 0.5, np.float32)
    assert np.array_equal(R.emu_f32_step(dm, s, ac), R.ref_delta(dm, s, ac))
