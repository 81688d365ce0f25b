"""The dynamics training step (metrpo_dyn_train_step) as two separate quantities, against oracle/dynamics_oracle.py:

1. the gradient.  A step with lr = 0 leaves the weights bitwise unchanged (lr_t = 0, decay = 0) and leaves the moments at
   m = fl(c1 g), v = fl(c2 g^2), c1 = 1.0f - 0.9f, c2 = 1.0f - 0.999f (both exact in fp32).  get_train_adam reads them back through
   the get_dynamics layout, g = m / c1 is compared with D.model_gradients block by block.  Adam's update does not see the
   gradient's scale, so the weight checks of test_gpu_training.py cannot.
2. the Adam arithmetic.  From an injected state (m0, v0, t0) at the same weights and batch, one step with lr = 1e-3 must give
   D.adam_expect's m1, v1, w1 from that gradient, within a few fp32 ulps of the terms involved (bounds derived in _adam_bounds).

Routes of the step's GEMMs per shape (choose_split, gemm_auto, gemm_mfma_launch, skinny_splits; dyn_train.hip, gemm_mfma.h).
k_gemm_mfma<TM, TN, EPI, TA, TB, AL[, PD 4]>, EPI 1 = BIAS_RELU, 0 = BIAS_ID, 3 = RELU_MASK, 4 = ADAM, 6 = PARTIAL; T/F = true/false.
fwd = hidden layers, out = output layer (gemm_skinny_bias: split-K xS + k_splitk_bias_reduce, or unsplit), dH = input gradients
(l > 0), dW = weight gradient with the Adam update (EPI_ADAM fused, or EPI_PARTIAL xS / kchunk kc (rows of the last split) + k_adam_apply).

  shape                              fwd                   out                dH                       dW
  half_cheetah 23-1024-1024-18 K5    <1,1,1,F,F,F>         <1,1,6,F,F,F,4>x8  <1,1,3,F,T,F>            W0 <1,1,6,T,F,F,4>x7 kc144 (136)
   b1000 (ant 35-..-29, hopper       <1,1,1,F,F,T,4>                          <1,1,3,F,T,T,4>          W1 <1,1,4,T,F,T,4>
   14-..-11 the same)                                                                                  W2 <1,1,6,T,F,F,4>x7 kc144 (136)
  humanoid 76-1024-1024-55 K5 b1000  <1,1,1,F,F,T>, ..T,4>  <1,1,6,F,F,F,4>x8  as above                 W0 <1,1,6,T,F,T,4>x7, W1, W2 as above
  swimmer 10-512-512-10 K5 b1000     <1,1,1,F,F,F>, ..T,4>  <1,1,6,F,F,F,4>x4  <1,1,3,F,T,F>, ..T,T,4>  W0, W2 <1,1,6,T,F,F,4>x8 kc128 (104),
                                                                                                       W1 <1,1,6,T,F,T,4>x4 kc256 (232)
  C3 ant 35-512-512-29 K10 b1000     <1,1,1,F,F,F>, ..T,4>  <1,1,6,F,F,F,4>x4  <1,1,3,F,T,F>, ..T,T,4>  W0, W2 <1,1,6,T,F,F,4>x7 kc144 (136),
                                                                                                       W1 <1,1,4,T,F,T,4>
  C4 humanoid 76-1024x3-55 K20 b1000 <1,2,1,F,F,T>         <1,1,6,F,F,F,4>x3  <1,2,3,F,T,F>, ..T,T>    W0 <1,1,4,T,F,T,4>, W1 W2 <1,2,4,T,F,T>,
                                                                                                       W3 <1,1,4,T,F,F,4>
  hopper 14-50-50-11 K1 b1           <1,1,1,F,F,F>         <1,1,0,F,F,F>      <1,1,3,F,T,F>            all <1,1,4,T,F,F>
  swimmer 10-50-50-10 K3 b15         as K1 b1
  half_cheetah 23-64-64-18 K2 b17    <1,1,1,F,F,F>, ..T>   <1,1,0,F,F,F>      <1,1,3,F,T,F>, ..T,T>    W0, W2 <1,1,4,T,F,F>, W1 <1,1,4,T,F,T>
  ant 35-64-64-29 K3 b255            as b17
  ant 35-64-64-29 K3 b256            as b17                                                            W0, W2 <1,1,6,T,F,F,4>x2 kc128 (128),
                                                                                                       W1 <1,1,6,T,F,T,4>x2 kc128 (128)
  swimmer 10-64-64-10 K3 b257        as b17                                                            x3 kc96 (65), AL as b256
  hopper 14-96-64-48-11 K2 b1000     <1,1,1,F,F,F>, ..T>   <1,1,0,F,F,F>      <1,1,3,F,T,F>, ..T,T>    W0, W3 <1,1,6,T,F,F,4>x8 kc128 (104),
                                                                                                       W1, W2 <1,1,6,T,F,T,4>x8 kc128 (104)

Covered: EPI_ADAM with PD 1 (<1,1> and <1,2> tiles) and PD 4, AL true and false; EPI_PARTIAL + k_adam_apply with AL true and false,
last splits of 136, 104, 232 and 65 rows; the forward output layer split (x3, x4, x8) and unsplit; K = 1; batches 1, 15, 17, 255,
256, 257 and 1000; three hidden layers (with and without split-K).  profiles/r07_dyn_train_coverage.txt lists the kernels this module
launches.
"""
import numpy as np
import pytest
import torch
from oracle import dynamics_oracle as D
import helpers as Hh
import tolerances as TOL
from adam_bounds import U, TINY, B1, B2, EPS, C1, C2, adam_bounds as _adam_bounds      # shared with test_gpu_gemm.py

pytestmark = pytest.mark.gpu

# (id, env, K, hidden, batch rows per model, heads compared with the float64 oracle)
SHAPES = [('params_half_cheetah', 'half_cheetah', 5, (1024, 1024), 1000, None),
          ('params_ant', 'ant', 5, (1024, 1024), 1000, None),
          ('params_hopper', 'hopper', 5, (1024, 1024), 1000, None),
          ('params_humanoid', 'humanoid', 5, (1024, 1024), 1000, None),
          ('params_swimmer', 'swimmer', 5, (512, 512), 1000, None),
          ('C3', 'ant', 10, (512, 512), 1000, None),
          ('C4', 'humanoid', 20, (1024, 1024, 1024), 1000, (0, 10, 19)),
          ('K1_b1', 'hopper', 1, (50, 50), 1, None),
          ('b15', 'swimmer', 3, (50, 50), 15, None),
          ('b17', 'half_cheetah', 2, (64, 64), 17, None),
          ('b255', 'ant', 3, (64, 64), 255, None),
          ('b256', 'ant', 3, (64, 64), 256, None),
          ('b257', 'swimmer', 3, (64, 64), 257, None),
          ('3hidden', 'hopper', 2, (96, 64, 48), 1000, None)]


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def blocks(flat, dm):
    """[n][api layout] -> [(layer, 'W' | 'b', [n, ...])] in get_dynamics' order W0, b0, W1, b1, ..."""
    out, o = [], 0
    for l, (W, b) in enumerate(zip(dm.Ws, dm.bs)):
        n = W.shape[1] * W.shape[2]
        out.append((l, 'W', flat[:, o:o + n].reshape((-1,) + W.shape[1:]))); o += n
        out.append((l, 'b', flat[:, o:o + b.shape[1]])); o += b.shape[1]
    assert o == flat.shape[1]
    return out


def _draw(dm, rng, n):
    """test_gpu_training.data's distribution: states ~ 0.5 N(0, 1), actions clipped to [-1, 1], next state = state + 0.1 N(0, 1)"""
    x = (rng.randn(n, dm.ns + dm.na) * 0.5).astype(np.float32).astype(np.float64)
    x[:, dm.ns:] = np.clip(x[:, dm.ns:], -1, 1)
    y = (x[:, :dm.ns] + rng.randn(n, dm.ns) * 0.1).astype(np.float32).astype(np.float64)
    return x, y


def batch_clear_of_relu_kinks(dm, rows, seed, c=16.0):
    """A training batch (rows * K samples; model k trains on samples b K + k) none of whose relu pre-activations z lies within
    c sqrt(n) u (|W|^T |h| + |b|) of zero, n = the layer's fan-in: device (fp32) and oracle (float64) then take the same relu'
    everywhere.  Observed |z_fp32 - z_64| <= 1.3 sqrt(n) u (...) on these nets; a sample that comes closer is drawn again."""
    K = dm.K
    rng = np.random.RandomState(seed)
    x, y = _draw(dm, rng, rows * K)

    def near_kink(idx, k):
        h = ((x[idx] - dm.in_mean) / dm.in_std)[:, dm.n_drop:]
        near = np.zeros(len(idx), bool)
        for l in range(len(dm.Ws) - 1):
            W, b = dm.Ws[l][k], dm.bs[l][k]
            z = h @ W + b
            near |= (np.abs(z) <= c * np.sqrt(W.shape[0]) * U * (np.abs(h) @ np.abs(W) + np.abs(b))).any(1)
            h = np.maximum(z, 0)
        return idx[near]
    todo = [np.arange(k, rows * K, K) for k in range(K)]
    for _ in range(100):
        todo = [near_kink(idx, k) for k, idx in enumerate(todo)]
        bad = np.concatenate(todo)
        if bad.size == 0:
            return x, y
        x[bad], y[bad] = _draw(dm, rng, bad.size)
    raise AssertionError('could not draw a batch clear of relu kinks')


def setup(env, K, dh, rows, seed):
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, (32, 32), seed=seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    dm.Ws = [f32(w) for w in dm.Ws]; dm.bs = [f32(b) for b in dm.bs]       # the engine holds fp32 copies: start the oracle from those
    for a in ('in_mean', 'in_std', 'diff_mean', 'diff_std'):
        setattr(dm, a, f32(getattr(dm, a)))
    x, y = batch_clear_of_relu_kinks(dm, rows, seed + 1)
    return eng, dm, x, y


def read_gradient(eng, x, y, rows, reg=0.0):
    """-> (m, v, t) after one step with lr = 0 from zero moments (device tensors)"""
    eng.train_reset()
    eng.train_step(x, y, rows, 0.0, reg)
    return eng.get_train_adam()


def rel_l2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def within(err, bound, dm=None, heads=None, what=''):
    """|err| <= bound element by element (through assert_allclose: METRPO_TOL_REPORT records the fraction of the bound used); the
    message names the (head, layer, W | b) blocks that break it"""
    r = np.abs(err) / bound
    msg = what
    if dm is not None and not (r <= 1.0).all():
        msg += ' violations per block: ' + ', '.join('head %d %s%d: %d' % (heads[i], kind, l, n) for l, kind, blk in blocks(r, dm)
                                                    for i, n in enumerate((blk > 1.0).reshape(len(blk), -1).sum(1)) if n)
    np.testing.assert_allclose(r, 0.0, rtol=0, atol=1.0, err_msg=msg)


@pytest.mark.parametrize('sid,env,K,dh,rows,heads', SHAPES, ids=[s[0] for s in SHAPES])
def test_gradient_and_adam_step_match_oracle(sid, env, K, dh, rows, heads):
    eng, dm, x, y = setup(env, K, dh, rows, seed=81)
    heads = list(range(K)) if heads is None else list(heads)
    w0_dev = eng.get_dynamics()
    hsel = torch.tensor(heads, device=w0_dev.device)

    # ---- 1. gradient read-out
    m_dev, v_dev, t = read_gradient(eng, x, y, rows)
    assert t == 1
    assert torch.equal(eng.get_dynamics(), w0_dev)                         # lr = 0: lr_t = 0 and decay = 0
    m2, v2, _ = read_gradient(eng, x, y, rows)
    assert torch.equal(m2, m_dev) and torch.equal(v2, v_dev)               # deterministic: the same batch reads the same bits
    m3, _, _ = read_gradient(eng, x, y, rows, reg=1e-3)
    assert torch.equal(m3, m_dev)                                          # the regulariser goes to SGD, not to Adam
    del m2, v2, m3
    m, v = cpu(m_dev[hsel]), cpu(v_dev[hsel])
    g = m / C1                                                             # within 1 u of the kernel's fp32 gradient
    within(v - C2 * g * g, 6 * U * C2 * g * g + TINY, dm, heads, 'v after the read-out')
    xs, ys = D.split_batch(x, y, rows, K)
    gref = np.zeros_like(g)
    for i, k in enumerate(heads):
        gW, gb = D.model_gradients(dm, k, xs[k], ys[k])
        gref[i] = np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in zip(gW, gb)])
    for (l, kind, got), (_, _, ref) in zip(blocks(g, dm), blocks(gref, dm)):
        for i, k in enumerate(heads):
            np.testing.assert_allclose(rel_l2(got[i], ref[i]), 0.0, rtol=0, atol=TOL.DYN_GRAD_REL_L2,
                                       err_msg='rel-L2, head %d layer %d %s' % (k, l, kind))
            np.testing.assert_allclose(np.abs(got[i] - ref[i]).max() / np.abs(ref[i]).max(), 0.0, rtol=0, atol=TOL.DYN_GRAD_MAX,
                                       err_msg='worst element, head %d layer %d %s' % (k, l, kind))

    # ---- 2. Adam from an injected state, at the same weights and batch: the step sees the gradient g just read
    gen = torch.Generator(device=m_dev.device).manual_seed(5)
    g_dev = m_dev / C1
    rms = torch.sqrt(torch.mean(g_dev * g_dev, dim=1, keepdim=True))
    rnd = lambda: torch.rand(g_dev.shape, generator=gen, device=g_dev.device)
    # b1 m0 ~ c1 g and b2 v0 ~ c2 g^2 (neither the old moment nor the new gradient dominates); m0 of either sign, v0 > 0 even where g = 0
    m0_dev = ((C1 / B1) * (g_dev.abs() + 0.3 * rms) * (0.5 + 1.5 * rnd()) * torch.where(rnd() < 0.5, -1.0, 1.0)).float()
    v0_dev = ((C2 / B2) * (g_dev * g_dev + 0.09 * rms * rms) * (0.5 + 1.5 * rnd())).float()
    m0, v0, w0 = cpu(m0_dev[hsel]), cpu(v0_dev[hsel]), cpu(w0_dev[hsel])
    del g_dev, rms
    lr = 1e-3
    for t0, reg in ((0, 0.0), (3, 1e-3), (10 ** 6, 0.0), (0, 1e-3), (3, 0.0), (10 ** 6, 1e-3)):
        eng.set_dynamics(w0_dev, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
        eng.set_train_adam(m0_dev, v0_dev, t0)
        eng.train_step(x, y, rows, lr, reg)
        m1_dev, v1_dev, t1 = eng.get_train_adam()
        assert t1 == t0 + 1
        got_m, got_v, got_w = cpu(m1_dev[hsel]), cpu(v1_dev[hsel]), cpu(eng.get_dynamics()[hsel])
        lr_t = float(np.float32(D.adam_lr_t(lr, t0 + 1)))                  # formed from the float64 betas on the host, rounded to fp32
        decay = float(np.float32(lr * reg))
        m1, v1, w1 = D.adam_expect(w0, m0, v0, g, lr_t, decay, B1, B2, EPS)
        bm, bv, bw = _adam_bounds(w0, m0, v0, g, m1, v1, lr_t, decay)
        what = 't0 %d reg %g:' % (t0, reg)
        within(got_m - m1, bm, dm, heads, what + ' m1')
        within(got_v - v1, bv, dm, heads, what + ' v1')
        within(got_w - w1, bw, dm, heads, what + ' w1')
        assert np.abs(got_w - w0).max() > 0.1 * lr                         # the step moved the weights (Adam moves each by ~lr)
