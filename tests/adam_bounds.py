"""Bounds on one fp32 Adam step (tf.train.AdamOptimizer with SGD on the regulariser) against oracle.dynamics_oracle.adam_expect, shared
by test_gpu_dyn_train_grad.py (the training step) and the direct GEMM tests (EPI_ADAM of csrc/gemm_mfma.h).  NumPy only."""
import numpy as np

U = 2.0 ** -24                                   # fp32 unit round-off
TINY = 4 * 2.0 ** -149                           # a few fp32 subnormal steps: moments of (near-)zero gradients
B1, B2, EPS = (float(np.float32(c)) for c in (0.9, 0.999, 1e-8))     # the fp32 constants the kernels use
C1, C2 = 1.0 - B1, 1.0 - B2                      # 1.0f - 0.9f, 1.0f - 0.999f: exact in fp32 (Sterbenz)


def adam_bounds(w0, m0, v0, g, m1, v1, lr_t, decay):
    """Bounds on |device - adam_expect| for one step, in fp32 rounding units of the terms the kernel forms:
    m1 = b1 m0 + c1 g: two products and a sum, fma-contracted or not: <= 3 u (|b1 m0| + |c1 g|); g itself is known to 1 u
    (g = m / c1 from m = fl(c1 g)): one more u on the c1 g term.  v1 = b2 v0 + c2 g g: three roundings plus 2 u from g: 6 u.
    q = lr_t m1 / (sqrt(v1) + eps): m1's bound through lr_t / den, half v1's relative bound through sqrt, and the product, sqrt,
    sum, quotient (and lr_t's own fp32 rounding): 5 u of |q|.  w1 = w0 - q - decay w0: q's bound plus two roundings of each term,
    held at 3 u (an fp32 emulation of the kernel's arithmetic uses 0.93 of 2 u with reg > 0)."""
    bm = 4 * U * (np.abs(B1 * m0) + np.abs(C1 * g)) + TINY
    bv = 6 * U * (B2 * v0 + C2 * g * g) + TINY
    den = np.sqrt(v1) + EPS
    q = lr_t * m1 / den
    bq = lr_t * bm / den + np.abs(q) * (bv / (2 * np.maximum(v1, TINY)) + 5 * U)
    bw = bq + 3 * U * (np.abs(w0) + np.abs(q) + np.abs(decay * w0)) + TINY
    return bm, bv, bw
