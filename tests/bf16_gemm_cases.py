"""Case table of the direct tests of the bf16 layer GEMM and its weight image (csrc/rollout_bf16.hip: k_gemm_bf16 behind gemm_bf16_pick, k_bf16_wimage,
through Engine.debug_gemm_bf16), with its float64 side.  NumPy only; nothing of the library is imported.

A case names one launch.  op 'gemm': C[h] = act(A[h] . W[h]^T + bias[h]) in one of the three (A type, C type) pairs launch_bf16_layers passes --
(f32, bf16) layer 0, (bf16, bf16) a layer between, (bf16, f32) the output layer -- with the 64- or 128-column tile forced or left to the rule (bn = 0).
`K` is the real contraction length: for f32 A it is Kd = lda (a multiple of 4), for bf16 A the width of the layer in front, whose columns K .. Kp - 1 hold
zeros in A and in the image.  op 'image': W f32 [heads][K][N] -> img bf16 [heads][N][Kp].  build(case) lays every operand out exactly as the device call
sees it, gaps between heads and behind lda filled with NaN, outputs with a sentinel no result can equal; expect(case, prob) states in float64 what every
cell of the output must hold; want_form(case, n_cu) restates the pick rule and the grids.  test_bf16_gemm_cases.py checks this module on the CPU,
test_gpu_bf16_gemm.py runs the table on the device.

Data kinds.  'dyadic': A and W multiples of 1/8 with |x| <= 2 (bf16 holds them exactly), bias a multiple of 1/64 with |b| <= 6 and two planted cells
(below): every product is a multiple of 1/64, every partial sum in any order stays far below 2^24 quanta (headroom), so the f32 accumulation is exact
and an f32 output must EQUAL the float64 result, a bf16 output bf16_round of it bit for bit.  Sums of 4 and more in magnitude carry more than eight
significant bits, so the output rounding really rounds; an odd multiple of 1/64 in [4, 8) is an exact tie.  Per head the bias of column N - 1 is moved so
that cell (M - 1, N - 1) lands on 4 + 1/64 (a tie whose kept bit is even: nearest-even goes down, half-up goes up) and, for N > 1, the bias of column 0
so that cell (0, 0) lands on 4 + 3/64 (a tie whose kept bit is odd: nearest-even goes up, truncation goes down).  'dyadic_small' (tanh): A as above,
W with a few entries of +-1/8, +-1/4 per column at the k positions where the k map can slip, |pre-activation| <= 3.5.  'float': fp32 normals with
magnitudes in [2^-6, 4]; f32 A is rounded by the reference (bf16_round, nearest-even), bf16 A and the image hold rounded values to begin with; an f32
output is held per cell to (n + 2) u (|A| @ |W| + |bias|) on the rounded operands, n the real contraction length, u = 2^-24 (a dot product of n exact
products and a bias added in any order, each sum rounded once); a bf16 output by monotonicity of rounding to
bf16_round(ref - bound) <= got <= bf16_round(ref + bound).
"""
from collections import namedtuple
import numpy as np
from dyn_bf16_ref import bf16_round
import tolerances as TOL

U = 2.0 ** -24
TANH_ATOL = TOL.STEP['atol']
F32_SENTINEL = np.float32(-1.2345e30)
U16_SENTINEL = 0xFFFF                      # a NaN pattern bf16_rne never produces from a finite value (and 0x7FC0-class NaNs only from NaN inputs)
U16_POISON = 0x7FC0                        # bf16 NaN: one stray read turns the cell into NaN
ACT_NAMES = ('identity', 'relu', 'tanh')
TIE_EVEN, TIE_ODD = 4.0 + 1.0 / 64, 4.0 + 3.0 / 64

Case = namedtuple('Case', 'op at ct bn M N K Kp lda heads sa0 act kind seed')


def ceil_div(a, b):
    return -(-a // b)


def gemm_case(at, ct, bn, M, N, K, Kp=None, lda=None, heads=1, sa0=False, act=0, kind='dyadic', seed=0):
    if at == 'f32':
        assert K % 4 == 0 and Kp is None and lda is None
        Kp, lda = (K + 63) & ~63, K
    else:
        assert Kp % 64 == 0 and K <= Kp and not sa0
        lda = Kp if lda is None else lda
    if act == 2 and kind == 'dyadic':
        kind = 'dyadic_small'
    return Case('gemm', at, ct, bn, M, N, K, Kp, lda, heads, sa0, act, kind, seed)


def image_case(K, N, heads, seed):
    return Case('image', 'f32', 'bf16', 0, 0, N, K, (K + 63) & ~63, 0, heads, False, 0, 'ties', seed)


def case_id(c):
    if c.op == 'image':
        return 'image-%dx%d-h%d' % (c.K, c.N, c.heads)
    return '%s-%s-bn%d-%dx%dx%d(%d)-h%d%s-%s-%s%s' % (c.at, c.ct, c.bn, c.M, c.N, c.K, c.Kp, c.heads, 's0' if c.sa0 else '', ACT_NAMES[c.act], c.kind,
                                                    '+lda' if c.lda > max(c.Kp, c.K) else '')


# ------------------------------------------------------------------------------------------------ the host's launch rule, restated
def want_form(c, n_cu):
    """the form the library must report: dict over Engine.BF16_GEMM_FORM_FIELDS"""
    if c.op == 'image':
        return dict(bn=0, gx=c.Kp // 32, gy=ceil_div(c.N, 32), gz=c.heads, n_cu=n_cu)
    rt = ceil_div(c.M, 128)
    bn = c.bn
    if bn == 0:
        bn = 64 if (c.N <= 64 or c.heads * rt * ceil_div(c.N, 128) < n_cu) else 128
    return dict(bn=bn, gx=ceil_div(c.N, bn), gy=rt, gz=c.heads, n_cu=n_cu)


def layout(c):
    if c.op == 'image':
        return dict(sW=c.K * c.N + 5, sC=c.N * c.Kp + 7)
    ldc = ((c.N + 63) & ~63) if c.ct == 'bf16' else c.N
    return dict(ldc=ldc, sC=(c.M + 1) * ldc + 5, sA=0 if c.sa0 else c.M * c.lda + 8, sW=c.N * c.Kp + 16, sB=c.N + 3)


# ------------------------------------------------------------------------------------------------ operands
def bits16(x):
    """bf16-representable f32 values -> their 16 bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not np.any(u & 0xffff), 'not representable in bf16'
    return (u >> 16).astype(np.uint16)


def from_bits16(b):
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(np.float32)


def _dyadic(rng, shape, amp=16):
    return rng.randint(-amp, amp + 1, size=shape).astype(np.float64) / 8.0


def _floats(rng, shape):
    v = np.exp2(rng.uniform(-6.0, 2.0, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32).astype(np.float64)


def _tie_pool():
    even, odd = np.float32(1 + 2.0 ** -8), np.float32(1 + 2.0 ** -7 + 2.0 ** -8)
    near = [np.nextafter(even, np.float32(2)), np.nextafter(even, np.float32(0)), np.nextafter(odd, np.float32(2)), np.nextafter(odd, np.float32(0))]
    return np.array([sg * sc * v for v in [even, odd] + near for sg in (1.0, -1.0) for sc in (1.0, 0.25, 4.0)], np.float32)


class Problem(object):
    """bufs: the device's initial contents (A, W, bias, C; f32 or uint16 arrays), L: layout numbers, A / W / bias: logical operands"""


def _idx3(s_h, ld, H, R, Cc):
    h, r, cc = np.meshgrid(np.arange(H), np.arange(R), np.arange(Cc), indexing='ij')
    return h * s_h + r * ld + cc


def build(c):
    rng = np.random.RandomState(7000 + c.seed)
    p = Problem()
    p.case, p.L, p.bufs = c, layout(c), {}
    L, H, M, N, n, Kp = p.L, c.heads, c.M, c.N, c.K, c.Kp
    if c.op == 'image':
        pool = _tie_pool()
        W = np.where(rng.rand(H, n, N) < 0.5, rng.choice(pool, size=(H, n, N)), _floats(rng, (H, n, N)).astype(np.float32)).astype(np.float32)
        W[0, 0, 0] = np.float32(1 + 2.0 ** -8)                          # a tie whose kept bit is even ...
        if H * n * N > 1:
            W[H - 1, n - 1, N - 1] = np.float32(1 + 2.0 ** -7 + 2.0 ** -8)      # ... and one whose kept bit is odd
        if n * N >= 8:                                                  # +Inf, -Inf and a NaN whose payload sits in the bits that are cut off
            flat = W[0].reshape(-1).view(np.uint32)
            flat[1], flat[2], flat[3] = 0x7f800000, 0xff800000, 0x7f800001
        p.W = W
        fw = np.full(H * L['sW'] + 4, np.nan, np.float32)
        fw[_idx3(L['sW'], N, H, n, N)] = W
        p.bufs['W'] = fw
        p.bufs['C'] = np.full(H * L['sC'] + 4, U16_SENTINEL, np.uint16)
        return p
    HA = 1 if c.sa0 else H
    if c.kind == 'float':
        A, W, bias = _floats(rng, (HA, M, n)), _floats(rng, (H, n, N)), _floats(rng, (H, N))
        W = bf16_round(W).astype(np.float64)                            # the image holds rounded weights
        if c.at == 'bf16':
            A = bf16_round(A).astype(np.float64)
    else:
        A, W = _dyadic(rng, (HA, M, n)), _dyadic(rng, (H, n, N))
        bias = rng.randint(-384, 385, size=(H, N)).astype(np.float64) / 64.0
        if c.kind == 'dyadic_small':
            keep = np.zeros((H, n, N), bool)
            for k in (n - 1, 8 * ((n - 1) // 8), min(64, n - 1), min(127, n - 1), min(8, n - 1)):
                keep[:, k, :] = True
            hh, nn = np.meshgrid(np.arange(H), np.arange(N), indexing='ij')
            keep[hh, rng.randint(n, size=(H, N)), nn] = True
            W = np.where(keep, rng.choice([-2.0, -1.0, 1.0, 2.0], size=W.shape) / 8.0, 0.0)
            bias = _dyadic(rng, (H, N), 4)
        elif c.ct == 'bf16':                                            # the planted ties
            z = bias[:, None, :] + A @ W
            bias[:, N - 1] += TIE_EVEN - z[:, M - 1, N - 1]
            if N > 1:
                bias[:, 0] += TIE_ODD - z[:, 0, 0]
    p.A, p.W, p.bias = A, W, bias
    n_a = (HA - 1) * L['sA'] + M * c.lda + 8
    if c.at == 'f32':
        fa = np.full(n_a, np.nan, np.float32)
        fa[_idx3(L['sA'], c.lda, HA, M, n)] = A
    else:
        fa = np.full(n_a, U16_POISON, np.uint16)
        fa[_idx3(L['sA'], c.lda, HA, M, Kp)] = 0                        # the zero columns width .. Kp - 1 of a hidden-activation buffer
        fa[_idx3(L['sA'], c.lda, HA, M, n)] = bits16(A)
    fw = np.full(H * L['sW'] + 8, U16_POISON, np.uint16)
    fw[_idx3(L['sW'], Kp, H, N, Kp)] = 0                                # the image's k pad
    fw[_idx3(L['sW'], Kp, H, N, n)] = bits16(W.transpose(0, 2, 1))
    fb = np.full(H * L['sB'] + 4, np.nan, np.float32)
    fb[_idx3(L['sB'], N, H, 1, N)] = bias[:, None, :]
    p.bufs['A'], p.bufs['W'], p.bufs['bias'] = fa, fw, fb
    p.bufs['C'] = (np.full(H * L['sC'] + 4, U16_SENTINEL, np.uint16) if c.ct == 'bf16' else np.full(H * L['sC'] + 4, F32_SENTINEL, np.float32))
    return p


def device_fields(c, p):
    """scalar fields of _lib.DebugGemmBf16Args (the pointer fields are p.bufs' names)"""
    L = p.L
    if c.op == 'image':
        return dict(N=c.N, Kd=c.K, Kp=c.Kp, heads=c.heads, sW=L['sW'], sC=L['sC'])
    return dict(a_bf16=int(c.at == 'bf16'), c_bf16=int(c.ct == 'bf16'), bn=c.bn, M=c.M, N=c.N, Kd=(c.lda if c.at == 'f32' else c.Kp), Kp=c.Kp, heads=c.heads,
                lda=c.lda, ldc=L['ldc'], act=c.act, sA=L['sA'], sW=L['sW'], sB=L['sB'], sC=L['sC'])


# ------------------------------------------------------------------------------------------------ the float64 side
GEMM_MUTATIONS = ('k_last_chunk_dropped', 'k_tile2_dropped', 'k_halves_swapped', 'head_prev_w', 'head_prev_bias', 'bias_shifted', 'edge_from_neighbour',
                  'pad_nonzero', 'out_unrounded', 'out_trunc', 'out_half_up', 'op_trunc')
IMAGE_MUTATIONS = ('img_pad_garbage', 'img_trunc', 'img_half_up', 'img_head_prev')


def applies(mut, c):
    if c.op == 'image':
        return {'img_pad_garbage': c.K < c.Kp, 'img_head_prev': c.heads > 1}.get(mut, mut in IMAGE_MUTATIONS)
    exact_bf16 = c.kind == 'dyadic' and c.ct == 'bf16'
    bn = c.bn or want_form(c, 256)['bn']
    return {'k_tile2_dropped': c.K > 64, 'head_prev_w': c.heads > 1, 'head_prev_bias': c.heads > 1, 'bias_shifted': c.N > 1,
            'edge_from_neighbour': c.M > 128 or c.N > bn, 'pad_nonzero': c.ct == 'bf16' and c.N % 64 != 0,
            'out_unrounded': exact_bf16, 'out_half_up': exact_bf16, 'out_trunc': c.ct == 'bf16' and (c.kind != 'dyadic' or c.N > 1),
            'op_trunc': c.kind == 'float' and c.at == 'f32'}.get(mut, mut in GEMM_MUTATIONS)


Expect = namedtuple('Expect', 'idx exact val lo hi centre bound pad')
# idx: flat indices of every cell the launch must write; exact: val must be met bit for bit, else lo <= got <= hi; val: what this (possibly mutated)
# restatement returns, float64 (bf16 outputs: the bf16 value); centre / bound: the unrounded reference and its bound where there is one; pad: mask of
# the zero-written pad cells


def _act(act, z):
    return np.maximum(z, 0.0) if act == 1 else np.tanh(z) if act == 2 else z


def expect(c, p, mut=None):
    if c.op == 'image':
        return expect_image(c, p, mut)
    L, H, M, N, n, Kp = p.L, c.heads, c.M, c.N, c.K, c.Kp
    A, W, bias = p.A, p.W, p.bias
    if c.at == 'f32':
        A = bf16_round(A.astype(np.float32), 'trunc' if mut == 'op_trunc' else 'rne').astype(np.float64)
    Ap = np.zeros((A.shape[0], M, Kp)); Ap[:, :, :n] = A
    Wp = np.zeros((H, Kp, N)); Wp[:, :n, :] = W
    ks = np.arange(Kp)
    if mut == 'k_last_chunk_dropped':
        ks = ks[ks // 8 != (n - 1) // 8]
    if mut == 'k_tile2_dropped':
        ks = ks[ks // 64 != 1]
    ka = ks ^ 8 if mut == 'k_halves_swapped' else ks
    prev = np.maximum(np.arange(H) - 1, 0)
    if mut == 'head_prev_w':
        Wp = Wp[prev]
    if mut == 'head_prev_bias':
        bias = bias[prev]
    if mut == 'bias_shifted':
        bias = np.concatenate([bias[:, 1:], np.zeros((H, 1))], axis=1)
    z = bias[:, None, :] + Ap[:, :, ka] @ Wp[:, ks, :]
    absz = np.abs(bias)[:, None, :] + np.abs(Ap[:, :, ka]) @ np.abs(Wp[:, ks, :])
    y = _act(c.act, z)
    if mut == 'edge_from_neighbour':
        bn = c.bn or want_form(c, 256)['bn']
        y = y.copy()
        if M > 128:
            y[:, M - 1, :] = y[:, M - 1 - 128, :]
        else:
            y[:, :, N - 1] = y[:, :, N - 1 - bn]
    exact = c.kind != 'float' and c.act != 2               # (a tanh case run with act = 0 gives its pre-activation: exact as well)
    bound = None if exact else (np.full(y.shape, TANH_ATOL) if c.act == 2 else (n + 2) * U * absz)
    ldc = L['ldc']
    idx = _idx3(L['sC'], ldc, H, M, ldc)
    pad = np.zeros((H, M, ldc), bool); pad[:, :, N:] = True
    full = lambda x: np.concatenate([x, np.zeros((H, M, ldc - N))], axis=2)
    if c.ct == 'f32':
        lo, hi = (y, y) if exact else (y - bound, y + bound)
        val = y
    else:
        mode = {'out_trunc': 'trunc', 'out_half_up': 'half_up', 'out_unrounded': 'none'}.get(mut, 'rne')
        val = bf16_round(y.astype(np.float32), mode).astype(np.float64)
        if exact:
            assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
            lo = hi = val
        else:
            lo, hi = bf16_round((y - bound).astype(np.float32)).astype(np.float64), bf16_round((y + bound).astype(np.float32)).astype(np.float64)
    val, lo, hi, y = full(val), full(lo), full(hi), full(y)
    bound = None if bound is None else full(bound)
    if mut == 'pad_nonzero':
        val = np.where(pad, float(from_bits16(np.array([U16_SENTINEL], np.uint16))[0]), val)     # left as they were
    return Expect(idx.ravel(), exact, val.ravel(), lo.ravel(), hi.ravel(), y.ravel(), None if bound is None else bound.ravel(), pad.ravel())


def expect_image(c, p, mut=None):
    """-> Expect whose val / lo / hi are the 16 bits every cell of img [heads][N][Kp] must hold (always exact)"""
    L, H, N, n, Kp = p.L, c.heads, c.N, c.K, c.Kp
    W = p.W[np.maximum(np.arange(H) - 1, 0)] if mut == 'img_head_prev' else p.W
    r = bf16_round(W.transpose(0, 2, 1), {'img_trunc': 'trunc', 'img_half_up': 'half_up'}.get(mut, 'rne'))
    img = np.full((H, N, Kp), U16_SENTINEL if mut == 'img_pad_garbage' else 0, np.uint16)
    img[:, :, :n] = (r.view(np.uint32) >> 16).astype(np.uint16)
    pad = np.zeros((H, N, Kp), bool); pad[:, :, n:] = True
    b = img.ravel()
    return Expect(_idx3(L['sC'], Kp, H, N, Kp).ravel(), True, b, b, b, None, None, pad.ravel())


def differs(c, good, bad):
    """would the comparison the device test makes against `good` reject an output equal to `bad`'s?"""
    if c.op == 'image':
        return bool(np.any(bad.val != good.val))
    return bool(np.any(~((bad.val >= good.lo) & (bad.val <= good.hi))))                 # (NaN compares false: rejected)


def headroom(c, p):
    """largest sum of |terms| of any accumulation of a dyadic case in quanta of 1/64: below 2^24 every partial sum of every order is exact in f32"""
    return float((np.abs(p.A) @ np.abs(p.W) + np.abs(p.bias)[:, None, :]).max() * 64.0)


# ------------------------------------------------------------------------------------------------ the table
MS = (1, 31, 32, 33, 127, 128, 129, 257)
NS = (1, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 136, 192, 200)
LDAS = (4, 20, 60, 64, 68, 76, 128, 132)                                          # f32 A: Kp 64, 128, 192; a partial second / third k tile
WIDTHS = ((40, 64), (64, 64), (100, 128), (128, 128), (136, 192), (200, 256), (72, 128), (250, 256))      # bf16 A: (width of the layer in front, Kp)
PAIRS = (('f32', 'bf16'), ('bf16', 'bf16'), ('bf16', 'f32'))
IMG_KD = (1, 31, 32, 33, 63, 64, 65, 76, 128, 129)
IMG_N = (1, 31, 32, 33, 55, 64, 100)


def _contraction(at, i):
    return dict(K=LDAS[i % 8]) if at == 'f32' else dict(K=WIDTHS[i % 8][0], Kp=WIDTHS[i % 8][1])


def _gemm_cases():
    out, seed = [], 0
    for ip, (at, ct) in enumerate(PAIRS):
        for bn in (64, 128):
            ns = [N for N in NS if bn == 64 or N > 64]                            # the library never launches the 128-column tile at N <= 64
            i = 0
            for ps in range(1 if bn == 64 else 2):
                for j, N in enumerate(ns):
                    M = MS[(j + 3 * ps + ip) % 8]
                    heads = 3 if i % 2 else 1
                    kw = dict(_contraction(at, i + ip), heads=heads, sa0=(at == 'f32' and i % 4 == 1))
                    seed += 1
                    out.append(gemm_case(at, ct, bn, M, N, act=i % 3, seed=seed, **kw))
                    if i % 2 == 0:                                                # the float twin (relu where the dyadic case has tanh)
                        seed += 1
                        out.append(gemm_case(at, ct, bn, M, N, act=(0, 1, 1)[i % 3], kind='float', seed=seed, **kw))
                    i += 1
    # lda > Kp: the columns behind Kp hold NaN and are never read
    for (ct, bn, M, N, (w, Kp), act) in (('bf16', 64, 33, 65, WIDTHS[0], 1), ('bf16', 128, 129, 136, WIDTHS[2], 0), ('f32', 64, 127, 31, WIDTHS[4], 0),
                                         ('f32', 128, 31, 100, WIDTHS[5], 1)):
        for kind in ('dyadic', 'float'):
            seed += 1
            out.append(gemm_case('bf16', ct, bn, M, N, K=w, Kp=Kp, lda=Kp + 8 * (1 + seed % 3), heads=3, act=act, kind=kind, seed=seed))
    # the rule itself (bn = 0) where it does not depend on the CU count: N = 64 stays on the 64-column tile whatever the grid, N = 65 with a handful of tiles too
    for at, ct in (('f32', 'bf16'), ('bf16', 'f32')):
        for N in (64, 65):
            seed += 1
            out.append(gemm_case(at, ct, 0, 129, N, heads=3, act=1, seed=seed, **_contraction(at, 3)))
    return out


def threshold_cases(n_cu):
    """bn = 0 at heads * rt * ct = n_cu - 1 (64-column tiles) and = n_cu (128-column tiles): one head, one 128-column tile, N = 65"""
    return [gemm_case('f32', 'bf16', 0, M, 65, K=4, heads=1, act=1, seed=900 + i) for i, M in enumerate((128 * (n_cu - 1), 128 * (n_cu - 1) + 1))]


def _image_cases():
    out = []
    for ps in range(2):
        for i, Kd in enumerate(IMG_KD):
            out.append(image_case(Kd, IMG_N[(i + 1 + 3 * ps) % 7], 3 if (i + ps) % 2 else 1, 500 + len(out)))
    return out


GEMM_CASES = _gemm_cases()
IMAGE_CASES = _image_cases()
CASES = GEMM_CASES + IMAGE_CASES


def group_of(c, n_cu=256):
    """the instantiation a case pins: (A type, C type, bn as launched), 'rule' cases under their own name, the image"""
    if c.op == 'image':
        return 'image'
    return '%s-%s-%s%d' % (c.at, c.ct, 'rule' if c.bn == 0 else 'bn', want_form(c, n_cu)['bn'])


def cases_by_group():
    d = {}
    for c in CASES:
        d.setdefault(group_of(c), []).append(c)
    return d
