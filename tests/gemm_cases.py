"""Case table of the direct tests of the shared MFMA GEMM (csrc/gemm_mfma.h through Engine.debug_gemm), with its float64 side.  NumPy only.

A case names one call: the entry (`op`), the epilogue, the transposes, a forced tile or the entry's own rule, the extents, layout quirks and
the data kind.  build(case) lays the operands out in flat float32 buffers exactly as the device call sees them (gaps filled with POISON,
outputs with SENTINEL), expect(case, prob) states in float64 what every written cell must hold and which cells may be written at all, and
want_form(case) restates the host's launch rules (gemm_auto_tile, gemm_launch_form, skinny_plan, gemm_fused_out_tile) so that the form the
library reports can be asserted.  test_gemm_cases.py checks this module on the CPU (coverage of the forms, exactness of the dyadic data,
and that the checks see each restatement mutation); test_gpu_gemm.py runs the table on the device.

Data kinds.  'dyadic': every operand a multiple of 1/8, |value| <= amp / 8 <= 2, so that every product and every partial sum in any
order is exact in fp32 and the device must return the float64 result bit for bit ('dyadic_small': as dyadic, W sparse so that the
pre-activation stays within [-2, 2] for the tanh epilogue).  'float': fp32 normals with magnitudes in [2^-6, 4], held to
(n + 2) u (|opA(A)| @ |opB(W)| + |bias|), the bound of a dot product of n terms summed in any order with each product and sum rounded at
most once (u = 2^-24).
"""
from collections import namedtuple
import numpy as np
from oracle.dynamics_oracle import adam_expect
from adam_bounds import B1, B2, EPS, adam_bounds

U = 2.0 ** -24
POISON = np.float32(3.0e4 + 0.3)          # fills what no kernel may read: one stray read breaks exactness and every bound
SENTINEL = np.float32(-1.2345e30)         # fills what a kernel writes or must leave alone
BK = 16

_FIELDS = ('op epi ta tb tm tn M N Kd heads kind amp lda_pad ldw_pad ldc_pad a_off w_off sa_pad sw_pad splits kchunk act defer use_part '
           'no decay seed')
Case = namedtuple('Case', _FIELDS)
_DEFAULTS = dict(ta=False, tb=False, tm=0, tn=0, heads=1, kind='dyadic', amp=16, lda_pad=0, ldw_pad=0, ldc_pad=0, a_off=0, w_off=0, sa_pad=0,
                 sw_pad=0, splits=0, kchunk=0, act=0, defer=False, use_part=False, no=0, decay=0.0, seed=0)


def case(op, epi, M, N, Kd, **kw):
    d = dict(_DEFAULTS); d.update(kw)
    return Case(op=op, epi=epi, M=M, N=N, Kd=Kd, **d)


def case_id(c):
    q = ''.join(s for s, on in (('+lda', c.lda_pad), ('+ldw', c.ldw_pad), ('+ldc', c.ldc_pad), ('+aoff', c.a_off), ('+woff', c.w_off),
                                ('+sA', c.sa_pad), ('+sW', c.sw_pad)) if on)
    return '%dx%dx%d-h%d-%s%s' % (c.M, c.N, c.Kd, c.heads, c.kind, q)


# ------------------------------------------------------------------------------------------------ the host's launch rules, restated
def ceil_div(a, b):
    return -(-a // b)


def auto_tile(M, N, heads):
    blocks = lambda tm, tn: ceil_div(M, 64 * tm) * ceil_div(N, 64 * tn) * heads
    tm, tn = (2 if M > 64 else 1), (2 if N > 64 else 1)
    if tm == 2 and blocks(tm, tn) < 2048:
        tm = 1
    if tn == 2 and blocks(tm, tn) < 2048:
        tn = 1
    return tm, tn


def fused_out_tile(M, N, heads, no):
    blocks = lambda tm, tn: ceil_div(M, 64 * tm) * ceil_div(N, 64 * tn) * heads
    if no > 64:
        return 0
    if M > 64 and N > 64 and N % 128 == 0 and blocks(2, 2) >= 2048:
        return 2
    if N % 64 == 0 and blocks(2, 1) < 2048 and blocks(1, 2) < 2048:
        return 1
    return 0


def skinny_plan(M, N, Kd, heads, have_part):
    """-> (splits, kchunk, stridePart); splits 1: one unsplit launch writes C"""
    S = 1
    blocks = ceil_div(M, 64) * ceil_div(N, 64) * heads
    if Kd >= 256 and blocks < 512:
        S = max(min(min(8, max(1, 1024 // max(blocks, 1))), Kd // 128), 1)
    if S <= 1 or not have_part:
        return 1, Kd, 0
    kchunk = (ceil_div(Kd, S) + 15) & ~15
    return ceil_div(Kd, kchunk), kchunk, (M * N + N + 3) & ~3


def layout(c):
    """leading dimensions, head strides and base offsets (floats) of the operands as stored"""
    a_rows, a_cols = (c.Kd, c.M) if c.ta else (c.M, c.Kd)
    w_rows, w_cols = (c.N, c.Kd) if c.tb else (c.Kd, c.N)
    lda, ldw = a_cols + c.lda_pad, w_cols + c.ldw_pad
    L = dict(lda=lda, ldw=ldw, sA=a_rows * lda + c.sa_pad, sW=w_rows * ldw + c.sw_pad, a_rows=a_rows, a_cols=a_cols, w_rows=w_rows, w_cols=w_cols)
    if c.op == 'auto':
        L['ldc'] = c.N + c.ldc_pad
        L['sC'] = (c.M + 1) * L['ldc'] + 5                  # a guard row and a gap between heads
    else:
        L['ldc'] = c.N
        L['sC'] = c.M * c.N + 7
    return L


def want_form(c):
    """the form the library must report for this case: dict over Engine.GEMM_FORM_FIELDS"""
    L = layout(c)
    splits, kchunk, stride, reduced, epi = 0, c.Kd, 0, 0, c.epi
    if c.op == 'auto':
        tm, tn = (c.tm, c.tn) if c.tm else ((1, 1) if (c.epi == 'PARTIAL' and not c.ta) else auto_tile(c.M, c.N, c.heads))
        if c.epi == 'PARTIAL':
            splits, kchunk, stride = c.splits, c.kchunk, part_stride(c)
    elif c.op == 'skinny':
        s, kc, st = skinny_plan(c.M, c.N, c.Kd, c.heads, c.use_part)
        if s <= 1:
            tm, tn = auto_tile(c.M, c.N, c.heads)
        else:
            tm, tn, epi, splits, kchunk, stride = 1, 1, 'PARTIAL', s, kc, st
            reduced = 0 if (c.defer and c.act == 0) else 1
    else:
        tm = tn = c.tm if c.tm else fused_out_tile(c.M, c.N, c.heads, c.no)
        splits, stride = c.N // (64 * tm), (c.M * c.no + 3) & ~3
    m4 = lambda v: v % 4 == 0
    al = (m4(c.a_off) and m4(c.w_off) and m4(L['sA']) and m4(L['sW']) and m4(L['lda']) and m4(L['ldw']) and m4(c.M if c.ta else c.Kd) and
          m4(c.Kd if c.tb else c.N) and (epi != 'PARTIAL' or m4(kchunk)))
    gx, gy, gz = ceil_div(c.N, 64 * tn), ceil_div(c.M, 64 * tm), c.heads * (splits if epi == 'PARTIAL' else 1)
    pd = 4 if (tm * tn == 1 and gx * gy * gz <= 1280 and c.Kd >= 256) else 1
    return dict(tm=tm, tn=tn, al=int(al), pd=pd, splits=splits, kchunk=kchunk, gx=gx, gy=gy, gz=gz, reduced=reduced, stride_part=stride)


def part_stride(c):
    return c.M * c.N + c.N + 5                              # op auto, PARTIAL: five floats between a partial's end and the next


Form = namedtuple('Form', 'op variant ta tb tm tn al pd')


def form_of(c):
    """the instantiation a case pins; gemm_skinny_bias's cases are grouped by its arguments (the kernel it launches depends on the shape)"""
    w = want_form(c)
    if c.op == 'skinny':
        return Form('skinny', 'act%d%s%s' % (c.act, '-defer' if c.defer else '', '-part' if c.use_part else ''), False, False, 0, 0, 0, 0)
    variant = c.epi if c.op == 'auto' else ('RELU_OUT' if c.no <= 32 else 'RELU_OUT48' if c.no <= 48 else 'RELU_OUT64')
    return Form(c.op, variant, c.ta, c.tb, w['tm'], w['tn'], w['al'], w['pd'])


# ------------------------------------------------------------------------------------------------ operands
def _dyadic(rng, shape, amp):
    return rng.randint(-amp, amp + 1, size=shape).astype(np.float64) / 8.0


def _floats(rng, shape):
    v = np.exp2(rng.uniform(-6.0, 2.0, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32).astype(np.float64)


def _store(flat, off, stride_h, ld, x, transposed):
    """x [heads, R, Cc] logical -> flat[off + h stride_h + r ld + c] (or the transpose of each head)"""
    if transposed:
        x = x.transpose(0, 2, 1)
    h, r, cc = np.meshgrid(np.arange(x.shape[0]), np.arange(x.shape[1]), np.arange(x.shape[2]), indexing='ij')
    idx = off + h * stride_h + r * ld + cc
    flat[idx] = x
    return idx


def _gather(flat, off, stride_h, ld, heads, R, Cc, transposed, head_shift=0):
    """the reading side of _store, with the index formula spelled out again (mutations flip `transposed` or shift the head)"""
    h, r, cc = np.meshgrid(np.arange(heads), np.arange(R), np.arange(Cc), indexing='ij')
    h = np.maximum(h - head_shift, 0)
    idx = off + h * stride_h + (cc * ld + r if transposed else r * ld + cc)
    return flat[idx % flat.size].astype(np.float64)


class Problem(object):
    """flat float32 buffers `bufs` (the device's initial contents), layout numbers `L`, logical float64 operands"""


def build(c):
    rng = np.random.RandomState(1000 + c.seed)
    p = Problem()
    p.case, p.L, p.bufs = c, layout(c), {}
    L, H, M, N, Kd = p.L, c.heads, c.M, c.N, c.Kd
    if c.kind == 'float':
        A, W = _floats(rng, (H, M, Kd)), _floats(rng, (H, Kd, N))
        bias, w2 = _floats(rng, (H, N)), _floats(rng, (H, N, max(c.no, 1)))
    else:
        A, W = _dyadic(rng, (H, M, Kd), c.amp), _dyadic(rng, (H, Kd, N), c.amp)
        bias, w2 = _dyadic(rng, (H, N), c.amp), _dyadic(rng, (H, N, max(c.no, 1)), c.amp)
        if c.kind == 'dyadic_small':            # per column three entries of |w| <= 1/4 (the last k, the first k of the last k-tile, a random one): |z| <= 1.5 + 1/2
            keep = np.zeros((H, Kd, N), bool)
            keep[:, Kd - 1, :] = True
            keep[:, BK * ((Kd - 1) // BK), :] = True
            hh, nn = np.meshgrid(np.arange(H), np.arange(N), indexing='ij')
            keep[hh, rng.randint(Kd, size=(H, N)), nn] = True
            W = np.where(keep, rng.choice([-2.0, -1.0, 1.0, 2.0], size=W.shape) / 8.0, 0.0)
            bias = _dyadic(rng, (H, N), 4)
    mask = _dyadic(rng, (H, M, N), 7)           # DTANH: a hidden tanh activation, |hm| < 1; RELU_MASK: its sign decides
    p.A, p.W, p.bias, p.mask, p.w2 = A, W, bias, mask, w2
    fa = np.full(c.a_off + H * L['sA'] + 4, POISON, np.float32); _store(fa, c.a_off, L['sA'], L['lda'], A, c.ta)
    fw = np.full(c.w_off + H * L['sW'] + 4, POISON, np.float32); _store(fw, c.w_off, L['sW'], L['ldw'], W, c.tb)
    p.bufs['A'], p.bufs['W'] = fa, fw
    L['sBias'] = N + 3
    fb = np.full(H * L['sBias'], POISON, np.float32); _store(fb, 0, L['sBias'], N, bias[:, None, :], False)
    p.bufs['bias'] = fb
    if c.epi in ('RELU_MASK', 'DTANH'):
        L['ldm'] = N + 2; L['sMask'] = M * L['ldm'] + 3
        fm = np.full(H * L['sMask'], POISON, np.float32); _store(fm, 0, L['sMask'], L['ldm'], mask, False)
        p.bufs['mask'] = fm
    if c.op == 'fused_out':
        L['sW2'] = N * c.no + 1
        f2 = np.full(H * L['sW2'], POISON, np.float32); _store(f2, 0, L['sW2'], c.no, w2, False)
        p.bufs['w2'] = f2
    w = want_form(c)
    p.want = w
    if c.epi == 'ADAM' and c.op == 'auto':      # C is the weight matrix, am / av share its layout; the bias vectors share its head stride
        p.w0 = _floats(rng, (H, M, N))
        p.m0 = _floats(rng, (H, M, N)) * 0.1
        p.v0 = np.abs(_floats(rng, (H, M, N))) * 0.01
        p.bw0, p.bm0, p.bv0 = _floats(rng, (H, N)), _floats(rng, (H, N)) * 0.1, np.abs(_floats(rng, (H, N))) * 0.01
        for name, x in (('C', p.w0), ('am', p.m0), ('av', p.v0)):
            f = np.full(H * L['sC'], SENTINEL, np.float32); _store(f, 0, L['sC'], L['ldc'], x, False); p.bufs[name] = f
        for name, x in (('bvec', p.bw0), ('bam', p.bm0), ('bav', p.bv0)):
            f = np.full(H * L['sC'], SENTINEL, np.float32); _store(f, 0, L['sC'], N, x[:, None, :], False); p.bufs[name] = f
        p.lr_t = float(np.float32(1e-3 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)))
    elif not (c.op == 'auto' and c.epi == 'PARTIAL') and c.op != 'fused_out':
        p.bufs['C'] = np.full(H * L['sC'] + 4, SENTINEL, np.float32)
    if w['splits'] and w['stride_part']:
        p.bufs['part'] = np.full(w['splits'] * H * w['stride_part'] + 8, SENTINEL, np.float32)
    return p


def device_fields(c, p):
    """scalar fields of _lib.DebugGemmArgs (the pointer fields are p.bufs' names; A and W take the offsets c.a_off, c.w_off)"""
    L = p.L
    f = dict(ta=int(c.ta), tb=int(c.tb), tm=c.tm, tn=c.tn, M=c.M, N=c.N, Kd=c.Kd, heads=c.heads, lda=L['lda'], ldw=L['ldw'], ldc=L['ldc'],
             strideA=L['sA'], strideW=L['sW'], strideC=L['sC'], strideBias=L['sBias'], act=c.act, defer=int(c.defer), no=c.no)
    if 'mask' in p.bufs:
        f.update(ldm=L['ldm'], strideMask=L['sMask'])
    if c.op == 'fused_out':
        f.update(strideW2=L['sW2'])
    if c.op == 'auto' and c.epi == 'PARTIAL':
        f.update(splits=c.splits, kchunk=c.kchunk, stridePart=part_stride(c))
    if c.op == 'auto' and c.epi == 'ADAM':
        f.update(strideAdam=L['sC'], lr_t=p.lr_t, beta1=B1, beta2=B2, eps=EPS, decay=float(np.float32(c.decay)))
    return f


def pointer_names(c, p):
    names = [n for n in ('A', 'W', 'C', 'mask', 'w2', 'part', 'am', 'av', 'bvec', 'bam', 'bav') if n in p.bufs]
    if not (c.op == 'auto' and (c.epi in ('RELU_MASK', 'PLAIN', 'PARTIAL', 'ADAM') or (c.epi == 'DTANH' and c.tb))):
        names.append('bias')                   # DTANH<F, T> (the policy's back-propagation) passes no bias
    if c.op == 'skinny' and not c.use_part and 'part' in names:
        names.remove('part')
    return names


# ------------------------------------------------------------------------------------------------ the float64 side
MUTATIONS = ('k_last_dropped', 'k_tile_first_dropped', 'ta_flipped', 'tb_flipped', 'head_prev', 'bias_shifted', 'mask_row_off',
             'colsum_last_slice', 'split_overrun', 'edge_from_neighbour')


def applies(mut, c):
    w = want_form(c)
    has_bias = c.op != 'auto' or c.epi in ('BIAS_ID', 'BIAS_RELU', 'BIAS_TANH') or (c.epi == 'DTANH' and not c.tb)
    colsum = c.epi in ('PARTIAL', 'ADAM') or (c.op == 'skinny' and w['splits'] > 1)
    return {'head_prev': c.heads > 1, 'bias_shifted': has_bias and c.N > 1, 'mask_row_off': c.epi in ('RELU_MASK', 'DTANH') and c.M > 1,
            'colsum_last_slice': colsum, 'split_overrun': w['splits'] > 1 and c.op != 'fused_out',
            'edge_from_neighbour': c.M > 64 * w['tm'] or c.N > 64 * w['tn'],
            'ta_flipped': c.M > 1 and c.Kd > 1, 'tb_flipped': c.N > 1 and c.Kd > 1}.get(mut, True)


def quantum(c):
    """the smallest change exact dyadic arithmetic can make to an output cell"""
    if c.op == 'fused_out':
        return 2.0 ** -9                        # (a w + b) w2: 1/64 times 1/8
    return 2.0 ** -12 if c.epi == 'DTANH' else 2.0 ** -6


def expect(c, p, mut=None):
    """-> {buffer name: (flat indices, float64 reference, bound or None)}.  bound None: the cells must hold the reference bit for bit
    (dyadic data); bound 'tanh': the tanh allowance; an array: |got - ref| <= bound cell by cell.  Cells of an output buffer that no
    entry lists must keep their initial contents.  `mut` restates the operation with one mistake (test_gemm_cases.py)."""
    L, H, M, N, Kd, w = p.L, c.heads, c.M, c.N, c.Kd, p.want
    fa, fw, fb = p.bufs['A'], p.bufs['W'], p.bufs['bias']
    ta = c.ta != (mut == 'ta_flipped'); tb = c.tb != (mut == 'tb_flipped')
    A = _gather(fa, c.a_off, L['sA'], L['lda'], H, M, Kd, ta, head_shift=1 if mut == 'head_prev' else 0)         # opA(A) [H, M, Kd]
    W = _gather(fw, c.w_off, L['sW'], L['ldw'], H, Kd, N, tb)                                                      # opB(W) [H, Kd, N]
    if mut == 'ta_flipped' or mut == 'tb_flipped':
        A, W = np.where(np.abs(A) > 1e4, 0.0, A), np.where(np.abs(W) > 1e4, 0.0, W)       # a flipped reader sees gaps: keep the sums finite and readable
    bias = _gather(fb, 1 if mut == 'bias_shifted' else 0, L['sBias'], N, H, 1, N, False)[:, 0, :]
    if mut == 'bias_shifted':
        bias = np.where(np.abs(bias) > 1e4, 0.0, bias)
    exact = c.kind != 'float'
    tm, tn = w['tm'], w['tn']

    def contract(k0, k1, colsum_slices=False):
        """(sum over k in [k0, k1) of A[:, :, k] W[:, k, :], column sums of W over the same rows, sum of |a||w|, sum of |w|)"""
        ks = np.arange(k0, k1)
        if mut == 'k_last_dropped' and k1 == Kd:
            ks = ks[:-1]
        if mut == 'k_tile_first_dropped' and k1 == Kd:
            ks = ks[ks != k0 + BK * ((k1 - k0 - 1) // BK)]
        cs = ks
        if mut == 'colsum_last_slice':
            cs_k = BK // (256 // (64 * tn))
            cs = ks[(ks - k0) % BK < BK - cs_k]
        a, ww = A[:, :, ks], W[:, ks, :]
        return a @ ww, W[:, cs, :].sum(1), np.abs(a) @ np.abs(ww), np.abs(W[:, cs, :]).sum(1)

    def neighbour(x):
        """the edge row (or column) written from the neighbouring tile"""
        if mut != 'edge_from_neighbour':
            return x
        x = x.copy()
        if M > 64 * tm:
            x[..., M - 1, :] = x[..., M - 1 - 64 * tm, :]
        else:
            x[..., :, N - 1] = x[..., :, N - 1 - 64 * tn]
        return x

    hh, mm, nn = np.meshgrid(np.arange(H), np.arange(M), np.arange(N), indexing='ij')
    hb, nb = np.meshgrid(np.arange(H), np.arange(N), indexing='ij')
    out = {}
    n_terms = Kd

    def partials(splits, kchunk, stride):
        tot, tot_abs = 0.0, 0.0
        idx, ref, bnd = [], [], []
        for s in range(splits):
            k0, k1 = s * kchunk, min(Kd, (s + 1) * kchunk)
            if mut == 'split_overrun':
                k1 = min(Kd, (s + 2) * kchunk)
            acc, csum, aabs, cabs = contract(k0, k1)
            acc = neighbour(acc)
            base = (s * H + hh) * stride
            idx += [(base + mm * N + nn).ravel(), ((s * H + hb) * stride + M * N + nb).ravel()]
            ref += [acc.ravel(), csum.ravel()]
            bnd += [((k1 - k0 + 2) * U * aabs).ravel(), ((k1 - k0 + 2) * U * cabs).ravel()]
            tot, tot_abs = tot + acc, tot_abs + aabs
        return np.concatenate(idx), np.concatenate(ref), (None if exact else np.concatenate(bnd)), tot, tot_abs

    if c.op == 'auto' and c.epi == 'PARTIAL':
        idx, ref, bnd, _, _ = partials(c.splits, c.kchunk, part_stride(c))
        out['part'] = (idx, ref, bnd)
        return out
    if c.op == 'skinny' and w['splits'] > 1:
        idx, ref, bnd, acc, aabs = partials(w['splits'], w['kchunk'], w['stride_part'])
        out['part'] = (idx, ref, bnd)
        n_terms = Kd + w['splits']
        if not w['reduced']:
            return out
    else:
        acc, csum, aabs, cabs = contract(0, Kd)
        acc = neighbour(acc) if c.op != 'fused_out' else acc
    cidx = (hh * L['sC'] + mm * L['ldc'] + nn).ravel()
    fbound = lambda extra=0.0: None if exact else ((n_terms + 2) * U * (aabs + extra)).ravel()
    if c.op == 'fused_out':
        # one M x no partial per column block of 64 tile columns: relu(acc + bias) of the block's columns times the block's rows of w2
        w2 = _gather(p.bufs['w2'], 0, L['sW2'], c.no, H, N, c.no, False)
        h1 = np.maximum(acc + bias[:, None, :], 0.0)
        e1 = (Kd + 2) * U * (aabs + np.abs(bias[:, None, :]))                          # bound on the hidden activation (relu is 1-Lipschitz)
        bn = 64 * tm
        ho, mo, jo = np.meshgrid(np.arange(H), np.arange(M), np.arange(c.no), indexing='ij')
        idx, ref, bnd = [], [], []
        for b in range(N // bn):
            cols = slice(b * bn, (b + 1) * bn)
            r = h1[:, :, cols] @ w2[:, cols, :]
            if mut == 'edge_from_neighbour' and M > bn:
                r[:, M - 1, :] = r[:, M - 1 - bn, :]
            # the hidden cell's own error carried through |w2|, plus the second dot product of bn terms on the device's hidden values
            bb = e1[:, :, cols] @ np.abs(w2[:, cols, :]) + (bn + 2) * U * ((h1 + e1)[:, :, cols] @ np.abs(w2[:, cols, :]))
            idx.append(((b * H + ho) * w['stride_part'] + mo * c.no + jo).ravel()); ref.append(r.ravel()); bnd.append(bb.ravel())
        out['part'] = (np.concatenate(idx), np.concatenate(ref), None if exact else np.concatenate(bnd))
        return out
    epi = c.epi if c.op == 'auto' else ('BIAS_ID', 'BIAS_RELU', 'BIAS_TANH')[c.act]
    if epi in ('RELU_MASK', 'DTANH'):
        hm = _gather(p.bufs['mask'], L['ldm'] if mut == 'mask_row_off' else 0, L['sMask'], L['ldm'], H, M, N, False)
        hm = np.where(np.abs(hm) > 1e4, 0.0, hm)
    if epi == 'BIAS_ID':
        out['C'] = (cidx, (acc + bias[:, None, :]).ravel(), fbound(np.abs(bias[:, None, :])))
    elif epi == 'BIAS_RELU':
        out['C'] = (cidx, np.maximum(acc + bias[:, None, :], 0.0).ravel(), fbound(np.abs(bias[:, None, :])))
    elif epi == 'BIAS_TANH':
        out['C'] = (cidx, np.tanh(acc + bias[:, None, :]).ravel(), 'tanh')
        p.pre_max = float(np.abs(acc + bias[:, None, :]).max())
    elif epi == 'RELU_MASK':
        out['C'] = (cidx, np.where(hm > 0, acc, 0.0).ravel(), fbound())
    elif epi == 'PLAIN':
        out['C'] = (cidx, acc.ravel(), fbound())
    elif epi == 'DTANH':
        z = acc + (0.0 if c.tb else bias[:, None, :])
        out['C'] = (cidx, (z * (1.0 - hm * hm)).ravel(), None)
    elif epi == 'ADAM':
        dec = float(np.float32(c.decay))
        for g, names, x0, idx in ((acc, ('C', 'am', 'av'), (p.w0, p.m0, p.v0), cidx),
                                  (csum, ('bvec', 'bam', 'bav'), (p.bw0, p.bm0, p.bv0), (hb * L['sC'] + nb).ravel())):
            m1, v1, w1 = adam_expect(x0[0], x0[1], x0[2], g, p.lr_t, dec, B1, B2, EPS)
            bm, bv, bw = adam_bounds(x0[0], x0[1], x0[2], g, m1, v1, p.lr_t, dec)
            for name, r, b in zip(names, (w1, m1, v1), (bw, bm, bv)):
                out[name] = (idx, r.ravel(), b.ravel())
    return out


def headroom(c, p):
    """largest sum of |terms| of any accumulation of the case, in quanta of its products: below 2^24 every partial sum of every order is exact"""
    A, W = np.abs(p.A), np.abs(p.W)
    s1 = (A @ W + np.abs(p.bias[:, None, :])).max() * 64.0
    worst = max(s1, np.abs(p.W).sum(1).max() * 8.0)
    if c.op == 'fused_out':
        h = A @ W + np.abs(p.bias[:, None, :])
        bn = 64 * p.want['tm']
        worst = max(worst, max((h[:, :, b * bn:(b + 1) * bn] @ np.abs(p.w2[:, b * bn:(b + 1) * bn, :])).max() for b in range(c.N // bn)) * 512.0)
    if c.epi == 'DTANH':
        worst = max(worst, (A @ W + np.abs(p.bias[:, None, :])).max() * 4096.0)
    return worst


# ------------------------------------------------------------------------------------------------ the table
AUTO_COMBOS = (('BIAS_ID', False, False), ('BIAS_RELU', False, False), ('BIAS_TANH', False, False), ('RELU_MASK', False, True), ('PLAIN', False, True),
               ('DTANH', False, False), ('DTANH', False, True), ('PARTIAL', True, False), ('ADAM', True, False))
FLOAT_EPIS = ('BIAS_ID', 'BIAS_RELU', 'RELU_MASK', 'PLAIN', 'PARTIAL')


def _kind(epi, want):
    return 'dyadic_small' if epi == 'BIAS_TANH' else (want if (want != 'float' or epi in FLOAT_EPIS) else 'dyadic')


def _partial_kw(epi, Kd, kchunk=None):
    if epi != 'PARTIAL':
        return {}
    kchunk = kchunk or Kd
    return dict(splits=ceil_div(Kd, kchunk), kchunk=kchunk)


def _auto_cases():
    out, seed = [], 0
    for epi, ta, tb in AUTO_COMBOS:
        for tm, tn in ((1, 1), (1, 2), (2, 1), (2, 2)):
            # extents at the tile's edges: one short of it, on it, one beyond it (more than one block), plus the smallest matrices
            em, en = 64 * tm, 64 * tn
            # AL: every contiguous extent a multiple of 4; the unaligned forms come from an odd extent, a padded leading dimension, a base
            # pointer off by one float or a head stride that is no multiple of 4 -- one quirk per case
            al_shapes = [(em + 4, en, 16, 1, {}), (em, en + 4, 32, 3, {}), (4, 8, 4, 1, dict(ldc_pad=3))]
            un_shapes = [(em + 1, en - 1, 17, 3, dict(ldc_pad=3)), (em - 1, en + 1, 33, 1, dict(lda_pad=1)), (1, 1, 1, 1, {}), (em, en, 16, 1, dict(a_off=1)),
                         (em + 4, en + 4, 16, 1, dict(ldw_pad=1)), (8, 8, 8, 3, dict(sa_pad=1)), (8, 12, 4, 3, dict(sw_pad=2)), (3, 5, 2, 1, dict(w_off=1)),
                         (em + 1, 7, 3, 1, {}), (5, en + 1, 15, 1, {}), (9, 9, 257, 1, {}), (8, 8, 256, 1, {})]
            for i, (M, N, Kd, heads, q) in enumerate(al_shapes + un_shapes):
                for kind in (('dyadic', 'float') if i < 5 else ('dyadic',)):
                    seed += 1
                    kw = dict(q); kw.update(_partial_kw(epi, Kd, 16 if (Kd > 16 and i % 2) else None))
                    if epi == 'PARTIAL':
                        kw.pop('ldc_pad', None)         # a partial is a dense M x N block followed by its N column sums: ldc = N
                    out.append(case('auto', epi, M, N, Kd, ta=ta, tb=tb, tm=tm, tn=tn, heads=heads, kind=_kind(epi, kind), seed=seed,
                                    decay=1e-6 if i % 2 else 0.0, **kw))
        # <1, 1> with the deep prefetch: Kd >= 256 (and few workgroups); 255 stays at PD 1 and is covered above the line by Kd = 255 here
        for i, (M, N, Kd, heads, q) in enumerate([(68, 64, 256, 1, {}), (64, 68, 260, 3, {}), (65, 63, 257, 1, {}), (63, 65, 256, 3, dict(lda_pad=1)),
                                                  (129, 129, 257, 1, dict(a_off=1)), (64, 64, 255, 1, {}), (64, 64, 252, 1, {})]):
            for kind in ('dyadic', 'float'):
                seed += 1
                kw = dict(q); kw.update(_partial_kw(epi, Kd, (0, 48, 16, 32, 48, 0, 0)[i] or None))
                out.append(case('auto', epi, M, N, Kd, ta=ta, tb=tb, tm=1, tn=1, heads=heads, kind=_kind(epi, kind), seed=seed, amp=8 if epi == 'DTANH' else 16,
                                decay=1e-6 if i % 2 else 0.0, **kw))
    # EPI_PARTIAL<F, F>: shipped on 64 x 64 tiles only (gemm_skinny_bias)
    for i, (M, N, Kd, kc, q) in enumerate([(65, 18, 256, 128, {}), (63, 12, 260, 48, {}), (129, 11, 257, 16, {}), (64, 64, 257, 32, dict(lda_pad=1)),
                                           (7, 5, 33, 16, {}), (8, 8, 32, 16, {}), (68, 8, 48, 48, {}), (1, 1, 1, 1, {}),
                                           (64, 16, 256, 128, {}), (68, 16, 272, 48, {})]):
        for kind in ('dyadic', 'float'):
            seed += 1
            out.append(case('auto', 'PARTIAL', M, N, Kd, tm=0, tn=0, heads=3 if i % 2 else 1, kind=kind, seed=seed, splits=ceil_div(Kd, kc), kchunk=kc, **q))
    # split-K corner forms on <T, F>: nk = 1, 2, 3 under PD 4, a shorter last split, a last split of one row, M no multiple of 4
    for M, N, Kd, kc in ((66, 64, 257, 16), (62, 30, 257, 32), (65, 65, 260, 48), (64, 64, 272, 48), (64, 64, 256, 32)):
        seed += 1
        out.append(case('auto', 'PARTIAL', M, N, Kd, ta=True, tm=1, tn=1, heads=1, seed=seed, splits=ceil_div(Kd, kc), kchunk=kc))
    # workgroup counts under the XCD remap: 1, 2, 3, 7, 9 and 15
    for M, N, heads in ((5, 5, 1), (5, 65, 1), (5, 5, 3), (5, 445, 1), (129, 129, 1), (5, 319, 3)):
        for epi, ta, tb in (('BIAS_ID', False, False), ('RELU_MASK', False, True), ('PARTIAL', True, False)):
            seed += 1
            out.append(case('auto', epi, M, N, 17, ta=ta, tb=tb, tm=1, tn=1, heads=heads, seed=seed, **_partial_kw(epi, 17)))
    return out


def _rule_cases():
    """gemm_auto's own rule (tm = tn = 0): for each tile one workgroup below the 2048 threshold and at it; matrices of one tile, many heads"""
    out = []
    for M, N in ((65, 65), (65, 8), (8, 65), (8, 8)):
        for heads in (2047, 2048):
            out.append(case('auto', 'BIAS_ID', M, N, 8, heads=heads, seed=900 + len(out)))
    return out


RULE_WANT = {(65, 65, 2047): (1, 2), (65, 65, 2048): (2, 2), (65, 8, 2047): (1, 1), (65, 8, 2048): (2, 1), (8, 65, 2047): (1, 1), (8, 65, 2048): (1, 2),
             (8, 8, 2047): (1, 1), (8, 8, 2048): (1, 1)}


def _skinny_cases():
    out, seed = [], 2000
    for act in (0, 1, 2):
        for defer in (False, True):
            for use_part in (False, True):
                # split (Kd >= 256 with a workspace): aligned and not, a last split shorter than the others; unsplit below the threshold
                for M, N, Kd, heads in ((65, 18, 257, 3), (64, 16, 512, 1), (129, 11, 300, 1), (63, 29, 255, 1), (5, 7, 16, 3)):
                    for kind in (('dyadic',) if act == 2 else ('dyadic', 'float')):
                        seed += 1
                        out.append(case('skinny', 'BIAS_ID', M, N, Kd, heads=heads, act=act, defer=defer, use_part=use_part, seed=seed,
                                        kind='dyadic_small' if act == 2 else kind))
    return out


def _fused_cases():
    out, seed = [], 3000
    for tile in (1, 2):
        for no in (10, 32, 33, 48, 49, 64):
            bn = 64 * tile
            shapes = [(bn + 4, bn, 16, 1, {}), (bn - 1, 2 * bn, 33, 3, {}), (1, bn, 1, 1, {}), (bn + 1, bn, 17, 1, dict(lda_pad=1)), (bn, 2 * bn, 32, 1, dict(a_off=1)),
                      (9, bn, 20, 3, dict(sa_pad=2))]
            if tile == 1:
                shapes += [(65, 128, 256, 1, {}), (63, 64, 257, 3, {})]
            for M, N, Kd, heads, q in shapes:
                for kind in ('dyadic', 'float'):
                    seed += 1
                    out.append(case('fused_out', 'BIAS_RELU', M, N, Kd, tm=tile, tn=tile, heads=heads, no=no, kind=kind, amp=4, seed=seed, **q))
    # the entry's own tile rule
    out.append(case('fused_out', 'BIAS_RELU', 70, 128, 16, heads=1, no=18, amp=4, seed=3999))
    return out


CASES = _auto_cases() + _rule_cases() + _skinny_cases() + _fused_cases()


def cases_by_form():
    d = {}
    for c in CASES:
        d.setdefault(form_of(c), []).append(c)
    return d


def form_id(f):
    if f.op == 'skinny':
        return 'skinny-' + f.variant
    return '%s-%s-%s%s-%d%d-%s-pd%d' % (f.op, f.variant, 'T' if f.ta else 'F', 'T' if f.tb else 'F', f.tm, f.tn, 'AL' if f.al else 'un', f.pd)
