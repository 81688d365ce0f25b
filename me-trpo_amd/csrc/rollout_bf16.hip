// Dynamics forward of metrpo_rollout with bf16 OPERANDS (metrpo_set_dyn_precision(ctx, METRPO_DYN_BF16), include/metrpo.h): every layer of every head is
//     out[b][j] = act( b[j] + sum_i bf16(in[b][i]) * bf16(W[i][j]) )
// with bf16(.) = round-to-nearest-even from f32, exact products, f32 accumulation in the matrix instruction's order, bias and activation in f32.  Only the
// per-layer GEMMs of the plain tile-GEMM branch of rollout_gemm_chunk come here; pre-step, closing of a step, selection, reward, done, reset and every draw
// are rollout_gemm.hip's kernels, unchanged (reference: training.py:218-269, env_helpers.py:597-635).
//   k_bf16_wimage   d_dyn (f32, [Kd][N] per layer) -> [head][layer][N][Kp] bf16, k contiguous and zero-padded to a multiple of 64: built in front of every
//                   bf16 rollout call (no cache: nothing to keep coherent with metrpo_set_dynamics*, metrpo_dyn_train_step, checkpoint loads)
//   k_gemm_bf16     128 x BN tile (BN = 128 / 64), 4 waves, v_mfma_f32_32x32x16_bf16; both operands 16 bytes of consecutive k per lane out of LDS
//                   rows of 64 k (+ 8 pad: conflict-free ds_read_b128); the next k step's global loads fly under the current one's matrix instructions.
//                   Layer 0 reads the f32 input rows X and rounds on the way into LDS; hidden layers store their activations ROUNDED ONCE as bf16
//                   ([K][B][ld], ld = width rounded up to 64, pad columns written as zeros); the output layer stores f32 [K][B][ns] for k_big_post.
// Every edge is predicated: rows >= M and columns >= N load zeros and store nothing (pad columns of a bf16 output: zeros).
// At the end of the file: two diagnostics hooks for the tests (not in include/metrpo.h), metrpo_debug_gemm_bf16 (one launch of either kernel on
// caller-owned memory: tests/test_gpu_bf16_gemm.py) and metrpo_debug_last_bf16_layers (the column tile each layer of the last step was launched on).
#include <algorithm>
#include "metrpo_internal.h"
#include "device_common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// f32 -> bf16, round to nearest, ties to even (NaN stays a quiet NaN)
__device__ __forceinline__ uint32_t bf16_rne(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t bf16_pack2(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }

Bf16Img bf16_img_layout(const ProblemDesc& pd) {
    Bf16Img im = {};
    size_t off = 0;
    for (int l = 0; l < pd.dyn.n_layers; ++l) {
        const int Kd = (l == 0) ? pd.nin : pd.dyn.dims[l];
        im.Kp[l] = (Kd + 63) & ~63;
        im.off[l] = off;
        off += (size_t)pd.dyn.dims[l + 1] * im.Kp[l];
    }
    im.per_head = off;
    return im;
}

// one layer of every head: W [Kd][N] f32 -> img [N][Kp] bf16 (32 x 32 tiles through LDS: both sides coalesced)
__global__ void __launch_bounds__(256) k_bf16_wimage(const float* __restrict__ W, long long sW, int Kd, int N, int Kp, uint16_t* __restrict__ img, long long sImg) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const float* Wh = W + (size_t)blockIdx.z * sW;
    uint16_t* ih = img + (size_t)blockIdx.z * sImg;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + ty + 8 * j, n = n0 + tx;
        tile[ty + 8 * j][tx] = (k < Kd && n < N) ? Wh[(size_t)k * N + n] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + ty + 8 * j, k = k0 + tx;
        if (n < N && k < Kp) ih[(size_t)n * Kp + k] = (uint16_t)bf16_rne(tile[tx][ty + 8 * j]);
    }
}

static void bf16_wimage_launch(const float* W, long long sW, int Kd, int N, int Kp, uint16_t* img, long long sImg, int heads, hipStream_t st) {
    hipLaunchKernelGGL(k_bf16_wimage, dim3(Kp / 32, (N + 31) / 32, heads), dim3(256), 0, st, W, sW, Kd, N, Kp, img, sImg);
}

int launch_bf16_dyn_image(metrpo_ctx* c, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const Bf16Img im = bf16_img_layout(pd);
    { const int rc = ws_grow(c, c->d_dyn_bf16, sizeof(uint16_t) * im.per_head * pd.K); if (rc) return rc; }
    for (int l = 0; l < pd.dyn.n_layers; ++l) {
        const int Kd = (l == 0) ? pd.nin : pd.dyn.dims[l], N = pd.dyn.dims[l + 1];
        bf16_wimage_launch(c->d_dyn.p + pd.dyn.w_off[l], (long long)pd.dyn.n_params, Kd, N, im.Kp[l], c->d_dyn_bf16.p + im.off[l], (long long)im.per_head, pd.K, st);
    }
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

// C[head] = act(A[head] . W[head]^T + bias[head]).  A: [M][lda] rows, AT = float (k < Kd valid, Kd and lda multiples of 4) or uint16_t (bf16; lda >= Kp, the
// columns up to Kp hold zeros beyond the layer's width); W: the image [N][Kp]; C: [M][ldc], CT = uint16_t (bf16, columns N .. ldc - 1 written as zeros) or float.
// grid = (column tiles, row tiles, heads)
template <typename AT, typename CT, int BN>
__global__ void __launch_bounds__(256) k_gemm_bf16(const AT* __restrict__ A, long long sA, int lda, const uint16_t* __restrict__ W, long long sW, int Kp,
                                                   const float* __restrict__ bias, long long sB, CT* __restrict__ C, long long sC, int ldc, int M, int N, int Kd, int act) {
    constexpr int BM = 128, BK = 64, LD = BK + 8;                 // LDS rows of 144 bytes
    constexpr int WN = BN / 64, WM = 4 / WN, TM = BM / WM / 32;     // waves over columns / rows; 32-row tiles per wave (2 column tiles each)
    constexpr bool AF32 = sizeof(AT) == 4;
    constexpr int NLA = AF32 ? 8 : 4, NLB = BN * 8 / 256;
    __shared__ __attribute__((aligned(16))) uint16_t As[BM * LD];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[BN * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN, head = blockIdx.z;
    const AT* Ah = A + (size_t)head * sA;
    const uint16_t* Wh = W + (size_t)head * sW;
    uint4 ra[NLA], rb[NLB];
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int ch = tid + 256 * i;
            ra[i] = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (AF32) {
                const int r = ch >> 4, k = kt + 4 * (ch & 15);
                if (row0 + r < M && k < Kd) ra[i] = *(const uint4*)(Ah + (size_t)(row0 + r) * lda + k);
            } else {
                const int r = ch >> 3, k = kt + 8 * (ch & 7);
                if (row0 + r < M) ra[i] = *(const uint4*)(Ah + (size_t)(row0 + r) * lda + k);
            }
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            const int ch = tid + 256 * i, r = ch >> 3, k = kt + 8 * (ch & 7);
            rb[i] = make_uint4(0u, 0u, 0u, 0u);
            if (col0 + r < N) rb[i] = *(const uint4*)(Wh + (size_t)(col0 + r) * Kp + k);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int ch = tid + 256 * i;
            if constexpr (AF32) {
                const int r = ch >> 4, kc = 4 * (ch & 15);
                uint2 p;
                p.x = bf16_pack2(__uint_as_float(ra[i].x), __uint_as_float(ra[i].y));
                p.y = bf16_pack2(__uint_as_float(ra[i].z), __uint_as_float(ra[i].w));
                *(uint2*)&As[r * LD + kc] = p;
            } else {
                const int r = ch >> 3, kc = 8 * (ch & 7);
                *(uint4*)&As[r * LD + kc] = ra[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            const int ch = tid + 256 * i, r = ch >> 3, kc = 8 * (ch & 7);
            *(uint4*)&Bs[r * LD + kc] = rb[i];
        }
    };
    f32x16_t acc[TM][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int fr = lane & 31, fk = 8 * (lane >> 5);                // operand maps: lane holds row / column fr, k = 8 (lane >> 5) + 0 .. 7 of the 16-deep step
    load(0);
    for (int kt = 0; kt < Kp; kt += BK) {
        stage();
        __syncthreads();
        if (kt + BK < Kp) load(kt + BK);
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            bf16x8_t af[TM], bfr[2];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = __builtin_bit_cast(bf16x8_t, *(const uint4*)&As[(wm * 32 * TM + 32 * i + fr) * LD + 16 * s + fk]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = __builtin_bit_cast(bf16x8_t, *(const uint4*)&Bs[(wn * 64 + 32 * j + fr) * LD + 16 * s + fk]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: register e of a 32 x 32 tile = row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
    CT* Ch = C + (size_t)head * sC;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + wn * 64 + 32 * j + fr;
        if (col >= ldc) continue;
        const float bv = (col < N) ? bias[(size_t)head * sB + col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = row0 + wm * 32 * TM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                if (row >= M) continue;
                const float v = (col < N) ? act_apply(act, bv + acc[i][j][e]) : 0.0f;
                if constexpr (sizeof(CT) == 4) Ch[(size_t)row * ldc + col] = v;
                else Ch[(size_t)row * ldc + col] = (uint16_t)bf16_rne(v);
            }
    }
}

// The launch gemm_bf16_pick makes, as a pure host function: 64-column tiles for narrow layers (the output layer: ns <= 64) and while 128-column tiles would
// leave CUs without one.  force_bn = 64 / 128 (metrpo_debug_gemm_bf16 only) takes the tile as given.
Bf16GemmForm gemm_bf16_form(int n_cu, int M, int N, int heads, int force_bn) {
    const int rt = (M + 127) / 128;
    int bn = force_bn;
    if (bn == 0) bn = (N <= 64 || (long long)heads * rt * ((N + 127) / 128) < n_cu) ? 64 : 128;
    return Bf16GemmForm{bn, (N + bn - 1) / bn, rt, heads};
}

template <typename AT, typename CT>
static Bf16GemmForm gemm_bf16_pick(int n_cu, const AT* A, long long sA, int lda, const uint16_t* W, long long sW, int Kp, const float* bias, long long sB, CT* C, long long sC,
                                   int ldc, int M, int N, int Kd, int heads, int act, hipStream_t st, int force_bn = 0) {
    const Bf16GemmForm f = gemm_bf16_form(n_cu, M, N, heads, force_bn);
    if (f.bn == 64) hipLaunchKernelGGL((k_gemm_bf16<AT, CT, 64>), dim3(f.gx, f.gy, f.gz), dim3(256), 0, st, A, sA, lda, W, sW, Kp, bias, sB, C, sC, ldc, M, N, Kd, act);
    else hipLaunchKernelGGL((k_gemm_bf16<AT, CT, 128>), dim3(f.gx, f.gy, f.gz), dim3(256), 0, st, A, sA, lda, W, sW, Kp, bias, sB, C, sC, ldc, M, N, Kd, act);
    return f;
}

// floats of ONE hidden-activation buffer of the step loop's workspace: bf16 [K][B][widest hidden layer rounded up to 64]
size_t bf16_hidden_floats(const ProblemDesc& pd, int B) {
    int maxh = 0;
    for (int l = 1; l < pd.dyn.n_layers; ++l) maxh = std::max(maxh, pd.dyn.dims[l]);
    return ((size_t)pd.K * B * ((maxh + 63) & ~63) + 1) / 2 + 4;
}

// The dynamics layers of one step: X [B][ldx] f32 (pad columns zero) -> OUT [K][B][ns] f32, hidden activations through the two bf16 buffers HA / HB.
// Layer 0 reads f32 and stores bf16, the layers between read and store bf16, the output layer reads bf16 and stores f32: at least two layers.
int launch_bf16_layers(metrpo_ctx* c, const float* X, int ldx, void* HA, void* HB, float* OUT, int B, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const int L = pd.dyn.n_layers, K = pd.K;
    if (L < 2) return set_err(c, METRPO_EUNSUPPORTED, "bf16 dynamics forward: at least one hidden layer");
    const Bf16Img im = bf16_img_layout(pd);
    uint16_t* hb[2] = {(uint16_t*)HA, (uint16_t*)HB};
    const uint16_t* hin = nullptr; long long sA = 0; int lda = 0;
    for (int l = 0; l < L; ++l) {
        const int N = pd.dyn.dims[l + 1], ldc = (l == L - 1) ? N : ((N + 63) & ~63);
        const long long sC = (long long)B * ldc;
        const uint16_t* W = c->d_dyn_bf16.p + im.off[l];
        const float* bias = c->d_dyn.p + pd.dyn.b_off[l];
        const long long sW = (long long)im.per_head, sB = pd.dyn.n_params;
        Bf16GemmForm f;
        if (l == 0) f = gemm_bf16_pick(c->n_sm, X, 0LL, ldx, W, sW, im.Kp[l], bias, sB, hb[0], sC, ldc, B, N, ldx, K, pd.dyn.act[l], st);
        else if (l == L - 1) f = gemm_bf16_pick(c->n_sm, hin, sA, lda, W, sW, im.Kp[l], bias, sB, OUT, sC, ldc, B, N, im.Kp[l], K, pd.dyn.act[l], st);
        else f = gemm_bf16_pick(c->n_sm, hin, sA, lda, W, sW, im.Kp[l], bias, sB, hb[l & 1], sC, ldc, B, N, im.Kp[l], K, pd.dyn.act[l], st);
        hin = hb[l & 1]; sA = sC; lda = ldc;
        c->bf16_last_bn[l] = f.bn;
    }
    c->bf16_last_layers = L;
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

// Diagnostics hook (not part of include/metrpo.h; tests/test_gpu_dyn_bf16.py): the column tile of every layer GEMM of the last bf16 rollout step this context enqueued, as
// launch_bf16_layers wrote it down on the host (no device work, no synchronisation).  out[1 + MAXL] = number of layers (0: no bf16 rollout yet), then bn per layer.
extern "C" int32_t metrpo_debug_last_bf16_layers(const metrpo_ctx* c, int32_t* out) {
    if (!c || !out) return METRPO_ENULL;
    out[0] = c->bf16_last_layers;
    for (int l = 0; l < MAXL; ++l) out[1 + l] = (l < c->bf16_last_layers) ? c->bf16_last_bn[l] : 0;
    return METRPO_OK;
}

// Diagnostics hook (not part of include/metrpo.h; tests/test_gpu_bf16_gemm.py, Engine.debug_gemm_bf16): ONE launch of k_bf16_wimage or of gemm_bf16_pick on caller-owned
// device memory, in exactly the argument shapes launch_bf16_dyn_image / launch_bf16_layers pass.  It allocates nothing, measures nothing and reads and writes no context
// state besides the CU count the rule takes (a rejected call records its reason in the context's error string, like every entry point).  The caller sizes every buffer
// for the extents and strides it passes.
struct metrpo_debug_gemm_bf16_args {       // mirrored by _lib.DebugGemmBf16Args
    int32_t op;                            // 0 image: W f32 [heads][Kd][N] (head stride sW floats) -> C = img bf16 [heads][N][Kp] (head stride sC elements); 1 gemm
    int32_t a_bf16, c_bf16;                // gemm: element types of A and C: (0, 1) layer 0, (1, 1) a layer between, (1, 0) the output layer
    int32_t bn;                            // gemm: 0 the rule, 64 or 128 the tile as given (128 only where the rule can choose it: N > 64)
    int32_t M, N, Kd, Kp, heads, lda, ldc, act;
    int64_t sA, sW, sB, sC;                // head strides in elements of the operand's type
    const void* A; const void* W; const float* bias; void* C;
    int32_t o_bn, o_gx, o_gy, o_gz, o_n_cu;      // on return: the launched form (image: o_bn = 0)
};

extern "C" int32_t metrpo_debug_gemm_bf16(metrpo_ctx* c, metrpo_debug_gemm_bf16_args* a, void* stream) {
    if (!c || !a) return METRPO_ENULL;
    hipStream_t st = (hipStream_t)stream;
    auto bad = [&](const char* why) { return set_err(c, METRPO_EINVAL, std::string("debug_gemm_bf16: ") + why); };
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    if (!a->W || !a->C) return bad("W and C must be given");
    if (a->N < 1 || a->Kd < 1 || a->heads < 1 || a->heads > 65535) return bad("N, Kd and heads must be positive (heads below 65536)");
    if (a->Kp < 64 || a->Kp % 64 != 0) return bad("Kp must be a positive multiple of 64");
    a->o_n_cu = c->n_sm;
    if (a->op == 0) {
        if (a->Kp != ((a->Kd + 63) & ~63)) return bad("image: Kp must be Kd rounded up to 64");
        if (a->sW < 0 || a->sC < 0) return bad("image: head strides must not be negative");
        bf16_wimage_launch((const float*)a->W, a->sW, a->Kd, a->N, a->Kp, (uint16_t*)a->C, a->sC, a->heads, st);
        a->o_bn = 0; a->o_gx = a->Kp / 32; a->o_gy = (a->N + 31) / 32; a->o_gz = a->heads;
    } else if (a->op == 1) {
        if (!a->A || !a->bias) return bad("gemm: A and bias must be given");
        if (a->M < 1 || (a->M + 127) / 128 > 65535) return bad("gemm: M must be positive, at most 65535 row tiles");
        if (a->act < METRPO_ACT_IDENTITY || a->act > METRPO_ACT_TANH) return bad("gemm: act must be 0, 1 or 2");
        if (a->bn != 0 && a->bn != 64 && a->bn != 128) return bad("gemm: bn must be 0, 64 or 128");
        if (a->bn == 128 && a->N <= 64) return bad("gemm: the 128-column tile is launched at N > 64 only");
        if (!((a->a_bf16 == 0 && a->c_bf16 == 1) || (a->a_bf16 == 1 && (a->c_bf16 == 0 || a->c_bf16 == 1)))) return bad("gemm: (A, C) must be (f32, bf16), (bf16, bf16) or (bf16, f32)");
        if (!al16(a->A) || !al16(a->W)) return bad("gemm: A and W must be 16-byte aligned");
        if (a->sW < 0 || a->sW % 8 != 0) return bad("gemm: sW must be a non-negative multiple of 8");
        if (a->sA < 0 || a->sB < 0 || a->sC < 0) return bad("gemm: head strides must not be negative");
        if (a->a_bf16) {
            if (a->Kd != a->Kp) return bad("gemm: bf16 A is read up to Kp: Kd must equal Kp");
            if (a->lda < a->Kp || a->lda % 8 != 0 || a->sA % 8 != 0) return bad("gemm: bf16 A needs lda >= Kp, lda and sA multiples of 8");
        } else {
            if (a->Kd != a->lda || a->lda % 4 != 0 || a->sA % 4 != 0) return bad("gemm: f32 A needs Kd = lda, lda and sA multiples of 4");
            if (a->Kp != ((a->Kd + 63) & ~63)) return bad("gemm: f32 A needs Kp = Kd rounded up to 64");
        }
        if (a->ldc != (a->c_bf16 ? ((a->N + 63) & ~63) : a->N)) return bad("gemm: ldc must be N rounded up to 64 (bf16 C) or N (f32 C)");
        Bf16GemmForm f;
#define GB_ARGS_ a->sA, a->lda, (const uint16_t*)a->W, a->sW, a->Kp, a->bias, a->sB
#define GB_TAIL_ a->sC, a->ldc, a->M, a->N, a->Kd, a->heads, a->act, st, a->bn
        if (!a->a_bf16) f = gemm_bf16_pick(c->n_sm, (const float*)a->A, GB_ARGS_, (uint16_t*)a->C, GB_TAIL_);
        else if (a->c_bf16) f = gemm_bf16_pick(c->n_sm, (const uint16_t*)a->A, GB_ARGS_, (uint16_t*)a->C, GB_TAIL_);
        else f = gemm_bf16_pick(c->n_sm, (const uint16_t*)a->A, GB_ARGS_, (float*)a->C, GB_TAIL_);
#undef GB_ARGS_
#undef GB_TAIL_
        a->o_bn = f.bn; a->o_gx = f.gx; a->o_gy = f.gy; a->o_gz = f.gz;
    } else {
        return bad("unknown op");
    }
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}
