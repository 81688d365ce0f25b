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

int launch_bf16_dyn_image(metrpo_ctx* c, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const Bf16Img im = bf16_img_layout(pd);
    { const int rc = ws_grow(c, c->d_dyn_bf16, sizeof(uint16_t) * im.per_head * pd.K); if (rc) return rc; }
    for (int l = 0; l < pd.dyn.n_layers; ++l) {
        const int Kd = (l == 0) ? pd.nin : pd.dyn.dims[l], N = pd.dyn.dims[l + 1];
        hipLaunchKernelGGL(k_bf16_wimage, dim3(im.Kp[l] / 32, (N + 31) / 32, pd.K), dim3(256), 0, st, c->d_dyn.p + pd.dyn.w_off[l], (long long)pd.dyn.n_params, Kd, N,
                           im.Kp[l], c->d_dyn_bf16.p + im.off[l], (long long)im.per_head);
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

template <typename AT, typename CT>
static void gemm_bf16_pick(int n_cu, const AT* A, long long sA, int lda, const uint16_t* W, long long sW, int Kp, const float* bias, long long sB, CT* C, long long sC, int ldc,
                           int M, int N, int Kd, int heads, int act, hipStream_t st) {
    const int rt = (M + 127) / 128;
    // 64-column tiles for narrow layers (the output layer: ns <= 64) and while 128-column tiles would leave CUs without one
    if (N <= 64 || (long long)heads * rt * ((N + 127) / 128) < n_cu)
        hipLaunchKernelGGL((k_gemm_bf16<AT, CT, 64>), dim3((N + 63) / 64, rt, heads), dim3(256), 0, st, A, sA, lda, W, sW, Kp, bias, sB, C, sC, ldc, M, N, Kd, act);
    else
        hipLaunchKernelGGL((k_gemm_bf16<AT, CT, 128>), dim3((N + 127) / 128, rt, heads), dim3(256), 0, st, A, sA, lda, W, sW, Kp, bias, sB, C, sC, ldc, M, N, Kd, act);
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
        if (l == 0) gemm_bf16_pick(c->n_sm, X, 0LL, ldx, W, sW, im.Kp[l], bias, sB, hb[0], sC, ldc, B, N, ldx, K, pd.dyn.act[l], st);
        else if (l == L - 1) gemm_bf16_pick(c->n_sm, hin, sA, lda, W, sW, im.Kp[l], bias, sB, OUT, sC, ldc, B, N, im.Kp[l], K, pd.dyn.act[l], st);
        else gemm_bf16_pick(c->n_sm, hin, sA, lda, W, sW, im.Kp[l], bias, sB, hb[l & 1], sC, ldc, B, N, im.Kp[l], K, pd.dyn.act[l], st);
        hin = hb[l & 1]; sA = sC; lda = ldc;
    }
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}
