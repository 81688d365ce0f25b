// Device-side helpers shared by the generic (VALU) kernels.  gfx950 only.
#pragma once
#include "metrpo_internal.h"
#include "env_model.h"    // the environments' cost, adjoint and termination

#define LOG_MIN_STD (-13.815510557964274f)   // log(1e-6): [rllab] GaussianMLPPolicy(min_std=1e-6)
#define KL_EPS 1e-8f                         // [rllab] DiagonalGaussian.kl_sym denominator constant
#define HALF_LOG_2PI 0.9189385332046727f     // 0.5 log(2 pi): DiagonalGaussian.log_likelihood_sym's constant term

// One element of tf.train.AdamOptimizer.apply_gradients with the bias correction folded into lr_t (launch_policy_adam, bptt.hip):
// k_policy_adam and the 'vpg' step in k_finalize's tail (policy_update.hip) share it, so the two forms agree bit for bit.  Contraction is
// spelt out: left to the compiler, which products fuse depends on the surrounding kernel.  The one fma (m1) is the form k_policy_adam
// always compiled to.
__device__ __forceinline__ void tf_adam_elem(float g, float* theta, float* am, float* av, int i, float lr_t, float b1, float b2, float eps) {
#pragma clang fp contract(off)
    const float m1 = fmaf(b1, am[i], (1.0f - b1) * g), v1 = b2 * av[i] + (1.0f - b2) * g * g;
    am[i] = m1; av[i] = v1;
    theta[i] = theta[i] - lr_t * m1 / (sqrtf(v1) + eps);
}

// PPO's head (ppo.py:112-117) for one sample with likelihood ratio lr and advantage adv: min(lr adv, clip(lr, lo, hi) adv) -> *surr, and the
// sample's weight d surr / d logli: lr adv on the unclipped branch (tf.minimum: a tie goes to its first argument), 0 on the clipped one
// (tf.clip_by_value passes no gradient outside the bounds).
__device__ __forceinline__ float ppo_gate(float lr, float adv, float lo, float hi, float* surr) {
    const float un = lr * adv, cl = fminf(fmaxf(lr, lo), hi) * adv;
    const bool pass = un <= cl;
    *surr = pass ? un : cl;
    return pass ? un : 0.0f;
}
// PPO's KL penalty (ppo.py:120-121) for one action dim of one sample: the dim's term of DiagonalGaussian.kl_sym(old, new) exactly as the OP_LOSSKL
// kernels write it (returned), and its derivatives with sigma = exp(ls), ls the clamped log_std and inv_std = exp(-ls):
//   d kl / d mean = (mean - old_mean) / sigma^2,   d kl / d log_std = 1 - (sigma_old^2 + (old_mean - mean)^2) / sigma^2      (os2 = sigma_old^2 = exp(2 ols))
// (The derivatives are those of the exact KL, as include/metrpo.h states them: kl_sym's 1e-8 in the denominator changes them by 1e-8 / (2 sigma^2) relative.)
__device__ __forceinline__ float ppo_kl_dim(float mu, float omu, float ls, float ols, float os2, float inv_std, float* dmu, float* dls) {
    const float s2 = expf(2.0f * ls), dm = omu - mu, iv = inv_std * inv_std;
    *dmu = -dm * iv;
    *dls = 1.0f - (os2 + dm * dm) * iv;
    return (dm * dm + os2 - s2) / (2.0f * s2 + KL_EPS) + ls - ols;
}
// The penalty's gate, tf.maximum(0., mean_kl - step_size) with MaximumGrad's tie rule (a tie sends the gradient to the constant): open iff strictly
// positive, decided on the float64 reduced mean KL.  Every wave of the launch reads the same cell.
__device__ __forceinline__ bool ppo_kl_open(const double* __restrict__ mean_kl, double delta) { return mean_kl[0] - delta > 0.0; }
#define ENTROPY_CONST 1.4189385332046727f    // 0.5 (1 + log(2 pi)): DiagonalGaussian.entropy_sym's constant per action dim

// tanh(x) = 1 - 2 / (1 + exp(2x)) in 5 VALU ops (v_mul, v_exp_f32, v_add, v_rcp_f32, v_fma): absolute error
// <= ~2e-7 everywhere (exact saturation to +-1); libm's tanhf costs ~40 ops and sat on every kernel's critical path.
__device__ __forceinline__ float tanh_fast(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);          // exp(2x) = 2^(2x log2 e)
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
}

__device__ __forceinline__ float act_apply(int act, float x) {
    if (act == METRPO_ACT_RELU) return fmaxf(x, 0.0f);
    if (act == METRPO_ACT_TANH) return tanh_fast(x);
    return x;
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG (production draws; parity tests supply the draws explicitly).
// counter = (env index lo, env index hi, t, purpose<<16 | chunk), key = seed.
// ---------------------------------------------------------------------------------------------
// RNG_STEP, chunk c of (env, t): .x,.y -> Box-Muller pair = policy noise of action dims 2c, 2c+1.  Chunk 0 also carries
//   .z -> step_rand model index of step t (high bits) and cur_model_idx of the reset following step t (low 16 bits),
//   .w -> pool row of that reset.   => the common case (na <= 2) costs ONE Philox block per env-step.
// RNG_SELNOISE, chunk c: 4 normals = model_mean_std noise of state dims 4c..4c+3.  RNG_RESET: initial reset (.x row, .y model).
// RNG_BPTT ('bptt-stochastic' gradient, bptt.hip): counter (env b, model i, t, RNG_BPTT<<16 | chunk c) -> normal4 = eps of action dims
//   4c .. 4c+3 of (model i, step t, env b)  => one Philox block per (i, t, b) for na <= 4.  Both sweeps of every family recompute it.
enum { RNG_STEP = 1, RNG_SELNOISE = 2, RNG_RESET = 3, RNG_BPTT = 4 };

__device__ __forceinline__ uint4 philox4x32(uint4 ctr, uint2 key) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
        uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += W0;
        key.y += W1;
    }
    return ctr;
}

__device__ __forceinline__ uint4 rng_draw(uint64_t seed, uint64_t env, uint32_t t, uint32_t purpose, uint32_t chunk) {
    return philox4x32(make_uint4((uint32_t)env, (uint32_t)(env >> 32), t, (purpose << 16) | chunk),
                      make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// 4 standard normals from one Philox block (Box-Muller)
__device__ __forceinline__ void normal4(uint4 r, float out[4]) {
    const float S = 2.3283064365386963e-10f;   // 2^-32
    float u0 = ((float)r.x + 0.5f) * S, u1 = ((float)r.y + 0.5f) * S;
    float u2 = ((float)r.z + 0.5f) * S, u3 = ((float)r.w + 0.5f) * S;
    float r0 = sqrtf(-2.0f * __logf(u0)), r1 = sqrtf(-2.0f * __logf(u2));
    float s0, c0, s1, c1;
    __sincosf(6.283185307179586f * u1, &s0, &c0);
    __sincosf(6.283185307179586f * u3, &s1, &c1);
    out[0] = r0 * c0; out[1] = r0 * s0; out[2] = r1 * c1; out[3] = r1 * s1;
}

__device__ __forceinline__ void normal2(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float S = 2.3283064365386963e-10f;
    const float u0 = ((float)a + 0.5f) * S, u1 = ((float)b + 0.5f) * S;
    const float rad = sqrtf(-2.0f * __logf(u0));
    float sn, cs;
    __sincosf(6.283185307179586f * u1, &sn, &cs);
    n0 = rad * cs; n1 = rad * sn;
}

// eps of action dims 4 chunk .. 4 chunk + 3 of (model i, step t, env b < B); dims >= na read as 0 in parity mode
__device__ __forceinline__ void bptt_eps4(const BpttNoise& nz, int i, int t, int B, int b, int na, int chunk, float e[4]) {
    if (nz.eps != nullptr) {
        const float* p = nz.eps + (((size_t)i * nz.T + t) * B + b) * na;
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = (4 * chunk + j < na) ? p[4 * chunk + j] : 0.0f;
    } else {
        normal4(rng_draw(nz.seed, ((uint64_t)(uint32_t)i << 32) | (uint32_t)b, (uint32_t)t, RNG_BPTT, (uint32_t)chunk), e);
    }
}

__device__ __forceinline__ int rng_index(uint32_t r, int n) { return (int)(((uint64_t)r * (uint64_t)n) >> 32); }
__device__ __forceinline__ int rng_index16(uint32_t r, int n) { return (int)(((r & 0xFFFFu) * (uint32_t)n) >> 16); }   // n <= 65535

// ---------------------------------------------------------------------------------------------
// "Column" layout: one thread = one env/sample; activation u of thread tid lives at buf[u*LD + tid]
// (lanes hit consecutive LDS banks).  Weights are wave-uniform reads of a const __restrict__ kernel
// argument, which hipcc turns into scalar (s_load) traffic: no LDS bandwidth for weights.
// ---------------------------------------------------------------------------------------------
#define DENSE_JB 8
__device__ __forceinline__ void dense_col(const float* __restrict__ W, const float* __restrict__ b, int n_in,
                                          int n_out, int act, const float* in, float* out, int LD, int tid) {
    for (int j0 = 0; j0 < n_out; j0 += DENSE_JB) {
        float acc[DENSE_JB];
        const int nj = min(DENSE_JB, n_out - j0);
        if (nj == DENSE_JB) {
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj) acc[jj] = b[j0 + jj];
            for (int i = 0; i < n_in; ++i) {
                const float a = in[i * LD + tid];
                const float* __restrict__ w = W + (size_t)i * n_out + j0;
#pragma unroll
                for (int jj = 0; jj < DENSE_JB; ++jj) acc[jj] = fmaf(a, w[jj], acc[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj) out[(j0 + jj) * LD + tid] = act_apply(act, acc[jj]);
        } else {
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj) acc[jj] = (jj < nj) ? b[j0 + jj] : 0.0f;
            for (int i = 0; i < n_in; ++i) {
                const float a = in[i * LD + tid];
                const float* __restrict__ w = W + (size_t)i * n_out + j0;
#pragma unroll
                for (int jj = 0; jj < DENSE_JB; ++jj)
                    if (jj < nj) acc[jj] = fmaf(a, w[jj], acc[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj)
                if (jj < nj) out[(j0 + jj) * LD + tid] = act_apply(act, acc[jj]);
        }
    }
}

// dense_col restricted to the output columns [j_lo, j_hi) -- lets G thread groups of a block share one layer of one env tile
__device__ __forceinline__ void dense_col_range(const float* __restrict__ W, const float* __restrict__ b, int n_in, int n_out, int j_lo,
                                                int j_hi, int act, const float* in, float* out, int LD, int tid) {
    for (int j0 = j_lo; j0 < j_hi; j0 += DENSE_JB) {
        float acc[DENSE_JB];
        const int nj = min(DENSE_JB, j_hi - j0);
#pragma unroll
        for (int jj = 0; jj < DENSE_JB; ++jj) acc[jj] = (jj < nj) ? b[j0 + jj] : 0.0f;
        for (int i = 0; i < n_in; ++i) {
            const float a = in[i * LD + tid];
            const float* __restrict__ w = W + (size_t)i * n_out + j0;
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj)
                if (jj < nj) acc[jj] = fmaf(a, w[jj], acc[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < DENSE_JB; ++jj)
            if (jj < nj) out[(j0 + jj) * LD + tid] = act_apply(act, acc[jj]);
    }
}

// mlp_col with the outputs of every layer split over the G thread groups of the block (group g = threadIdx.x / LD); every thread of the
// block must call it (block barriers between layers).  Returns the buffer holding the outputs.
__device__ __forceinline__ float* mlp_col_groups(const NetDesc& net, const float* __restrict__ params, const float* in, float* bufA, float* bufB,
                                                 int LD, int lane, int g, int G) {
    const float* cur = in;
    float* dst = bufA;
    for (int l = 0; l < net.n_layers; ++l) {
        const int n_out = net.dims[l + 1];
        const int per = ((n_out + G * DENSE_JB - 1) / (G * DENSE_JB)) * DENSE_JB;       // columns per group, a multiple of the register block
        const int j_lo = min(n_out, g * per), j_hi = min(n_out, j_lo + per);
        dense_col_range(params + net.w_off[l], params + net.b_off[l], net.dims[l], n_out, j_lo, j_hi, net.act[l], cur, dst, LD, lane);
        __syncthreads();
        cur = dst;
        dst = (dst == bufA) ? bufB : bufA;
    }
    return const_cast<float*>(cur);
}

// Full MLP in column layout.  `in` is read-only; hidden activations ping-pong between bufA/bufB;
// returns the pointer (bufA or bufB) holding the n_out outputs.
__device__ __forceinline__ float* mlp_col(const NetDesc& net, const float* __restrict__ params, const float* in,
                                          float* bufA, float* bufB, int LD, int tid) {
    const float* cur = in;
    float* dst = bufA;
    for (int l = 0; l < net.n_layers; ++l) {
        dense_col(params + net.w_off[l], params + net.b_off[l], net.dims[l], net.dims[l + 1], net.act[l], cur, dst,
                  LD, tid);
        cur = dst;
        dst = (dst == bufA) ? bufB : bufA;
    }
    return const_cast<float*>(cur);
}

// dout[j] = sum_i W[j][i] * din[i]   (W row-major n_in x n_out: the VJP of  out = in . W); net_vjp's step (below) and the
// Jacobian rows of svg.hip
__device__ __forceinline__ void dense_col_T(const float* __restrict__ W, int n_in, int n_out, const float* din, float* dout, int LD, int tid) {
    for (int j = 0; j < n_in; ++j) {
        const float* __restrict__ w = W + (size_t)j * n_out;
        float s0 = 0.0f, s1 = 0.0f;
        int i = 0;
        for (; i + 1 < n_out; i += 2) { s0 = fmaf(w[i], din[i * LD + tid], s0); s1 = fmaf(w[i + 1], din[(i + 1) * LD + tid], s1); }
        if (i < n_out) s0 = fmaf(w[i], din[i * LD + tid], s0);
        dout[j * LD + tid] = s0 + s1;
    }
}

// A net's hidden layers and its vector-Jacobian product in column layout: the reverse sweeps of bptt.hip, score_actions_grad.hip and
// score_policy_actions_grad.hip, and the recompute of svg.hip's k_svg_jac.
__host__ __device__ inline int net_hidden_rows(const NetDesc& n) {
    int rows = 0;
    for (int l = 1; l < n.n_layers; ++l) rows += n.dims[l];
    return rows;
}
// the hidden layers of a net into `store` (all outputs kept; the output layer is not formed)
__device__ __forceinline__ void net_hidden(const NetDesc& n, const float* __restrict__ params, const float* in, float* store, int LD, int tid) {
    const float* cur = in; float* dst = store;
    for (int l = 0; l < n.n_layers - 1; ++l) {
        dense_col(params + n.w_off[l], params + n.b_off[l], n.dims[l], n.dims[l + 1], n.act[l], cur, dst, LD, tid);
        cur = dst; dst += n.dims[l + 1] * LD;
    }
}
// dout = W . (din * act'(h)) chains of one net, back from `da` (the adjoint of the net's output, n_out rows) to the adjoint of its input; `store` holds the
// hidden layers' outputs in layer order.  Returns the buffer (da or db) that holds the result.
__device__ __forceinline__ float* net_vjp(const NetDesc& n, const float* __restrict__ params, const float* store, float* da, float* db, int LD, int tid) {
    int off = 0;
    for (int l = 1; l < n.n_layers - 1; ++l) off += n.dims[l];                // rows of the LAST hidden layer in the store
    for (int l = n.n_layers - 1; l >= 0; --l) {
        dense_col_T(params + n.w_off[l], n.dims[l], n.dims[l + 1], da, db, LD, tid);
        if (l > 0) {
            const float* h = store + off * LD;                                 // output of layer l-1 (post-activation)
            for (int j = 0; j < n.dims[l]; ++j) {
                const float hv = h[j * LD + tid];
                const float dact = (n.act[l - 1] == METRPO_ACT_RELU) ? (hv > 0.0f ? 1.0f : 0.0f)
                                  : (n.act[l - 1] == METRPO_ACT_TANH) ? (1.0f - hv * hv) : 1.0f;
                db[j * LD + tid] *= dact;
            }
            if (l > 1) off -= n.dims[l - 1];
        }
        float* tmp = da; da = db; db = tmp;
    }
    return da;
}

// block-wide sum of a double over a 1-D block (<= 1024 threads); result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh /* >= 16 doubles */) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) r += sh[i];
    }
    return r;
}
