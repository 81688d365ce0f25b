// BPTT policy gradient through the unrolled imagined rollout ("next" row):
//   d/d theta  mean_i  sum_t gamma^t mean_b cost_tf(x_t, u_t, x_{t+1})     with  u_t = clip(policy(x_t)),  x_{t+1} = model_i(x_t, u_t)
//   build_policy_graph (model_based_rl.py:106-151), training_policy_cost = reduce_mean over models (:365), Adam with per-variable
//   tf.clip_by_norm (get_policy_optimizer :186-206, utils.py:262-276), 'bptt' branch of optimize_policy (:1181-1187).
//
// Three device stages, all stream-ordered, no host sync:
//   k_bptt_forward   thread = (env b, model i): the deterministic rollout of build_policy_graph; keeps every state x_t, the per-step
//                    weight gamma^t (1 - dones_t) / (B K) and the per-model costs (= k_validation + stores).
//   k_bptt_backward  same mapping, t = T-1 .. 0: recomputes the two MLPs of the step from x_t, pushes the state adjoint through
//                    cost -> dynamics head i (incl. the residual and the normalisers) -> clip -> policy input, and writes the adjoint
//                    of the policy MEAN for every (i, t, b).
//   policy VJP       sum over all (i, t, b) samples of J_policy(x_t)^T adjoint_mean: the gradient kernels of the TRPO update with
//                    the mean-adjoint supplied (PolK.gm) instead of derived from the surrogate loss -- MFMA path included.
// Generic in the layer widths (activations in LDS columns, one thread per trajectory).  The reverse sweep's pieces -- a net's hidden layers
// (net_hidden) and its vector-Jacobian product (net_vjp), device_common.h's, and the cost adjoint (env_cost_adjoint, env_model.h) -- are shared with the generic
// gradient kernels of score_actions_grad.hip and score_policy_actions_grad.hip.
#include <cmath>
#include "device_common.h"

struct BpttBufs { float *S, *XN, *U, *X, *PH, *DH, *GA, *GB, *LAM; };

__host__ __device__ inline int net_store_rows(const NetDesc& n, bool with_output) {
    int r = 0;
    for (int l = 1; l <= n.n_layers; ++l) if (l < n.n_layers || with_output) r += n.dims[l];
    return r;
}
__host__ __device__ inline size_t bptt_floats(const ProblemDesc& pd) {
    const int mw = max(max(pd.dyn.max_width, pd.pol.max_width), pd.ns + pd.na);
    return (size_t)(3 * pd.ns + pd.na + (pd.ns + pd.na) + net_store_rows(pd.pol, true) + net_store_rows(pd.dyn, false) + 2 * mw);
}
__device__ __forceinline__ BpttBufs bptt_carve(float* lds, const ProblemDesc& pd, int LD) {
    const int mw = max(max(pd.dyn.max_width, pd.pol.max_width), pd.ns + pd.na);
    BpttBufs e;
    e.S = lds; e.XN = e.S + pd.ns * LD; e.LAM = e.XN + pd.ns * LD; e.U = e.LAM + pd.ns * LD; e.X = e.U + pd.na * LD;
    e.PH = e.X + (pd.ns + pd.na) * LD; e.DH = e.PH + net_store_rows(pd.pol, true) * LD;
    e.GA = e.DH + net_store_rows(pd.dyn, false) * LD; e.GB = e.GA + mw * LD;
    return e;
}

// forward keeping the output of every layer in `store` (layer l+1 outputs at row offset sum_{j<=l} dims[j]); returns the last layer's
// rows.  with_output = false: the output layer goes to `out_last` instead (not kept).
__device__ __forceinline__ float* mlp_col_store(const NetDesc& net, const float* __restrict__ params, const float* in, float* store,
                                                float* out_last, int LD, int tid) {
    const float* cur = in;
    float* dst = store;
    for (int l = 0; l < net.n_layers; ++l) {
        float* o = (l == net.n_layers - 1 && out_last != nullptr) ? out_last : dst;
        dense_col(params + net.w_off[l], params + net.b_off[l], net.dims[l], net.dims[l + 1], net.act[l], cur, o, LD, tid);
        cur = o;
        dst += net.dims[l + 1] * LD;
    }
    return const_cast<float*>(cur);
}

// STOCH ('bptt-stochastic'): the policy mean gets the noise of nz before the clip, u = clip(mean + eps exp(log_std)) (training.py:115-116);
// the deterministic instantiations never read nz.
// eps of action dim d of (model, t, env b): e4[d & 3] after bptt_eps4 for chunk d >> 2 (drawn when d % 4 == 0); u_pre returned
template <bool STOCH>
__device__ __forceinline__ float bptt_noisy_mean(const BpttNoise& nz, int model, int t, int B, int b, bool active, int na, int d, float m, float e4[4]) {
    if (!STOCH) return m;
    if ((d & 3) == 0) {
        if (active) bptt_eps4(nz, model, t, B, b, na, d >> 2, e4);
        else e4[0] = e4[1] = e4[2] = e4[3] = 0.0f;
    }
    return fmaf(e4[d & 3], expf(nz.log_std[d]), m);
}

// XS [K][T+1][B][ns], WT [K][T][B], costs [K] (+=)
template <bool STOCH>
__global__ void k_bptt_forward(ProblemDesc pd, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm,
                               const float* __restrict__ s0, int B, int T, double gamma, float* __restrict__ XS, float* __restrict__ WT,
                               double* __restrict__ costs, BpttNoise nz) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[16];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int b = blockIdx.x * blockDim.x + tid, model = blockIdx.y;
    const bool active = b < B;
    const int ns = pd.ns, na = pd.na, K = pd.K;
    BpttBufs e = bptt_carve(lds, pd, LD);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_mean = norm + 2 * (ns + na); const float* diff_std = diff_mean + ns;
    const float* __restrict__ pk = dynp + (size_t)model * pd.dyn.n_params;
    float* xs = XS + (size_t)model * (T + 1) * B * ns;
    for (int i = 0; i < ns; ++i) { const float v = active ? s0[(size_t)b * ns + i] : 0.0f; e.S[i * LD + tid] = v; if (active) xs[(size_t)b * ns + i] = v; }
    double acc = 0.0, g = 1.0;
    float dones = 0.0f;
    for (int t = 0; t < T; ++t) {
        float* m = mlp_col(pd.pol, theta, e.S, e.GA, e.GB, LD, tid);
        float e4[4];
        for (int d = 0; d < na; ++d) {
            const float u = fminf(fmaxf(bptt_noisy_mean<STOCH>(nz, model, t, B, b, active, na, d, m[d * LD + tid], e4), -1.0f), 1.0f);   // :128
            e.U[d * LD + tid] = u;
            if (STOCH && nz.n_sat != nullptr && active && fabsf(u) == 1.0f) atomicAdd(&nz.n_sat[(size_t)b * na + d], 1);       // :129
        }
        for (int i = 0; i < ns; ++i) e.X[i * LD + tid] = (e.S[i * LD + tid] - in_mean[i]) / in_std[i];
        for (int d = 0; d < na; ++d) e.X[(ns + d) * LD + tid] = (e.U[d * LD + tid] - in_mean[ns + d]) / in_std[ns + d];
        float* out = mlp_col(pd.dyn, pk, e.X + pd.n_drop * LD, e.GA, e.GB, LD, tid);
        for (int i = 0; i < ns; ++i) e.XN[i * LD + tid] = fmaf(diff_std[i], out[i * LD + tid], diff_mean[i]) + e.S[i * LD + tid];
        const float c = env_cost(pd.env, ns, na, env_col(e.XN, LD, tid), env_col(e.U, LD, tid));
        const float live = 1.0f - dones;
        if (pd.env == METRPO_ENV_ANT) dones = fmaxf(dones, env_done_scan(pd.env, ns, env_col(e.XN, LD, tid)) ? 1.0f : 0.0f);
        if (active) {
            acc += g * (double)(c * live);
            WT[((size_t)model * T + t) * B + b] = (float)(g * (double)live / ((double)B * (double)K));
            for (int i = 0; i < ns; ++i) xs[((size_t)(t + 1) * B + b) * ns + i] = e.XN[i * LD + tid];
        }
        g *= gamma;
        for (int i = 0; i < ns; ++i) e.S[i * LD + tid] = e.XN[i * LD + tid];
    }
    const double tot = block_sum(acc, red);
    if (tid == 0) costs[(size_t)model * gridDim.x + blockIdx.x] = tot / (double)B;      // one partial per block; added in block order by k_det_cost_reduce
}

// GM [K][T+1][B][na]: adjoint of the (pre-clip) policy mean for every sample; slice t = T stays zero.  STOCH: the clip gate is taken on
// mean + eps exp(log_std), eps recomputed (d u_pre / d mean = 1, so GM keeps its meaning)
template <bool STOCH>
__global__ void k_bptt_backward(ProblemDesc pd, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm,
                                int B, int T, const float* __restrict__ XS, const float* __restrict__ WT, float* __restrict__ GM, BpttNoise nz) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int b = blockIdx.x * blockDim.x + tid, model = blockIdx.y;
    const bool active = b < B;
    const int ns = pd.ns, na = pd.na;
    const NetDesc& dn = pd.dyn; const NetDesc& pn = pd.pol;
    BpttBufs e = bptt_carve(lds, pd, LD);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_std = norm + 2 * (ns + na) + ns;
    const float* __restrict__ pk = dynp + (size_t)model * dn.n_params;
    const float* xs = XS + (size_t)model * (T + 1) * B * ns;
    for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        for (int i = 0; i < ns; ++i) {
            e.S[i * LD + tid] = active ? xs[((size_t)t * B + b) * ns + i] : 0.0f;
            e.XN[i * LD + tid] = active ? xs[((size_t)(t + 1) * B + b) * ns + i] : 0.0f;
        }
        const float w = active ? WT[((size_t)model * T + t) * B + b] : 0.0f;
        // ---- recompute the step: policy (all layer outputs kept), clip, normalise, dynamics hidden layers ----
        float* mu = mlp_col_store(pn, theta, e.S, e.PH, nullptr, LD, tid);         // output rows: not read by the policy VJP below
        float e4[4];
        for (int d = 0; d < na; ++d) {
            if (STOCH) mu[d * LD + tid] = bptt_noisy_mean<STOCH>(nz, model, t, B, b, active, na, d, mu[d * LD + tid], e4);
            e.U[d * LD + tid] = fminf(fmaxf(mu[d * LD + tid], -1.0f), 1.0f);
        }
        for (int i = 0; i < ns; ++i) e.X[i * LD + tid] = (e.S[i * LD + tid] - in_mean[i]) / in_std[i];
        for (int d = 0; d < na; ++d) e.X[(ns + d) * LD + tid] = (e.U[d * LD + tid] - in_mean[ns + d]) / in_std[ns + d];
        net_hidden(dn, pk, e.X + pd.n_drop * LD, e.DH, LD, tid);
        // ---- adjoints: G = lambda_{t+1} + w dc/dx_next ;  gU_cost = w dc/du (kept in XN's place after use) -------------------
        float* G = e.LAM;                                       // lambda_{t+1} is consumed here
        float* gUc = e.X;                                       // the normalised input is dead after the forward recompute
        env_cost_adjoint(pd.env, ns, na, e.XN, e.U, w, gUc, G, LD, tid);
        // dynamics VJP: delta_out = diff_std * G ; back through the layers (relu masks from DH)
        for (int i = 0; i < ns; ++i) e.GA[i * LD + tid] = diff_std[i] * G[i * LD + tid];
        float* da = net_vjp(dn, pk, e.DH, e.GA, e.GB, LD, tid);
        float* db = (da == e.GA) ? e.GB : e.GA;
        // da = adjoint of the (dropped) normalised input [nin].  State part: residual + normaliser; action part -> gU
        for (int i = 0; i < ns; ++i) {
            float v = G[i * LD + tid];
            if (i >= pd.n_drop) v += da[(i - pd.n_drop) * LD + tid] / in_std[i];
            e.XN[i * LD + tid] = v;                             // gS (x_next is dead now)
        }
        for (int d = 0; d < na; ++d) {
            const float gu = gUc[d * LD + tid] + da[(ns - pd.n_drop + d) * LD + tid] / in_std[ns + d];
            const float m = mu[d * LD + tid];
            const float gm = (m >= -1.0f && m <= 1.0f) ? gu : 0.0f;             // tf.clip_by_value gradient
            db[d * LD + tid] = gm;
            if (active) GM[(((size_t)model * (T + 1) + t) * B + b) * na + d] = gm;
        }
        // policy input VJP: back through the layers with the stored activations
        const float* pa = net_vjp(pn, theta, e.PH, db, da, LD, tid);
        for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = e.XN[i * LD + tid] + pa[i * LD + tid];       // lambda_t
    }
}

// tf.clip_by_norm per variable + tf.train.AdamOptimizer on theta (one block per variable: W_l, b_l, log_std; the log_std gradient is 0 in
// the 'bptt' branch and k_bptt_logstd_* in 'bptt-stochastic')
__global__ void k_policy_adam(int n_seg, const int* __restrict__ seg_off, const double* __restrict__ grad, float* __restrict__ theta,
                              float* __restrict__ am, float* __restrict__ av, float lr_t, float b1, float b2, float eps, double clip_val) {
    __shared__ double red[16];
    __shared__ double s_scale;
    const int s = blockIdx.x, lo = seg_off[s], hi = seg_off[s + 1];
    double nn = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) nn += grad[i] * grad[i];
    const double tot = block_sum(nn, red);
    if (threadIdx.x == 0) { const double n = sqrt(tot); s_scale = (clip_val > 0.0) ? clip_val / fmax(n, clip_val) : 1.0; }
    __syncthreads();
    const double sc = s_scale;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        tf_adam_elem((float)(grad[i] * sc), theta, am, av, i, lr_t, b1, b2, eps);
    }
}

// 'bptt-stochastic' log_std gradient (bptt.hip header; the mean-adjoint GM is the adjoint of u_pre = mean + eps exp(log_std)):
//   g[log_std_d] = exp(p_d) * sum_{i,t,b} GM[i][t][b][d] eps[i][t][b][d]
// float64 in a fixed order: thread (block x, lane l) of action chunk blockIdx.y sums the samples s = (i T + t) B + b with s = 256 x + l mod
// (gridDim.x 256), in increasing s; the block's tree (block_sum) gives one partial per (chunk, block, dim); k_bptt_logstd_final adds a dim's
// partials in block order.  eps is recomputed exactly as the sweeps drew it (bptt_eps4), so nothing of [K][T][B][na] size is stored.
constexpr int LOGSTD_BLOCKS = 128;
__global__ void __launch_bounds__(256) k_bptt_logstd_part(int K, int T, int B, int na, const float* __restrict__ GM, BpttNoise nz,
                                                          double* __restrict__ part) {
    __shared__ double red[16];
    const int ch = blockIdx.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const long long n = (long long)K * T * B;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
        const int b = (int)(s % B);
        const long long it = s / B;
        const int t = (int)(it % T), i = (int)(it / T);
        float e[4];
        bptt_eps4(nz, i, t, B, b, na, ch, e);
        const float* gm = GM + (((size_t)i * (T + 1) + t) * B + b) * na;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * ch + j < na) acc[j] += (double)gm[4 * ch + j] * (double)e[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double v = block_sum(acc[j], red);
        if (threadIdx.x == 0) part[((size_t)ch * gridDim.x + blockIdx.x) * 4 + j] = v;
    }
}

// out[d] (the log_std slots of the gradient) = exp(p_d) * the nblk partials of dim d added in block order
__global__ void k_bptt_logstd_final(int na, int nblk, const double* __restrict__ part, const float* __restrict__ log_std, double* __restrict__ out) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= na) return;
    double s = 0.0;
    for (int x = 0; x < nblk; ++x) s += part[((size_t)(d >> 2) * nblk + x) * 4 + (d & 3)];
    out[d] = s * exp((double)log_std[d]);
}

// -------------------------------------------------------------------------------------------------
// nz == NULL: the 'bptt' gradient; otherwise 'bptt-stochastic' with the noise of *nz (nz->n_sat zeroed here when set)
int launch_bptt_grad(metrpo_ctx* c, const float* init, int B, int T, double gamma, double* costs, double* grad, hipStream_t st, const BpttNoise* nz) {
    const ProblemDesc& pd = c->pd;
    const int K = pd.K, ns = pd.ns, na = pd.na;
    const int nchunk = (na + 3) / 4;
    const size_t nXS = (((size_t)K * (T + 1) * B * ns) + 3) & ~(size_t)3, nWT = (((size_t)K * T * B) + 3) & ~(size_t)3,
                 nGM = (((size_t)K * (T + 1) * B * na) + 3) & ~(size_t)3;
    const size_t nLS = nz ? (size_t)nchunk * LOGSTD_BLOCKS * 4 : 0;
    const size_t need = (nXS + nWT + nGM) * sizeof(float) + sizeof(double) * (size_t)(pd.P + 1 + K + nLS);
    if (c->det_cfg >= 0) { const int rc0 = ensure_detpart(c, B); if (rc0) return rc0; }
    { const int rc = ws_grow(c, c->d_bptt, need); if (rc) return rc; }
    float* XS = (float*)c->d_bptt.p; float* WT = XS + nXS; float* GM = WT + nWT;
    double* gout = (double*)(GM + nGM); double* cst = gout + pd.P + 1; double* lpart = cst + K;
    HIP_TRY(c, hipMemsetAsync(GM, 0, sizeof(float) * nGM, st));
    if (nz && nz->n_sat) HIP_TRY(c, hipMemsetAsync(nz->n_sat, 0, sizeof(int) * (size_t)B * na, st));
    if (c->det_cfg >= 0) {                                   // MFMA sweeps (bptt_mfma.hip)
        int rc1 = launch_det_forward(c, c->det_cfg, init, B, T, gamma, XS, WT, c->d_detpart.p, cst, st, nz);
        if (rc1) return rc1;
        if ((rc1 = launch_det_backward(c, c->det_cfg, B, T, XS, WT, GM, st, nz))) return rc1;
    } else if (c->det_gemm) {                                // GEMM-path sweeps for large dynamics nets (det_gemm.hip)
        int rc1 = launch_dg_forward(c, init, B, T, gamma, XS, WT, cst, st, nz);
        if (rc1) return rc1;
        if ((rc1 = launch_dg_backward(c, B, T, XS, WT, GM, st, nz))) return rc1;
    } else {
        const size_t fpt = bptt_floats(pd);
        const int bs = lds_block_size(fpt);
        if (bs == 0) return set_err(c, METRPO_EUNSUPPORTED, "bptt: layer widths exceed the LDS budget of the generic kernel");
        const size_t sh = fpt * bs * sizeof(float);
        const void* fwd = nz ? (const void*)k_bptt_forward<true> : (const void*)k_bptt_forward<false>;
        const void* bwd = nz ? (const void*)k_bptt_backward<true> : (const void*)k_bptt_backward<false>;
        if (sh > 64 * 1024) {
            HIP_TRY(c, hipFuncSetAttribute(fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            HIP_TRY(c, hipFuncSetAttribute(bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        }
        const dim3 grid((B + bs - 1) / bs, K);
        const BpttNoise nz0 = nz ? *nz : BpttNoise{};
        { const int rcp = ensure_detpart_n(c, (size_t)K * grid.x); if (rcp) return rcp; }
        if (nz) hipLaunchKernelGGL(k_bptt_forward<true>, grid, dim3(bs), sh, st, pd, c->d_dyn.p, c->d_theta.p, c->d_norm.p, init, B, T, gamma, XS, WT, c->d_detpart.p, nz0);
        else hipLaunchKernelGGL(k_bptt_forward<false>, grid, dim3(bs), sh, st, pd, c->d_dyn.p, c->d_theta.p, c->d_norm.p, init, B, T, gamma, XS, WT, c->d_detpart.p, nz0);
        { const int rcp = launch_det_cost_reduce(c, (int)grid.x, c->d_detpart.p, cst, st); if (rcp) return rcp; }
        if (nz) hipLaunchKernelGGL(k_bptt_backward<true>, grid, dim3(bs), sh, st, pd, c->d_dyn.p, c->d_theta.p, c->d_norm.p, B, T, XS, WT, GM, nz0);
        else hipLaunchKernelGGL(k_bptt_backward<false>, grid, dim3(bs), sh, st, pd, c->d_dyn.p, c->d_theta.p, c->d_norm.p, B, T, XS, WT, GM, nz0);
        HIP_TRY(c, hipGetLastError());
    }
    // policy-parameter gradient: sum over the K (T+1) B samples of J(x)^T gm  (gradient kernels of the TRPO update, mean-adjoint supplied)
    const int rc = launch_policy_vjp(c, XS, GM, (long long)K * (T + 1) * B, gout, st);
    if (rc) return rc;
    if (nz) {                                                // the log_std slots (0 from the VJP: the mean does not depend on log_std)
        hipLaunchKernelGGL(k_bptt_logstd_part, dim3(LOGSTD_BLOCKS, nchunk), dim3(256), 0, st, K, T, B, na, (const float*)GM, *nz, lpart);
        hipLaunchKernelGGL(k_bptt_logstd_final, dim3((na + 63) / 64), dim3(64), 0, st, na, LOGSTD_BLOCKS, (const double*)lpart, nz->log_std, gout + 1 + pd.pol.n_params);
        HIP_TRY(c, hipGetLastError());
    }
    if (grad) HIP_TRY(c, hipMemcpyAsync(grad, gout + 1, sizeof(double) * pd.P, hipMemcpyDeviceToDevice, st));
    if (costs) HIP_TRY(c, hipMemcpyAsync(costs, cst, sizeof(double) * K, hipMemcpyDeviceToDevice, st));
    return METRPO_OK;
}

// policy optimizer state: m [P] | v [P] | segment table (one clip_by_norm segment per variable) [2L+2] int
int ensure_policy_adam(metrpo_ctx* c) {
    const ProblemDesc& pd = c->pd;
    const int P = pd.P, L = pd.pol.n_layers, nseg = 2 * L + 1;
    bool grew = false;
    { const int rc = ws_grow(c, c->d_pol_adam, sizeof(float) * 2 * (size_t)P + sizeof(int) * (nseg + 1), &grew); if (rc || !grew) return rc; }
    HIP_TRY(c, hipMemset(c->d_pol_adam.p, 0, sizeof(float) * 2 * (size_t)P));
    int seg[2 * MAXL + 2];
    for (int l = 0; l < L; ++l) { seg[2 * l] = pd.pol.w_off[l]; seg[2 * l + 1] = pd.pol.b_off[l]; }
    seg[2 * L] = pd.pol.n_params; seg[2 * L + 1] = P;
    HIP_TRY(c, hipMemcpy((char*)c->d_pol_adam.p + sizeof(float) * 2 * (size_t)P, seg, sizeof(int) * (nseg + 1), hipMemcpyHostToDevice));
    c->pol_adam_t = 0;
    return METRPO_OK;
}

int launch_policy_adam(metrpo_ctx* c, const double* grad, double lr, double b1, double b2, double eps, double clip_val, bool reset, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const int P = pd.P, L = pd.pol.n_layers, nseg = 2 * L + 1;
    { const int rc = ensure_policy_adam(c); if (rc) return rc; }
    float* am = (float*)c->d_pol_adam.p; float* av = am + P;
    if (reset) {
        HIP_TRY(c, hipMemsetAsync(am, 0, sizeof(float) * 2 * (size_t)P, st));
        c->pol_adam_t = 0;
        return METRPO_OK;
    }
    c->pol_adam_t += 1;
    const double lr_t = lr * std::sqrt(1.0 - std::pow(b2, (double)c->pol_adam_t)) / (1.0 - std::pow(b1, (double)c->pol_adam_t));
    hipLaunchKernelGGL(k_policy_adam, dim3(nseg), dim3(256), 0, st, nseg, (const int*)(av + P), grad, c->d_theta.p, am, av, (float)lr_t, (float)b1,
                       (float)b2, (float)eps, clip_val);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int ensure_detpart(metrpo_ctx* c, int B) { return ensure_detpart_n(c, (size_t)c->pd.K * (size_t)(4 * ((B + 63) / 64))); }
int ensure_detpart_n(metrpo_ctx* c, size_t n_doubles) {
    const size_t need = sizeof(double) * n_doubles;
    return ws_grow(c, c->d_detpart, need);
}
