// 'svg' policy update: value gradients along RECORDED rollouts (svg_utils.py:12-66 svg_gradient / svg_update; wired at model_based_rl.py:381-389,
// :654-660, :1204-1205).  Per rollout, t = len-1 .. 0 with lambda = 0:
//   c_s, c_a = d cost_tf(None, a_t, s_t) / d (s_t, a_t)       (the cost's x_next IS s_t, svg_utils.py:123-125)
//   Pi_t = d policy_mean(s_t) / d s_t  [na x ns]              (raw mean net, no clip)
//   F_t  = d model_head([s_t, a_t]) / d [s_t, a_t]  [ns x (ns+na)]   (normalisers, column drop and residual included; a_t as recorded)
//   q_t = c_a + gamma lambda F_t[:, ns:]      g_theta += gamma^t q_t J_theta(s_t)      lambda = c_s + q_t Pi_t + gamma lambda F_t[:, :ns]
// and avg_grads = the mean over the rollouts of g_theta and of lambda_0.
//
// The states and actions are recorded, so every Jacobian factor is known before the sweep starts and only the state-adjoint chain is serial:
//   stage A  F_t and Pi_t for all N = n T samples at once, in chunks that bound the workspace.  Two forms of the dynamics Jacobian: the GENERIC kernel
//            (thread = (sample, output row), activations in LDS columns as bptt.hip keeps them; any widths and activations) and the GEMM form (the
//            forward hidden layers by the tile GEMMs, a rank-one seed at the last hidden layer, then the transposed chain with the OUTPUT ROW as the
//            batch axis of gemm_auto -- one mask and one weight matrix serve all ns row blocks, as launch_dg_backward's launches do with heads = K).
//            Pi_t always comes from the generic kernel: the policy is small.
//   stage B  k_svg_scan, one wave per rollout: lambda and q in float64 (the reference's NumPy recursion), lanes over columns, sums over the row index
//            in a fixed order -- no atomics, bit-reproducible; the next step's F, Pi, s, a are in flight while this step's sums run.
//   stage C  the policy VJP of the update kernels on (s_t, gamma^t q_t), then k_svg_close: / n, the rollouts' lambda_0 added in rollout order, log_std
//            slots zeroed and, for metrpo_svg_update, theta += float32(-lr) * float32(g) on the W / b segments (svg_utils.py:56-66).
// Rows at or behind a rollout's length never reach a result: k_svg_prep copies the recorded rows into the workspace and writes zeros there, the scan
// stops at len, and the mean-adjoint of those rows is zero.
#include <algorithm>
#include <cmath>
#include "gemm_mfma.h"

__device__ __forceinline__ float svg_dact(int act, float h) {
    return (act == METRPO_ACT_RELU) ? (h > 0.0f ? 1.0f : 0.0f) : (act == METRPO_ACT_TANH) ? fmaf(-h, h, 1.0f) : 1.0f;
}

// OBSZ / ACTZ: the recorded rows in front of each rollout's length, zeros behind it; LEN: the clamped lengths
__global__ void k_svg_prep(int n, int T, int ns, int na, const float* __restrict__ obs, const float* __restrict__ act, const int32_t* __restrict__ d_len,
                           float* __restrict__ OBSZ, float* __restrict__ ACTZ, int32_t* __restrict__ LEN) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (long long)n * T) return;
    const int r = (int)(row / T), t = (int)(row % T);
    const int len = d_len ? min(max(d_len[r], 1), T) : T;
    if (t == 0) LEN[r] = len;
    if (t < len) {
        for (int i = 0; i < ns; ++i) OBSZ[(size_t)row * ns + i] = obs[(size_t)row * ns + i];
        for (int d = 0; d < na; ++d) ACTZ[(size_t)row * na + d] = act[(size_t)row * na + d];
    } else {
        for (int i = 0; i < ns; ++i) OBSZ[(size_t)row * ns + i] = 0.0f;
        for (int d = 0; d < na; ++d) ACTZ[(size_t)row * na + d] = 0.0f;
    }
}

// ---- stage A, generic: one thread per (sample, output row) ---------------------------------------------------------------------------------------
// LDS columns of a thread: IN [n_in] | H [hidden rows] | GA, GB [max width].  DYN: net = head `params` of the dynamics, row i of F; else the policy
// mean net, row d of Pi.  Forward hidden layers kept, the output layer's transposed product seeds the last hidden layer (rank one), then back
// through the layers as k_bptt_backward does.
__host__ __device__ inline size_t svg_jac_floats(const NetDesc& net) {
    int hid = 0;
    for (int l = 1; l < net.n_layers; ++l) hid += net.dims[l];
    return (size_t)net.dims[0] + hid + 2 * (size_t)net.max_width;
}

template <bool DYN>
__global__ void k_svg_jac(ProblemDesc pd, const float* __restrict__ params, const float* __restrict__ norm, const float* __restrict__ OBSZ,
                          const float* __restrict__ ACTZ, long long s0, int cnt, float* __restrict__ OUT) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int ns = pd.ns, na = pd.na, nsa = ns + na;
    const NetDesc& net = DYN ? pd.dyn : pd.pol;
    const int L = net.n_layers, nrow = DYN ? ns : na;
    const long long gid = (long long)blockIdx.x * blockDim.x + tid;
    const bool active = gid < (long long)cnt * nrow;
    const long long S = s0 + (active ? gid / nrow : 0);           // (an idle thread recomputes sample s0 and stores nothing)
    const int row = active ? (int)(gid % nrow) : 0;
    int hid = 0;
    for (int l = 1; l < L; ++l) hid += net.dims[l];
    float* IN = lds; float* H = IN + net.dims[0] * LD; float* da = H + hid * LD; float* db = da + net.max_width * LD;
    const float* in_mean = norm; const float* in_std = norm + nsa; const float* diff_std = norm + 2 * nsa + ns;
    if (DYN) {
        for (int c = pd.n_drop; c < nsa; ++c) {
            const float v = (c < ns) ? OBSZ[(size_t)S * ns + c] : ACTZ[(size_t)S * na + (c - ns)];
            IN[(c - pd.n_drop) * LD + tid] = (v - in_mean[c]) / in_std[c];
        }
    } else {
        for (int i = 0; i < ns; ++i) IN[i * LD + tid] = OBSZ[(size_t)S * ns + i];
    }
    net_hidden(net, params, IN, H, LD, tid);
    int off = 0;                                                   // rows of the LAST hidden layer in H
    for (int l = 1; l < L - 1; ++l) off += net.dims[l];
    {
        const float* __restrict__ Wo = params + net.w_off[L - 1];
        const int n_in = net.dims[L - 1], n_out = net.dims[L];
        const float sc = DYN ? diff_std[row] : 1.0f;
        for (int j = 0; j < n_in; ++j) {
            float v = sc * Wo[(size_t)j * n_out + row];
            if (L > 1) v *= svg_dact(net.act[L - 2], H[(off + j) * LD + tid]);
            da[j * LD + tid] = v;
        }
    }
    for (int l = L - 2; l >= 0; --l) {
        dense_col_T(params + net.w_off[l], net.dims[l], net.dims[l + 1], da, db, LD, tid);
        if (l > 0) {
            off -= net.dims[l];
            const float* h = H + off * LD;                         // output of layer l - 1
            for (int j = 0; j < net.dims[l]; ++j) db[j * LD + tid] *= svg_dact(net.act[l - 1], h[j * LD + tid]);
        }
        float* tmp = da; da = db; db = tmp;
    }
    if (!active) return;
    if (DYN) {
        float* o = OUT + ((size_t)S * ns + row) * nsa;
        for (int c = 0; c < nsa; ++c) {
            float v = (c == row) ? 1.0f : 0.0f;                    // the residual's identity
            if (c >= pd.n_drop) v += da[(c - pd.n_drop) * LD + tid] / in_std[c];
            o[c] = v;
        }
    } else {
        float* o = OUT + ((size_t)S * na + row) * ns;
        for (int i = 0; i < ns; ++i) o[i] = da[i * LD + tid];
    }
}

// ---- stage A, GEMM form ---------------------------------------------------------------------------------------------------------------------------
// X [cnt][nin]: the normalised, column-dropped input of the chunk's samples
__global__ void k_svg_x(ProblemDesc pd, const float* __restrict__ norm, const float* __restrict__ OBSZ, const float* __restrict__ ACTZ, long long s0, int cnt,
                        float* __restrict__ X) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)cnt * pd.nin) return;
    const int nsa = pd.ns + pd.na;
    const long long s = e / pd.nin; const int c = (int)(e % pd.nin) + pd.n_drop;
    const float v = (c < pd.ns) ? OBSZ[(size_t)(s0 + s) * pd.ns + c] : ACTZ[(size_t)(s0 + s) * pd.na + (c - pd.ns)];
    X[e] = (v - norm[c]) / norm[nsa + c];
}
// dz[i][s][j] = diff_std[i] W_out[j][i] relu'(h_last[s][j]): the output layer's transposed product is rank one and needs no GEMM
__global__ void k_svg_seed(int ns, int cnt, int nh, const float* __restrict__ diff_std, const float* __restrict__ Wout, const float* __restrict__ Hlast,
                           float* __restrict__ dz) {
    const long long tot = (long long)ns * cnt * nh;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(e % nh); const long long is = e / nh;
        const int s = (int)(is % cnt), i = (int)(is / cnt);
        dz[e] = (Hlast[(size_t)s * nh + j] > 0.0f) ? diff_std[i] * Wout[(size_t)j * ns + i] : 0.0f;
    }
}
// F[s0 + s][i][c] = 1 / in_std[c] dz[i][s][c - n_drop] (dropped columns: 0) + the residual's identity
__global__ void k_svg_finish(ProblemDesc pd, const float* __restrict__ norm, const float* __restrict__ dz, long long s0, int cnt, float* __restrict__ F) {
    const int ns = pd.ns, nsa = pd.ns + pd.na;
    const long long tot = (long long)cnt * ns * nsa;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e % nsa); const long long si = e / nsa;
        const int i = (int)(si % ns), s = (int)(si / ns);
        float v = (c == i) ? 1.0f : 0.0f;
        if (c >= pd.n_drop) v += dz[((size_t)i * cnt + s) * pd.nin + (c - pd.n_drop)] / norm[nsa + c];
        F[(size_t)s0 * ns * nsa + e] = v;
    }
}

// ---- stage B: the scan ----------------------------------------------------------------------------------------------------------------------------
// d cost(x_next = s, u = a) / d column c of [s | a]: the cost adjoint's per-dimension terms (env_model.h) at w = 1.  sa: the step's [s | a] in LDS.
// (Ant's columns would now carry Ant's terms where they were 0: svg is undefined on Ant and svg_check (api.hip) refuses it, so no launch reaches them.)
__device__ __forceinline__ float svg_cost_grad(int env, int ns, int na, const float* sa, int c) {
    const EnvVec x = {sa, 1}, u = {sa + ns, 1};
    const bool inside = env_clip_inside_at(env, ns, x, (env == METRPO_ENV_HALF_CHEETAH) ? env_su2(na, u) : 0.0f);
    return (c >= ns) ? env_cost_du(env, na, inside, 1.0f) * u(c - ns) : env_cost_dx(env, ns, c, x(c), inside, 1.0f);
}

// One wave per rollout.  A step's operands -- F_t [ns][nsa] | Pi_t [na][ns] | s_t | a_t, E floats -- are staged in LDS; lane l holds elements
// l, l + 64, ... of the NEXT step in PF registers while this step's sums run (they do not depend on lambda); PF = 4, 16 or 64 by E (the launcher
// picks the smallest that holds a step: every register costs a predicated load and a predicated LDS store per step), elements from 64 PF on
// (E > 4096: humanoid's 5411) are loaded where they are staged.  lam, q, v: float64 in LDS.  GM rows at or behind len are zeroed by the launcher.
template <int SVG_PF>
__global__ void __launch_bounds__(64) k_svg_scan(int env, int ns, int na, int T, double gamma, const int32_t* __restrict__ LEN, const float* __restrict__ OBSZ,
                                                 const float* __restrict__ ACTZ, const float* __restrict__ F, const float* __restrict__ PI,
                                                 float* __restrict__ GM, double* __restrict__ LAM0) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, r = blockIdx.x, nsa = ns + na;
    const int nF = ns * nsa, nP = na * ns, E = nF + nP + nsa;
    double* lam = (double*)lds; double* qq = lam + ns; double* vv = qq + na;
    float* stage = (float*)(vv + ns);
    const float* Fs = stage; const float* Ps = stage + nF; const float* sa = Ps + nP;
    const int len = LEN[r];
    auto ld = [&](long long row, int e) -> float {
        if (e < nF) return F[(size_t)row * nF + e];
        if (e < nF + nP) return PI[(size_t)row * nP + (e - nF)];
        e -= nF + nP;
        return (e < ns) ? OBSZ[(size_t)row * ns + e] : ACTZ[(size_t)row * na + (e - ns)];
    };
    float pre[SVG_PF];
    auto load_pre = [&](long long row) {
#pragma unroll
        for (int k = 0; k < SVG_PF; ++k) { const int e = lane + 64 * k; pre[k] = (e < E) ? ld(row, e) : 0.0f; }
    };
    for (int i = lane; i < ns; i += 64) lam[i] = 0.0;
    load_pre((long long)r * T + (len - 1));
    for (int t = len - 1; t >= 0; --t) {
        const long long row = (long long)r * T + t;
#pragma unroll
        for (int k = 0; k < SVG_PF; ++k) { const int e = lane + 64 * k; if (e < E) stage[e] = pre[k]; }
        for (int e = lane + 64 * SVG_PF; e < E; e += 64) stage[e] = ld(row, e);
        __syncthreads();
        if (t > 0) load_pre(row - 1);
        const double gt = pow(gamma, (double)t);
        for (int c = lane; c < nsa; c += 64) {
            double v = 0.0;
            for (int i = 0; i < ns; ++i) v = fma(lam[i], (double)Fs[i * nsa + c], v);
            if (c < ns) vv[c] = v;
            else {
                const double q = (double)svg_cost_grad(env, ns, na, sa, c) + gamma * v;
                qq[c - ns] = q;
                GM[(size_t)row * na + (c - ns)] = (float)(gt * q);
            }
        }
        __syncthreads();
        for (int c = lane; c < ns; c += 64) {
            double acc = (double)svg_cost_grad(env, ns, na, sa, c);
            for (int d = 0; d < na; ++d) acc = fma(qq[d], (double)Ps[d * ns + c], acc);
            lam[c] = acc + gamma * vv[c];
        }
        __syncthreads();
    }
    for (int i = lane; i < ns; i += 64) LAM0[(size_t)r * ns + i] = lam[i];
}

// ---- stage C's closing kernel -----------------------------------------------------------------------------------------------------------------------
// grad[p] = gout[1 + p] / n on the W / b segments, exactly 0 on the log_std slots; state[c] = (sum_r lam0[r][c], rollout order) / n;
// nlr != 0 (metrpo_svg_update): theta[p] += float32(-lr) * float32(grad[p]), the product rounded before the sum as NumPy's float32 arithmetic rounds it
__global__ void k_svg_close(int P, int npol, int n, int ns, const double* __restrict__ gout, const double* __restrict__ LAM0, double* __restrict__ grad,
                            double* __restrict__ state, float* __restrict__ theta, float nlr, int update) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) {
        const double g = (i < npol) ? gout[1 + i] / (double)n : 0.0;
        grad[i] = g;
        if (update && i < npol) { const float step = nlr * (float)g; theta[i] = theta[i] + step; }
    }
    if (state != nullptr && i < ns) {
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += LAM0[(size_t)r * ns + i];
        state[i] = s / (double)n;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static bool svg_gemm_ok(const metrpo_ctx* c) {
    if (!gemm_path_applicable(c)) return false;
    for (int l = 0; l < c->pd.dyn.n_layers - 1; ++l) if (c->pd.dyn.act[l] != METRPO_ACT_RELU) return false;
    return true;
}

// threads per block of k_svg_jac on `net`: the largest of 64, 32, ... whose LDS columns fit; 0: none does
static int svg_jac_block(const NetDesc& net, size_t* lds_bytes) {
    const size_t fpt = svg_jac_floats(net);
    const int bs = lds_block_size(fpt);
    if (bs == 0) return 0;
    *lds_bytes = fpt * bs * sizeof(float);
    return bs;
}

// Samples per Jacobian chunk when the caller leaves the choice (chunk = 0).  GEMM form: the two buffers of the transposed chain, 2 ns chunk maxw
// floats, stay within 2^26 floats (256 MiB; the 1024 x 1024 humanoid nets: 576 samples), a multiple of 64 and at least 64.  Generic form: no
// workspace grows with the chunk, 65 536 samples bound a launch's grid.
static int svg_default_chunk(const ProblemDesc& pd, int path, long long N) {
    if (path != 2) return (int)std::min<long long>(N, 65536);
    int maxw = pd.nin;
    for (int l = 1; l < pd.dyn.n_layers; ++l) maxw = std::max(maxw, pd.dyn.dims[l]);
    const long long cap = ((1LL << 26) / (2LL * pd.ns * maxw)) & ~63LL;
    return (int)std::min<long long>(N, std::max<long long>(cap, 64));
}

int run_svg(metrpo_ctx* c, const metrpo_svg_args* a, double lr, bool update, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const int ns = pd.ns, na = pd.na, nsa = ns + na, n = a->n, T = a->T, L = pd.dyn.n_layers;
    const long long N = (long long)n * T;
    const bool gemm_ok = svg_gemm_ok(c);
    if (a->path == 2 && !gemm_ok)
        return set_err(c, METRPO_EUNSUPPORTED, "svg: path = 2 (GEMM) needs relu hidden layers of at least 16 units, two weight layers or more and ns <= 64");
    const int path = a->path ? a->path : (gemm_ok ? 2 : 1);
    const int chunk = a->chunk > 0 ? (int)std::min<long long>(a->chunk, N) : svg_default_chunk(pd, path, N);
    size_t dyn_lds = 0, pol_lds = 0;
    const int pol_bs = svg_jac_block(pd.pol, &pol_lds), dyn_bs = (path == 1) ? svg_jac_block(pd.dyn, &dyn_lds) : 0;
    if (!pol_bs || (path == 1 && !dyn_bs)) return set_err(c, METRPO_EUNSUPPORTED, "svg: layer widths exceed the LDS budget of the generic Jacobian kernel");
    // ---- workspace: OBSZ | ACTZ | GM | F | PI | (GEMM: X | H[l] | DZa | DZb) | LEN | LAM0 | gout ----
    auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
    int maxw = pd.nin;
    for (int l = 1; l < L; ++l) maxw = std::max(maxw, pd.dyn.dims[l]);
    const size_t nO = up4((size_t)N * ns), nA = up4((size_t)N * na), nF = up4((size_t)N * ns * nsa), nP = up4((size_t)N * na * ns);
    size_t nX = 0, nH = 0, nZ = 0;
    if (path == 2) {
        nX = up4((size_t)chunk * pd.nin); nZ = up4((size_t)ns * chunk * maxw);
        for (int l = 1; l < L; ++l) nH += up4((size_t)chunk * pd.dyn.dims[l]);
    }
    const size_t nL = up4((size_t)n);
    const size_t need = (nO + 2 * nA + nF + nP + nX + nH + 2 * nZ + nL) * sizeof(float) + ((size_t)n * ns + pd.P + 1) * sizeof(double) + 16;
    { const int rc = ws_grow(c, c->d_svg, need); if (rc) return rc; }
    float* p = (float*)c->d_svg.p;
    float* OBSZ = p; p += nO; float* ACTZ = p; p += nA; float* GM = p; p += nA; float* Fj = p; p += nF; float* PIj = p; p += nP;
    float* X = p; p += nX;
    float* H[MAXL] = {};
    if (path == 2) for (int l = 1; l < L; ++l) { H[l - 1] = p; p += up4((size_t)chunk * pd.dyn.dims[l]); }
    float* DZa = p; p += nZ; float* DZb = p; p += nZ;
    int32_t* LEN = (int32_t*)p; p += nL;
    double* LAM0 = (double*)(((uintptr_t)p + 15) & ~(uintptr_t)15); double* gout = LAM0 + (size_t)n * ns;

    hipLaunchKernelGGL(k_svg_prep, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, T, ns, na, a->d_obs, a->d_act, a->d_len, OBSZ, ACTZ, LEN);
    HIP_TRY(c, hipMemsetAsync(GM, 0, sizeof(float) * (size_t)N * na, st));
    // ---- stage A ----
    const float* pk = c->d_dyn.p + (size_t)a->model * pd.dyn.n_params;
    if (pol_lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_svg_jac<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pol_lds));
    if (dyn_lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_svg_jac<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds));
    // Pi_t needs no workspace that grows with the chunk: a chunk the caller set is honoured, the library's own choice is the generic path's 65 536
    // (at humanoid 2 x 1024 the GEMM path's 576-sample chunks left this kernel 12 096 threads per launch: 36 % of the call, measured)
    const int pol_chunk = a->chunk > 0 ? chunk : svg_default_chunk(pd, 1, N);
    for (long long s0 = 0; s0 < N; s0 += pol_chunk) {
        const int cnt = (int)std::min<long long>(pol_chunk, N - s0);
        hipLaunchKernelGGL(k_svg_jac<false>, dim3((unsigned)(((long long)cnt * na + pol_bs - 1) / pol_bs)), dim3(pol_bs), pol_lds, st, pd, (const float*)c->d_theta.p,
                           (const float*)c->d_norm.p, (const float*)OBSZ, (const float*)ACTZ, s0, cnt, PIj);
    }
    for (long long s0 = 0; s0 < N; s0 += chunk) {
        const int cnt = (int)std::min<long long>(chunk, N - s0);
        if (path == 1) {
            hipLaunchKernelGGL(k_svg_jac<true>, dim3((unsigned)(((long long)cnt * ns + dyn_bs - 1) / dyn_bs)), dim3(dyn_bs), dyn_lds, st, pd, pk, (const float*)c->d_norm.p,
                               (const float*)OBSZ, (const float*)ACTZ, s0, cnt, Fj);
            continue;
        }
        hipLaunchKernelGGL(k_svg_x, dim3((unsigned)(((long long)cnt * pd.nin + 255) / 256)), dim3(256), 0, st, pd, (const float*)c->d_norm.p, (const float*)OBSZ,
                           (const float*)ACTZ, s0, cnt, X);
        const float* in = X; int ldin = pd.nin;
        for (int l = 0; l < L - 1; ++l) {                        // forward hidden layers of head `model`
            const int Kd = pd.dyn.dims[l], Nn = pd.dyn.dims[l + 1];
            gemm_skinny_bias(in, 0, ldin, pk + pd.dyn.w_off[l], 0, Nn, pk + pd.dyn.b_off[l], 0, H[l], 0, cnt, Nn, Kd, 1, nullptr, st, 1);
            in = H[l]; ldin = Nn;
        }
        const int nh = pd.dyn.dims[L - 1];
        {
            const long long tot = (long long)ns * cnt * nh;
            hipLaunchKernelGGL(k_svg_seed, dim3((unsigned)std::min<long long>((tot + 255) / 256, 8192)), dim3(256), 0, st, ns, cnt, nh,
                               (const float*)c->d_norm.p + 2 * nsa + ns, pk + pd.dyn.w_off[L - 1], (const float*)H[L - 2], DZa);
        }
        float* dz = DZa; float* dzn = DZb;
        for (int l = L - 2; l >= 0; --l) {                       // the transposed chain: batch axis = output row i, weights and mask shared (stride 0)
            const int n_in = pd.dyn.dims[l], n_out = pd.dyn.dims[l + 1];
            const float* Wl = pk + pd.dyn.w_off[l];
            GemmEpi ep = {};
            if (l > 0) {
                ep.mask = H[l - 1]; ep.strideMask = 0; ep.ldm = n_in;
                gemm_auto<EPI_RELU_MASK, false, true>(dz, (long long)cnt * n_out, n_out, Wl, 0, n_out, dzn, (long long)cnt * n_in, n_in, cnt, n_in, n_out, ns, ep, st);
            } else {
                gemm_auto<EPI_PLAIN, false, true>(dz, (long long)cnt * n_out, n_out, Wl, 0, n_out, dzn, (long long)cnt * n_in, n_in, cnt, n_in, n_out, ns, ep, st);
            }
            float* tmp = dz; dz = dzn; dzn = tmp;
        }
        {
            const long long tot = (long long)cnt * ns * nsa;
            hipLaunchKernelGGL(k_svg_finish, dim3((unsigned)std::min<long long>((tot + 255) / 256, 8192)), dim3(256), 0, st, pd, (const float*)c->d_norm.p, (const float*)dz,
                               s0, cnt, Fj);
        }
    }
    // ---- stage B ----
    {
        const size_t sh = sizeof(double) * (size_t)(2 * ns + na) + sizeof(float) * (size_t)(ns * nsa + na * ns + nsa);
        if (sh > 160 * 1024) return set_err(c, METRPO_EUNSUPPORTED, "svg: ns * (ns + na) exceeds the LDS budget of the scan");
        const int E = ns * nsa + na * ns + nsa;
        auto scan = (E <= 256) ? k_svg_scan<4> : (E <= 1024) ? k_svg_scan<16> : k_svg_scan<64>;
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL(scan, dim3(n), dim3(64), sh, st, pd.env, ns, na, T, a->gamma, (const int32_t*)LEN, (const float*)OBSZ, (const float*)ACTZ,
                           (const float*)Fj, (const float*)PIj, GM, LAM0);
    }
    HIP_TRY(c, hipGetLastError());
    // ---- stage C ----
    { const int rc = launch_policy_vjp(c, OBSZ, GM, N, gout, st); if (rc) return rc; }
    hipLaunchKernelGGL(k_svg_close, dim3((std::max(pd.P, ns) + 255) / 256), dim3(256), 0, st, pd.P, pd.pol.n_params, n, ns, (const double*)gout, (const double*)LAM0,
                       a->d_grad, a->d_state_grad, c->d_theta.p, (float)(-lr), update ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    if (update) { c->pg_fwd_rows = -1; c->f3_rows = -1; }           // activation caches keyed on theta (policy_gemm.hip, policy_fused3.hip)
    if (a->d_mean_adj) HIP_TRY(c, hipMemcpyAsync(a->d_mean_adj, GM, sizeof(float) * (size_t)N * na, hipMemcpyDeviceToDevice, st));
    if (a->d_dyn_jac) HIP_TRY(c, hipMemcpyAsync(a->d_dyn_jac, Fj, sizeof(float) * (size_t)N * ns * nsa, hipMemcpyDeviceToDevice, st));
    if (a->d_pol_jac) HIP_TRY(c, hipMemcpyAsync(a->d_pol_jac, PIj, sizeof(float) * (size_t)N * na * ns, hipMemcpyDeviceToDevice, st));
    c->last_svg_path = path;
    return METRPO_OK;
}
