// Policy-side kernels of the NPO/TRPO update (algos/npo.py:68-111; [rllab] ConjugateGradientOptimizer,
// PerlmutterHvp, DiagonalGaussian):
//   k_loss_grad  -- surrogate loss + flat gradient          (f_loss / f_grad)
//   k_fvp        -- Hessian(mean_kl) . v  (Gauss-Newton form, exact at theta_old; derivation in DESIGN.md)
//   k_loss_kl    -- surrogate loss + mean KL at a trial theta (f_loss_constraint)
//   k_finalize   -- fixed-order (deterministic) float64 reduction of the per-block partial rows
// and of the VPG update (algos/vpg.py:88): k_loss_grad<PT, OP_VPG> (surr_obj = -mean(logli * adv), no likelihood ratio) and k_finalize<true, false>,
// whose blocks apply one TF-Adam step to the columns they reduced (run_vpg_update); and of the PPO update (algos/ppo.py:107-119):
// k_loss_grad<PT, OP_PPO> (the clipped head) and k_finalize<.., true> (the entropy bonus on the reduced vector, then the same step), n_epochs times (run_ppo_update).
//
// Generic VALU formulation: a block of PT threads owns tiles of PT samples.  Phase A is thread-per-
// sample (forward / tangent / back-prop in LDS columns, weights via scalar loads); phase B is
// thread-per-parameter (weight-gradient outer products over the tile, rows padded to PT+1 floats so
// that lanes holding different units hit different LDS banks).  Each block accumulates into its own
// row of a global partial buffer; k_finalize sums rows in block order -> bitwise reproducible.
#include "device_common.h"
#ifdef FIN_TIMING
__device__ unsigned long long g_fin_phase[512][8];
#define CG_MARK(i) { if (threadIdx.x == 0 && blockIdx.x < 512) g_fin_phase[blockIdx.x][i] = __builtin_readcyclecounter(); }
#endif
#include "cg_device.h"



// offsets (in rows) of the per-layer activation buffers h_0 (= input) .. h_{L-1}; h_L (mean) lives in DM
__device__ __forceinline__ int hrow(const NetDesc& net, int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += net.dims[i];
    return o;
}

// forward pass storing every layer input; returns nothing, mean is written to DM rows [0,na)
template <int PT>
__device__ __forceinline__ void forward_store(const NetDesc& net, const float* __restrict__ th, float* H, float* DM, int tid) {
    constexpr int PLD = PT + 1;
    for (int l = 0; l < net.n_layers; ++l) {
        float* dst = (l == net.n_layers - 1) ? DM : (H + hrow(net, l + 1) * PLD);
        dense_col(th + net.w_off[l], th + net.b_off[l], net.dims[l], net.dims[l + 1], net.act[l], H + hrow(net, l) * PLD,
                  dst, PLD, tid);
    }
}

template <int PT>
__device__ __forceinline__ bool load_obs_tile(const PolK& k, int ns, long long base, float* H, int tid) {
    constexpr int PLD = PT + 1;
    const long long n = base + tid;
    const bool ok = (n < k.N) && (k.valid == nullptr || k.valid[n]);
    for (int i = 0; i < ns; ++i) H[i * PLD + tid] = (n < k.N) ? k.obs[n * ns + i] : 0.0f;
    return ok;
}

// Phase B for one layer: part[w_off + i*n_out + j] += sum_n h_l[i][n] * d[j][n];  part[b_off + j] += sum_n d[j][n]
template <int PT>
__device__ __forceinline__ void accum_layer(const NetDesc& net, int l, const float* Hl, const float* D, float* part, int tid) {
    constexpr int PLD = PT + 1;
    const int n_in = net.dims[l], n_out = net.dims[l + 1];
    for (int p = tid; p < n_in * n_out; p += PT) {
        const int i = p / n_out, j = p - i * n_out;
        const float* hr = Hl + i * PLD;
        const float* dr = D + j * PLD;
        float s = 0.0f;
#pragma unroll 8
        for (int n = 0; n < PT; ++n) s = fmaf(hr[n], dr[n], s);
        part[net.w_off[l] + p] += s;
    }
    for (int j = tid; j < n_out; j += PT) {
        const float* dr = D + j * PLD;
        float s = 0.0f;
#pragma unroll 8
        for (int n = 0; n < PT; ++n) s += dr[n];
        part[net.b_off[l] + j] += s;
    }
}

// delta_l[i] = (sum_j W_l[i][j] * delta_{l+1}[j]) * (1 - h_l[i]^2), written in place over h_l (tanh hidden layers)
template <int PT>
__device__ __forceinline__ void backprop_layer(const NetDesc& net, int l, const float* __restrict__ th, float* Hl, const float* D, int tid) {
    constexpr int PLD = PT + 1;
    const int n_in = net.dims[l], n_out = net.dims[l + 1];
    const float* __restrict__ W = th + net.w_off[l];
    for (int i = 0; i < n_in; ++i) {
        float s = 0.0f;
        const float* __restrict__ wr = W + (size_t)i * n_out;
        for (int j = 0; j < n_out; ++j) s = fmaf(wr[j], D[j * PLD + tid], s);
        const float h = Hl[i * PLD + tid];
        Hl[i * PLD + tid] = s * (1.0f - h * h);
    }
}

// shared tail of grad and fvp: DM holds d(objective)/d(mean) per sample (already scaled, zero if invalid)
template <int PT>
__device__ __forceinline__ void backward_accumulate(const NetDesc& net, const float* __restrict__ th, float* H, float* DM, float* part, int tid) {
    constexpr int PLD = PT + 1;
    const float* D = DM;
    for (int l = net.n_layers - 1; l >= 0; --l) {
        float* Hl = H + hrow(net, l) * PLD;
        __syncthreads();
        accum_layer<PT>(net, l, Hl, D, part, tid);
        __syncthreads();
        if (l > 0) { backprop_layer<PT>(net, l, th, Hl, D, tid); D = Hl; }
    }
}

// partial row layout: [0, P) gradient in theta order (log_std slots at pol.n_params..P), then
//   [P] = loss (or kl-side scalar), [P+1] = second scalar, [P+2] = valid-sample weight (count*inv_n)
#define PART_EXTRA 3

// VPG: the VPG surrogate (vpg.py:88) instead of NPO's: loss = -mean(logli * adv) with logli = DiagonalGaussian.log_likelihood_sym(act; mean,
// log_std) = -sum(ls) - 0.5 sum(z^2) - 0.5 na log(2 pi); its gradient is NPO's at ratio 1 (la = adv).  old_mean / old_log_std are not read.
// PPO (HEAD = OP_PPO): NPO's ratio through ppo_gate (ppo.py:112-117); block 0 leaves the entropy of the entry theta in column P+1 (ppo_entropy_term).
// HEAD = OP_GRAD and OP_VPG compile to the code k_loss_grad<PT, OP_GRAD> and <PT, true> had (only the template argument's type changed with the third head).
// PPOKL (HEAD = OP_PPOKL): PPO plus the KL penalty's seed and loss term (ppo.py:120-121; ppo_kl_open / ppo_kl_dim) under the gate read from PolK::mean_kl.
template <int PT, int HEAD>
__global__ void __launch_bounds__(PT) k_loss_grad(ProblemDesc pd, PolK k, const float* __restrict__ theta, float* __restrict__ partials) {
    constexpr bool VPG = (HEAD == OP_VPG), PPOKL = (HEAD == OP_PPOKL), PPO = (HEAD == OP_PPO) || PPOKL;
    constexpr int PLD = PT + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[16];
    const NetDesc& net = pd.pol;
    const int tid = threadIdx.x, ns = pd.ns, na = pd.na, P = pd.P;
    int hrows = 0;
    for (int l = 0; l < net.n_layers; ++l) hrows += net.dims[l];
    float* H = lds;
    float* DM = H + hrows * PLD;
    float* part = partials + (size_t)blockIdx.x * (P + PART_EXTRA);
    for (int p = tid; p < P + PART_EXTRA; p += PT) part[p] = 0.0f;
    const float* __restrict__ raw_ls = theta + net.n_params;
    double loss_acc = 0.0;
    float dls_acc[32];            // na <= 32 enforced by the launcher
#pragma unroll
    for (int d = 0; d < 32; ++d) dls_acc[d] = 0.0f;
    bool kl_open = false;                                        // the penalty's gate: the same for every thread of the launch
    if constexpr (PPOKL) kl_open = ppo_kl_open(k.mean_kl, k.kl_delta);
    const float kl_w = PPOKL ? k.kl_beta * k.inv_n : 0.0f;
    for (long long base = (long long)blockIdx.x * PT; base < k.N; base += (long long)gridDim.x * PT) {
        __syncthreads();
        const bool ok = load_obs_tile<PT>(k, ns, base, H, tid);
        forward_store<PT>(net, theta, H, DM, tid);
        const long long n = base + tid;
        if (k.gm != nullptr) {                                  // VJP mode (bptt.hip): d objective / d mean supplied
            for (int d = 0; d < na; ++d) DM[d * PLD + tid] = ok ? k.gm[n * na + d] : 0.0f;
            backward_accumulate<PT>(net, theta, H, DM, part, tid);
            continue;
        }
        float w = 0.0f;
        if (ok && VPG) {
            float logli = -(float)na * HALF_LOG_2PI;             // DiagonalGaussian.log_likelihood_sym
            for (int d = 0; d < na; ++d) {
                const float ls = fmaxf(raw_ls[d], LOG_MIN_STD);
                const float z = (k.act[n * na + d] - DM[d * PLD + tid]) * expf(-ls);
                logli -= ls + 0.5f * z * z;
            }
            const float la = k.adv[n];                           // ratio 1: d(logli * adv) = adv * d logli
            loss_acc -= (double)logli * (double)la * (double)k.inv_n;      // surr_obj = -mean(logli * adv) (vpg.py:88)
            w = -la * k.inv_n;
        } else if (ok) {
            float llr = 0.0f;                                   // logli_new - logli_old
            for (int d = 0; d < na; ++d) {
                const float ls = fmaxf(raw_ls[d], LOG_MIN_STD), ols = k.old_ls[(size_t)n * k.ls_stride + d];
                const float a = k.act[n * na + d];
                const float z = (a - DM[d * PLD + tid]) * expf(-ls);
                const float zo = (a - k.old_mean[n * na + d]) * expf(-ols);
                llr += (ols - ls) + 0.5f * (zo * zo - z * z);
            }
            const float lr = expf(llr);                          // likelihood_ratio_sym (npo.py:69)
            if constexpr (PPO) {
                float surr;
                const float la = ppo_gate(lr, k.adv[n], k.clip_lo, k.clip_hi, &surr);
                loss_acc -= (double)surr * (double)k.inv_n;      // clipped_surr_loss (ppo.py:115-117)
                w = -la * k.inv_n;
            } else {
                const float la = lr * k.adv[n];
                loss_acc -= (double)la * (double)k.inv_n;        // surr_loss = -mean(lr*adv) (npo.py:75)
                w = -la * k.inv_n;
            }
        }
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            if (d < na) {
                const float ls = fmaxf(raw_ls[d], LOG_MIN_STD);
                const float inv_std = expf(-ls);
                const float z = ok ? (k.act[n * na + d] - DM[d * PLD + tid]) * inv_std : 0.0f;
                float kmu = 0.0f, kls = 0.0f;
                if constexpr (PPOKL) {
                    if (kl_open && ok) {                         // the KL seed (a clipped sample carries it too); DM still holds the mean here
                        const float ols = k.old_ls[(size_t)n * k.ls_stride + d];
                        loss_acc += (double)(kl_w * ppo_kl_dim(DM[d * PLD + tid], k.old_mean[n * na + d], ls, ols, expf(2.0f * ols), inv_std, &kmu, &kls));
                    }
                }
                DM[d * PLD + tid] = w * z * inv_std;             // d loss / d mean
                dls_acc[d] += w * (z * z - 1.0f);                // d loss / d log_std
                if constexpr (PPOKL) {                           // + kl_penalty / N * d kl_i, in statements of their own: with the gate closed the arithmetic is OP_PPO's
                    if (kl_open && ok) { DM[d * PLD + tid] += kl_w * kmu; dls_acc[d] += kl_w * kls; }
                }
            }
        }
        if constexpr (PPOKL) { if (kl_open && ok) loss_acc -= (double)kl_w * k.kl_delta; }      // sum_i kl_penalty / N (kl_i - step_size) = kl_penalty (mean_kl - step_size)
        backward_accumulate<PT>(net, theta, H, DM, part, tid);
    }
    // block-reduce the per-thread scalars into the partial row
    const double l = block_sum(loss_acc, red);
    if (tid == 0) part[P] = (float)l;
    for (int d = 0; d < na; ++d) {
        const double s = block_sum((double)dls_acc[d], red);
        if (tid == 0) part[net.n_params + d] = (raw_ls[d] > LOG_MIN_STD) ? (float)s : 0.0f;
    }
    if (PPO && blockIdx.x == 0 && tid == 0) {
        float h = (float)na * ENTROPY_CONST;                     // DiagonalGaussian.entropy_sym (ppo.py:109) of the theta this launch read
        for (int d = 0; d < na; ++d) h += fmaxf(raw_ls[d], LOG_MIN_STD);
        part[P + 1] = h;
    }
}

// tangent forward: dpre_{l+1} = dh_l W_l + h_l V_l + vb_l ; dh_{l+1} = dpre * (1 - h_{l+1}^2)
template <int PT>
__device__ __forceinline__ void tangent_layer(const NetDesc& net, int l, const float* __restrict__ th, const float* __restrict__ v,
                                              const float* Hl, const float* dHl /*nullptr for l==0*/, const float* Hn /* h_(l+1), or nullptr for the output layer */,
                                              float* dst, int tid) {
    constexpr int PLD = PT + 1;
    const int n_in = net.dims[l], n_out = net.dims[l + 1];
    const float* __restrict__ W = th + net.w_off[l];
    const float* __restrict__ V = v + net.w_off[l];
    const float* __restrict__ vb = v + net.b_off[l];
    for (int j0 = 0; j0 < n_out; j0 += DENSE_JB) {
        float acc[DENSE_JB];
        const int nj = min(DENSE_JB, n_out - j0);
#pragma unroll
        for (int jj = 0; jj < DENSE_JB; ++jj) acc[jj] = (jj < nj) ? vb[j0 + jj] : 0.0f;
        for (int i = 0; i < n_in; ++i) {
            const float h = Hl[i * PLD + tid];
            const float dh = (dHl != nullptr) ? dHl[i * PLD + tid] : 0.0f;
#pragma unroll
            for (int jj = 0; jj < DENSE_JB; ++jj)
                if (jj < nj) acc[jj] = fmaf(h, V[(size_t)i * n_out + j0 + jj], fmaf(dh, W[(size_t)i * n_out + j0 + jj], acc[jj]));
        }
#pragma unroll
        for (int jj = 0; jj < DENSE_JB; ++jj)
            if (jj < nj) {
                float o = acc[jj];
                if (Hn != nullptr) { const float hn = Hn[(j0 + jj) * PLD + tid]; o *= (1.0f - hn * hn); }
                dst[(j0 + jj) * PLD + tid] = o;
            }
    }
}

template <int PT>
__global__ void __launch_bounds__(PT) k_fvp(ProblemDesc pd, PolK k, const float* __restrict__ theta, const float* __restrict__ v,
                                            float* __restrict__ partials) {
    constexpr int PLD = PT + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[16];
    const NetDesc& net = pd.pol;
    const int tid = threadIdx.x, ns = pd.ns, na = pd.na, P = pd.P, L = net.n_layers;
    int hrows = 0;
    for (int l = 0; l < L; ++l) hrows += net.dims[l];
    float* H = lds;                       // h_0..h_{L-1}
    float* DM = H + hrows * PLD;          // mean, then u
    float* dH = DM + na * PLD;            // tangents dh_1..dh_{L-1}, indexed with hrow(l) - dims[0]
    float* part = partials + (size_t)blockIdx.x * (P + PART_EXTRA);
    for (int p = tid; p < P + PART_EXTRA; p += PT) part[p] = 0.0f;
    const float* __restrict__ raw_ls = theta + net.n_params;
    double wsum = 0.0;
    for (long long base = (long long)blockIdx.x * PT; base < k.N; base += (long long)gridDim.x * PT) {
        __syncthreads();
        const bool ok = load_obs_tile<PT>(k, ns, base, H, tid);
        forward_store<PT>(net, theta, H, DM, tid);
        for (int l = 0; l < L; ++l) {
            const float* Hl = H + hrow(net, l) * PLD;
            const float* dHl = (l == 0) ? nullptr : dH + (hrow(net, l) - net.dims[0]) * PLD;
            const float* Hn = (l == L - 1) ? nullptr : H + hrow(net, l + 1) * PLD;
            float* dst = (l == L - 1) ? DM : dH + (hrow(net, l + 1) - net.dims[0]) * PLD;
            tangent_layer<PT>(net, l, theta, v, Hl, dHl, Hn, dst, tid);
        }
        for (int d = 0; d < na; ++d) {
            const float ls = fmaxf(raw_ls[d], LOG_MIN_STD);
            const float s2 = expf(2.0f * ls);
            // d2 KL / d mean^2 = 2 / (2 s^2 + eps) = 1 / (s^2 + eps/2)
            DM[d * PLD + tid] = ok ? DM[d * PLD + tid] / (s2 + 0.5f * KL_EPS) * k.inv_n : 0.0f;
        }
        if (ok) wsum += (double)k.inv_n;
        backward_accumulate<PT>(net, theta, H, DM, part, tid);
    }
    const double wtot = block_sum(wsum, red);
    if (tid == 0) part[P + 2] = (float)wtot;
}

template <int PT>
__global__ void __launch_bounds__(PT) k_loss_kl(ProblemDesc pd, PolK k, const float* __restrict__ theta, float* __restrict__ partials) {
    constexpr int PLD = PT + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[16];
    if (k.skip != nullptr && k.skip[0] >= 0.0) return;        // speculative line-search trial after the search stopped
    const NetDesc& net = pd.pol;
    const int tid = threadIdx.x, ns = pd.ns, na = pd.na;
    float* S = lds;
    float* A = S + ns * PLD;
    float* Bq = A + net.max_width * PLD;
    const float* __restrict__ raw_ls = theta + net.n_params;
    double loss_acc = 0.0, kl_acc = 0.0;
    for (long long base = (long long)blockIdx.x * PT; base < k.N; base += (long long)gridDim.x * PT) {
        const bool ok = load_obs_tile<PT>(k, ns, base, S, tid);
        const float* m = mlp_col(net, theta, S, A, Bq, PLD, tid);
        if (ok) {
            const long long n = base + tid;
            float llr = 0.0f, kl = 0.0f;
            for (int d = 0; d < na; ++d) {
                const float ls = fmaxf(raw_ls[d], LOG_MIN_STD), ols = k.old_ls[(size_t)n * k.ls_stride + d];
                const float mu = m[d * PLD + tid], omu = k.old_mean[n * na + d], a = k.act[n * na + d];
                const float z = (a - mu) * expf(-ls), zo = (a - omu) * expf(-ols);
                llr += (ols - ls) + 0.5f * (zo * zo - z * z);
                const float s2 = expf(2.0f * ls), os2 = expf(2.0f * ols);
                const float dm = omu - mu;
                kl += (dm * dm + os2 - s2) / (2.0f * s2 + KL_EPS) + ls - ols;      // DiagonalGaussian.kl_sym
            }
            loss_acc -= (double)(expf(llr) * k.adv[n]) * (double)k.inv_n;
            kl_acc += (double)kl * (double)k.inv_n;
        }
    }
    const double l = block_sum(loss_acc, red);
    const double q = block_sum(kl_acc, red);
    if (tid == 0) { partials[blockIdx.x * 2] = (float)l; partials[blockIdx.x * 2 + 1] = (float)q; }
}

// out[p] = sum over partial rows (fixed order) of column col(p), float64.
// mode 0: grad -> out[0] = loss (column P), out[1+p] = g[p]
// mode 1: fvp  -> out[p] = Hv[p] for the mean net; log_std rows get c(s) * v_ls * weight (column P+2)
// mode 2: loss/kl -> out[0], out[1] from columns (lk_col, lk_col+1)
#define FIN_C 32
#ifdef FIN_TIMING      // developer instrumentation (SRC=policy_update.hip tools/build_variant.sh ftiming -DFIN_TIMING; tools/fin_phases.py)
#define FT_MARK(i) { if (threadIdx.x == 0 && tail.op == 1 && blockIdx.x < 512) g_fin_phase[blockIdx.x][i] = __builtin_readcyclecounter(); }
extern "C" int32_t metrpo_debug_fin_phases(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_phase), sizeof(unsigned long long) * 4096) == hipSuccess ? 0 : -1; }
#else
#define FT_MARK(i)
#endif
// k_finalize<true, ..> (run_vpg_update, run_ppo_update; mode 0): every block applies TF-Adam (tf_adam_elem) to the theta elements of the columns it has just reduced --
// after adding the ranks' shares in a sharded run (each block pulls exactly the columns it pushed; no other workgroup reads them, so no arrival ticket).
// A template variant, so that the TRPO reductions (k_finalize<false, false>) compile to the code they had before.
struct AdamTail {
    float* theta; float* m; float* v;           // the ctx policy and its Adam moments (metrpo_ctx::d_pol_adam)
    float lr_t, b1, b2, eps;                    // lr_t: the bias-corrected step size of this step (launch_policy_adam's)
    double* loss;                               // non-NULL: the reduced loss (column 0) is also stored here
    double ent_coeff;                           // k_finalize<.., true> / k_ppo_step: PPO's entropy_bonus_coeff (last: the other members keep their offsets)
};
// PPO's entropy bonus on the reduced [loss | gradient] vector (ppo.py:109, 119: - entropy_bonus_coeff * mean(entropy_sym)).  The entropy of a
// state-independent log_std is the same for every sample, so the term is per parameter: -coeff on every unclamped log_std slot, and -coeff * H on
// the loss, H as the gradient kernel's block 0 left it in column P+1 of partial row 0.  (Not recomputed from theta here: under ADAM other
// workgroups of this launch are stepping the log_std slots.)  Added once, AFTER the ranks' shares are summed.
__device__ __forceinline__ double ppo_entropy_term(const ProblemDesc& pd, int p, const float* __restrict__ partials, const float* __restrict__ theta, double coeff) {
    if (p == 0) return -coeff * (double)partials[pd.P + 1];
    return (p - 1 >= pd.pol.n_params && theta[p - 1] > LOG_MIN_STD) ? -coeff : 0.0;
}
// ENT (mode 0 only): ppo_entropy_term with AdamTail::ent_coeff is added to each reduced element before it is stored / stepped.  k_finalize<false, false>
// and <true, false> compile to the code k_finalize<false> and <true> had.
template <bool ADAM, bool ENT>
__global__ void __launch_bounds__(1024) k_finalize(ProblemDesc pd, int mode, int nrows, int stride, int lk_col,
                                                   const float* __restrict__ partials, const float* __restrict__ theta,
                                                   const double* __restrict__ v, double* __restrict__ out, CgTail tail, XchgK xc, AdamTail ad) {
    // block = FIN_C output columns x (1024 / FIN_C) row slices (latency-bound sum: many small blocks); slice s adds rows
    // s, s+NSL, ... and the slice sums are added in slice order: deterministic.  32 columns = one 128-byte line per row read.
    constexpr int NSL = 1024 / FIN_C;
    __shared__ double sh[NSL][FIN_C + 1];
    if (tail.op == 4 && tail.ls[0] >= 0.0) {                  // speculative line-search trial after the search stopped (every block reads the same cell)
        // a sharded run keeps its exchanges in step: the slot protocol (xchg_device.h) counts on every sequence number being used by every rank
        if (xc.world > 1 && blockIdx.x == 0 && threadIdx.x < 2) { xchg_push(xc, (int)threadIdx.x, 0.0); (void)xchg_pull_sum(xc, (int)threadIdx.x); }
        if (tail.pub_dst != nullptr && blockIdx.x == 0) ls_publish(tail.scal, tail.pub_dst, tail.pub_stamp);      // the search's outcome still has to reach the host
        return;
    }
    FT_MARK(0)
    CgPre pre;
    cg_prefetch(tail, pre);                 // every block (nobody knows yet who arrives last); these vectors are not written by this launch
    const int P = pd.P;
    const int nout = (mode == 0) ? P + 1 : (mode == 1) ? P : 2;
    const int lc = threadIdx.x % FIN_C, sl = threadIdx.x / FIN_C;
    const int p = blockIdx.x * FIN_C + lc;
    int col = p;
    if (mode == 0) col = (p == 0) ? P : p - 1;
    if (mode == 2) col = lk_col + p;
    const bool lsrow = (mode == 1 && p >= pd.pol.n_params && p < nout);
    if (lsrow) col = P + 2;                                   // valid-sample weight column
    double a = 0.0;
    if (p < nout) {
        int b = sl;
        for (; b + 3 * NSL < nrows; b += 4 * NSL) {             // four independent loads in flight per thread
            const float v0 = partials[(size_t)b * stride + col], v1 = partials[(size_t)(b + NSL) * stride + col];
            const float v2 = partials[(size_t)(b + 2 * NSL) * stride + col], v3 = partials[(size_t)(b + 3 * NSL) * stride + col];
            a += (double)v0; a += (double)v1; a += (double)v2; a += (double)v3;
        }
        for (; b < nrows; b += NSL) a += (double)partials[(size_t)b * stride + col];
    }
    FT_MARK(1)
    sh[sl][lc] = a;
    __syncthreads();
    if (sl == 0 && p < nout) {
        double t = 0.0;
        for (int w = 0; w < NSL; ++w) t += sh[w][lc];
        if (lsrow) {
            // Hessian of mean KL w.r.t. log_std at theta_old: 4 s^2 (2 s^2 - eps) / (2 s^2 + eps)^2  (-> 2 as eps -> 0)
            const double raw = (double)theta[p];
            const double s2 = exp(2.0 * fmax(raw, (double)LOG_MIN_STD));
            const double c = 4.0 * s2 * (2.0 * s2 - 1e-8) / ((2.0 * s2 + 1e-8) * (2.0 * s2 + 1e-8));
            t = (raw > (double)LOG_MIN_STD) ? c * v[p] * t : 0.0;
        }
        if (ADAM) {
            if (xc.world > 1) { xchg_push(xc, p, t); t = xchg_pull_sum(xc, p); }
            if (ENT) t += ppo_entropy_term(pd, p, partials, ad.theta, ad.ent_coeff);   // (ad.theta[p - 1] is this thread's own element, stepped below)
            out[p] = t;
            if (p == 0) { if (ad.loss != nullptr) *ad.loss = t; }
            else tf_adam_elem((float)t, ad.theta, ad.m, ad.v, p - 1, ad.lr_t, ad.b1, ad.b2, ad.eps);
            return;
        }
        // a fused tail reads `out` in ANOTHER workgroup (the last to arrive): write-through (sc1) stores, drained before the arrival ticket, instead of a
        // cache-wide release per workgroup (buffer_wbl2 x 45 workgroups at C1, x 391 for the 100-50-25 policy: 25-49 us of that reduction).
        // This relies on gfx942 / gfx950 lowering a relaxed agent-scope atomic store to an sc1 write-through store (visible beyond this XCD's L2 once vmcnt
        // drains).  EVERYTHING the closing workgroup reads that another workgroup of this launch wrote must travel this way -- today exactly: `out` (here) and the
        // exchange packets (xchg_push: agent-scope stores).  theta, v, partials and the CG state are written by EARLIER launches.  A plain store added to that list
        // would be a silent stale read across XCDs: on any other target the build stops here instead of guessing.
#if !defined(__gfx942__) && !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "k_finalize's fence-free hand-over is written for gfx942 / gfx950 (sc1 write-through stores); other targets need fence(release, agent) before the ticket"
#endif
        if (ENT) t += ppo_entropy_term(pd, p, partials, theta, ad.ent_coeff);       // (launched without a tail and outside an exchange: launch_ppo_loss_grad)
        if (tail.op != 0 || xc.world > 1) __hip_atomic_store(out + p, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else out[p] = t;
        if (xc.world > 1) xchg_push(xc, p, t);                // sharded run: this rank's share goes straight into every rank's receive slot
    }
    if (ADAM || (tail.op == 0 && xc.world <= 1)) return;
    // ---- fused tail: the last block to arrive owns the complete `out` vector: it adds the ranks' shares (one-shot exchange,
    //      xchg_device.h; the packets of the other blocks have been under way since they were produced) and runs the CG vector step ----
    __shared__ unsigned int s_last;
    __shared__ double cgsh[16];
    FT_MARK(2)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    FT_MARK(3)
    if (threadIdx.x == 0) {
        const unsigned int tk = __hip_atomic_fetch_add(tail.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == gridDim.x - 1) ? 1u : 0u;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    FT_MARK(4)
    if (!s_last) return;
    if (xc.world > 1) {
        for (int i = threadIdx.x; i < nout; i += blockDim.x) out[i] = xchg_pull_sum(xc, i);
        __syncthreads();
    }
    if (tail.op != 0) cg_tail_run(tail, cgsh, &pre);
    if (threadIdx.x == 0) __hip_atomic_store(tail.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
}

__global__ void k_d2f(const double* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// ---------------------------------------------------------------------------------------------
static int ensure_partials(metrpo_ctx* c, int nrows) {
    const size_t need = (size_t)nrows * (c->pd.P + PART_EXTRA);
    return ws_grow(c, c->d_partials, need * sizeof(float));
}

// the descriptor of `op` on batch b at the context's theta, everything else off; validates what the operation reads
// (OP_FVP: no targets; OP_VPG: the VPG surrogate reads no old distribution -- d_old_mean / d_old_log_std may be NULL; OP_PPO: pr carries the clip; OP_PPOKL: and kp the penalty)
static int make_call(metrpo_ctx* c, UpdOp op, const metrpo_batch* b, UpdCall* u, const metrpo_ppo_params* pr = nullptr, const metrpo_ppo_kl_params* kp = nullptr) {
    const bool vpg = (op == OP_VPG), ppo = (op == OP_PPO || op == OP_PPOKL);
    if (!b || !b->d_obs) return set_err(c, METRPO_ENULL, "batch/d_obs is NULL");
    if (b->N <= 0) return set_err(c, METRPO_EINVAL, "batch N must be positive");
    if (c->pd.na > 32) return set_err(c, METRPO_EUNSUPPORTED, "na > 32");
    if (ppo) {
        if (!pr) return set_err(c, METRPO_ENULL, "ppo: params NULL");
        if (!b->d_old_mean || !b->d_old_log_std)
            return set_err(c, METRPO_EINVAL, "ppo: the PPO surrogate needs the old distribution (batch d_old_mean / d_old_log_std is NULL)");
        if (!(pr->clip_lr >= 0.0) || !std::isfinite(pr->entropy_bonus_coeff))
            return set_err(c, METRPO_EINVAL, "ppo: need clip_lr >= 0 and a finite entropy_bonus_coeff");
    }
    if (op == OP_PPOKL) {
        if (!kp) return set_err(c, METRPO_ENULL, "ppo_kl: KL penalty params NULL");
        if (!(kp->kl_penalty >= 0.0) || !std::isfinite(kp->kl_penalty) || !std::isfinite(kp->step_size))
            return set_err(c, METRPO_EINVAL, "ppo_kl: need a finite kl_penalty >= 0 and a finite step_size");
    }
    if (op != OP_FVP && (!b->d_act || !b->d_adv || (!vpg && (!b->d_old_mean || !b->d_old_log_std))))
        return set_err(c, METRPO_ENULL, "batch pointer is NULL");
    if ((vpg || ppo) && !(b->inv_n_global > 0.0)) return set_err(c, METRPO_EINVAL, "batch inv_n_global must be positive");
    *u = UpdCall{};
    u->op = op; u->theta = c->d_theta.p;
    PolK& k = u->k;
    k.obs = b->d_obs; k.act = b->d_act; k.adv = b->d_adv; k.old_mean = b->d_old_mean; k.old_ls = b->d_old_log_std;
    k.ls_stride = b->old_log_std_stride; k.valid = b->d_valid; k.N = b->N; k.inv_n = (float)b->inv_n_global;
    if (op == OP_PPOKL) { k.kl_beta = (float)kp->kl_penalty; k.kl_delta = kp->step_size; }      // (k.mean_kl: set by the caller, to where the reduced mean KL will be)
    if (ppo) { k.clip_lo = (float)(1.0 - pr->clip_lr); k.clip_hi = (float)(1.0 + pr->clip_lr); u->ent_coeff = pr->entropy_bonus_coeff; u->ent_in_reduction = true; }
    return METRPO_OK;
}

// partial rows of one launch in c->d_partials, as k_finalize reads them
struct PartRows { int rc, nrows, stride, lk_col; };

static void finalize(metrpo_ctx* c, const UpdCall& u, const PartRows& r, hipStream_t st) {
    const int mode = (u.op == OP_LOSSKL) ? 2 : (u.op == OP_FVP) ? 1 : 0;        // output layout: [loss | gradient], H v, [loss, kl]
    const int nout = (mode == 0) ? c->pd.P + 1 : (mode == 1) ? c->pd.P : 2;
    CgTail none; none.op = 0; none.ticket = c->d_ticket.p; none.vpos = nullptr; none.imgval = nullptr; none.ls = nullptr; none.pub_dst = nullptr;
    // inside a fused update of a sharded run the reduction carries the cross-rank sum in its tail
    const XchgK xc = (u.scope.exchange_in_tail && c->xg_world > 1) ? xchg_next(c) : xchg_none();
    const dim3 grid((nout + FIN_C - 1) / FIN_C);
    const bool ppo = (u.op == OP_PPO || u.op == OP_PPOKL);   // (the penalty is all in the gradient kernel: both reduce alike)
    if (ppo && u.adam)
        hipLaunchKernelGGL((k_finalize<true, true>), grid, dim3(1024), 0, st, c->pd, mode, r.nrows, r.stride, r.lk_col,
                           c->d_partials.p, c->d_theta.p, u.v64, u.out, none, xc, *u.adam);
    else if (ppo && u.ent_in_reduction) {
        AdamTail ent = {}; ent.ent_coeff = u.ent_coeff;
        hipLaunchKernelGGL((k_finalize<false, true>), grid, dim3(1024), 0, st, c->pd, mode, r.nrows, r.stride, r.lk_col,
                           c->d_partials.p, c->d_theta.p, u.v64, u.out, none, xc, ent);
    }
    else if (u.adam)
        hipLaunchKernelGGL((k_finalize<true, false>), dim3((nout + FIN_C - 1) / FIN_C), dim3(1024), 0, st, c->pd, mode, r.nrows, r.stride, r.lk_col,
                           c->d_partials.p, c->d_theta.p, u.v64, u.out, none, xc, *u.adam);
    else
        hipLaunchKernelGGL((k_finalize<false, false>), dim3((nout + FIN_C - 1) / FIN_C), dim3(1024), 0, st, c->pd, mode, r.nrows, r.stride, r.lk_col,
                           c->d_partials.p, c->d_theta.p, u.v64, u.out, u.tail ? *u.tail : none, xc, AdamTail{});
}

// generic kernels: pick the largest sample tile (threads per block) whose LDS columns fit
template <int PT>
static int launch_generic(metrpo_ctx* c, const UpdCall& u, int* nrows, hipStream_t st) {
    const NetDesc& net = c->pd.pol;
    const PolK& k = u.k;
    int hrows = 0; for (int l = 0; l < net.n_layers; ++l) hrows += net.dims[l];
    size_t rows = (u.op == OP_GRAD || u.op == OP_VPG || u.op == OP_PPO || u.op == OP_PPOKL) ? hrows + c->pd.na : (u.op == OP_FVP) ? hrows + c->pd.na + (hrows - net.dims[0])
                                                                         : (size_t)c->pd.ns + 2 * net.max_width;
    const size_t sh = rows * (PT + 1) * sizeof(float);
    if (sh > 160 * 1024) return METRPO_EUNSUPPORTED;
    const long long tiles = (k.N + PT - 1) / PT;
    const int g = (int)std::max<long long>(1, std::min<long long>(tiles, (long long)c->n_sm * 2));
    int rc = ensure_partials(c, g); if (rc) return rc;
    *nrows = g;
    c->upd_last = {0, (int)u.op, -1, PT, g, 0, 0};
    if (u.op == OP_GRAD) {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_loss_grad<PT, OP_GRAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL((k_loss_grad<PT, OP_GRAD>), dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, c->d_partials.p);
    } else if (u.op == OP_VPG) {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_loss_grad<PT, OP_VPG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL((k_loss_grad<PT, OP_VPG>), dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, c->d_partials.p);
    } else if (u.op == OP_PPO) {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_loss_grad<PT, OP_PPO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL((k_loss_grad<PT, OP_PPO>), dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, c->d_partials.p);
    } else if (u.op == OP_PPOKL) {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_loss_grad<PT, OP_PPOKL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL((k_loss_grad<PT, OP_PPOKL>), dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, c->d_partials.p);
    } else if (u.op == OP_FVP) {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_fvp<PT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL(k_fvp<PT>, dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, u.vf, c->d_partials.p);
    } else {
        if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)k_loss_kl<PT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL(k_loss_kl<PT>, dim3(g), dim3(PT), sh, st, c->pd, k, u.theta, c->d_partials.p);
    }
    return METRPO_OK;
}

// runs u on the fastest fused or generic family; on return the partial rows are in c->d_partials
static PartRows run_mode(metrpo_ctx* c, const UpdCall& u, hipStream_t st) {
    const int P = c->pd.P;
    const long long tiles = (u.k.N + 15) / 16;
    PartRows r = {METRPO_OK, 0, P + PART_EXTRA, P};
    const bool mfma = c->pol_mfma >= 0;
    if (mfma || f3_active(c, u.k.gm != nullptr)) {
        // policy_mfma.hip: one 8-wave block per CU = 2 waves per SIMD (measured in round 1: 2 and 3 waves per SIMD run at the same speed, 1 and 4
        // are slower) and only n_sm partial rows for k_finalize
        // (the loss + KL evaluation of the line search needs no transpose tiles and half the registers: two blocks per CU)
        // small batches (the params files' N = 50 000 - 60 000: 1.5 tiles per wave on a full grid): fewer, fuller blocks -- a launch's fixed cost does not
        // shrink with the tile count, but k_finalize reads one partial row per block (upd_tiles_per_wave, api.hip)
        // policy_fused3.hip: one block per CU; the back-prop kernel runs 4 waves per block (one per SIMD, 272 accumulator registers each), the
        // forward / tangent kernels 8; all write the same `nrows` partial rows
        const long long per_block = (mfma ? 8ll : 4ll) * std::max(1, c->upd_tiles_per_wave);
        const long long max_blocks = (long long)c->n_sm * ((mfma && u.op == OP_LOSSKL) ? 2 : 1);
        r.nrows = (int)std::max<long long>(1, std::min<long long>((tiles + per_block - 1) / per_block, max_blocks));
        const bool fvpc = mfma && u.scope.cache_activations && u.op == OP_FVP && u.k.gm == nullptr;       // (policy_mfma_launch's choice)
        c->upd_last = {mfma ? 1 : 3, fvpc ? (int)OP_FVPC : (int)u.op, mfma ? c->pol_mfma : -1, 0, r.nrows, 0, 0};
        if (!(r.rc = ensure_partials(c, r.nrows)))
            r.rc = mfma ? policy_mfma_launch(c, u, c->d_partials.p, r.nrows, st) : policy_f3_launch(c, u, c->d_partials.p, r.nrows, st);
        return r;
    }
    r.stride = (u.op == OP_LOSSKL) ? 2 : P + PART_EXTRA; r.lk_col = 0;
    r.rc = launch_generic<128>(c, u, &r.nrows, st);
    if (r.rc == METRPO_EUNSUPPORTED) r.rc = launch_generic<64>(c, u, &r.nrows, st);
    if (r.rc == METRPO_EUNSUPPORTED) r.rc = launch_generic<32>(c, u, &r.nrows, st);
    if (r.rc == METRPO_EUNSUPPORTED) r.rc = set_err(c, r.rc, "policy too wide for the update kernels' LDS tile");
    return r;
}

// One update launch: pick the family, launch, reduce into u.out (+ the step u.tail / u.adam describes, in the reduction's tail).
// The GEMM path (policy_gemm.hip) has its own reduction: it runs u.tail as a kernel of its own and cannot carry an accept test or an Adam step.
static int run_update(metrpo_ctx* c, const UpdCall& u, hipStream_t st) {
    if (policy_gemm_applicable(c, u.k.N, u.k.gm != nullptr)) {
        if (u.op == OP_LOSSKL && u.tail) return set_err(c, METRPO_EUNSUPPORTED, "device-side line search: not on the GEMM update path");
        return policy_gemm_run(c, u, st);
    }
    const bool timed = u.op == OP_FVP && ctx_opt(c, OPT_TIME_FVP) != nullptr && c->fvp_ev_n + 2 <= 32;      // diagnostics: metrpo_debug_fvp_us
    if (timed) {
        for (; c->fvp_ev_made < 32; ++c->fvp_ev_made) HIP_TRY(c, hipEventCreate(&c->fvp_ev[c->fvp_ev_made]));
        HIP_TRY(c, hipEventRecord(c->fvp_ev[c->fvp_ev_n], st));
    }
    const PartRows r = run_mode(c, u, st);
    if (r.rc) return r.rc;
    if (timed) { HIP_TRY(c, hipEventRecord(c->fvp_ev[c->fvp_ev_n + 1], st)); c->fvp_ev_n += 2; }
    finalize(c, u, r, st);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int launch_loss_grad(metrpo_ctx* c, const metrpo_batch* b, double* out, hipStream_t st, const CgTail* tail, SolveScope scope) {
    UpdCall u; int rc = make_call(c, OP_GRAD, b, &u); if (rc) return rc;
    u.out = out; u.tail = tail; u.scope = scope;
    return run_update(c, u, st);
}

// sum_n J_policy(obs_n)^T gm_n -> out[1 .. P] (out[0] = 0): the gradient kernels with the mean-adjoint supplied (bptt.hip)
int launch_policy_vjp(metrpo_ctx* c, const float* obs, const float* gm, long long N, double* out, hipStream_t st) {
    if (!obs || !gm || !out) return set_err(c, METRPO_ENULL, "policy_vjp: NULL pointer");
    if (c->pd.na > 32) return set_err(c, METRPO_EUNSUPPORTED, "na > 32");
    UpdCall u = {};
    u.op = OP_GRAD; u.theta = c->d_theta.p; u.out = out;
    u.k.obs = obs; u.k.N = N; u.k.inv_n = 1.0f; u.k.gm = gm;
    return run_update(c, u, st);
}

int launch_fvp(metrpo_ctx* c, const metrpo_batch* b, const double* v, double* hv, hipStream_t st) {
    if (!v || !hv) return set_err(c, METRPO_ENULL, "v/hv is NULL");
    const int P = c->pd.P;
    hipLaunchKernelGGL(k_d2f, dim3((P + 127) / 128), dim3(128), 0, st, v, c->d_vf.p, P);
    return launch_fvp_tail(c, b, c->d_vf.p, v, hv, nullptr, st);
}

int launch_fvp_tail(metrpo_ctx* c, const metrpo_batch* b, const float* vf, const double* v, double* hv, const CgTail* tail, hipStream_t st, SolveScope scope) {
    UpdCall u; int rc = make_call(c, OP_FVP, b, &u); if (rc) return rc;
    u.vf = vf; u.v64 = v; u.out = hv; u.tail = tail; u.scope = scope;
    return run_update(c, u, st);
}

int launch_loss_kl(metrpo_ctx* c, const metrpo_batch* b, const float* theta, double* out, hipStream_t st, const CgTail* decide, SolveScope scope) {
    UpdCall u; int rc = make_call(c, OP_LOSSKL, b, &u); if (rc) return rc;
    if (theta) u.theta = theta;
    if (decide) u.k.skip = decide->ls;
    u.out = out; u.tail = decide; u.scope = scope;
    return run_update(c, u, st);
}

// ---- 'vpg' (algos/vpg.py; FirstOrderOptimizer with batch_size=None, max_epochs=1: one Adam step on the whole batch's gradient) ----
int launch_vpg_loss_grad(metrpo_ctx* c, const metrpo_batch* b, double* out, hipStream_t st) {
    UpdCall u; int rc = make_call(c, OP_VPG, b, &u); if (rc) return rc;
    u.out = out;
    return run_update(c, u, st);
}

// k_finalize<true, false>'s step as a launch of its own: behind an all-reduce that k_finalize cannot carry (RCCL, a gradient longer than an exchange slot)
// and behind the GEMM path's own reduction.  gout = [loss | gradient], summed over the ranks.
__global__ void k_vpg_adam(const double* __restrict__ gout, int P, AdamTail ad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && ad.loss != nullptr) *ad.loss = gout[0];
    if (i < P) tf_adam_elem((float)gout[1 + i], ad.theta, ad.m, ad.v, i, ad.lr_t, ad.b1, ad.b2, ad.eps);
}

int run_vpg_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_vpg_params* pr, double* d_loss, hipStream_t st) {
    const int P = c->pd.P;
    if (!pr) return set_err(c, METRPO_ENULL, "vpg_update: params NULL");
    if (!(pr->lr >= 0.0) || !(pr->beta1 >= 0.0 && pr->beta1 < 1.0) || !(pr->beta2 >= 0.0 && pr->beta2 < 1.0) || !(pr->eps >= 0.0))
        return set_err(c, METRPO_EINVAL, "vpg_update: need lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0");
    UpdCall u; int rc = make_call(c, OP_VPG, b, &u); if (rc) return rc;
    if ((rc = ensure_policy_adam(c))) return rc;
    // TF's bias correction folded into the step size, exactly as launch_policy_adam (bptt.hip) computes it
    const int t1 = c->pol_adam_t + 1;
    const double lr_t = pr->lr * std::sqrt(1.0 - std::pow(pr->beta2, (double)t1)) / (1.0 - std::pow(pr->beta1, (double)t1));
    float* am = (float*)c->d_pol_adam.p;
    const AdamTail ad = {c->d_theta.p, am, am + P, (float)lr_t, (float)pr->beta1, (float)pr->beta2, (float)pr->eps, d_loss};
    double* gout = c->d_cg.p;                               // [1 + P] of the CG workspace (no update is open across this call)
    // the step rides in the reduction's tail unless an all-reduce the reduction cannot carry has to sit between them
    const UpdFusion f = update_fusion(c, b->N, false);
    const bool fused = f.carries_next_step();
    u.out = gout; u.adam = fused ? &ad : nullptr; u.scope.exchange_in_tail = f.exchange_in_tail;
    if ((rc = run_update(c, u, st))) return rc;
    if (!fused) {
        if ((c->xg_world > 1 || c->nccl_comm) && (rc = comm_allreduce_f64(c, gout, P + 1, st))) return rc;
        hipLaunchKernelGGL(k_vpg_adam, dim3((P + 255) / 256), dim3(256), 0, st, (const double*)gout, P, ad);
    }
    HIP_TRY(c, hipGetLastError());
    c->pol_adam_t = t1;
    return METRPO_OK;
}

// ---- 'ppo' (algos/ppo.py:107-119; the optimiser ppo.py:61-62 names but never defines is stated in include/metrpo.h: full-batch TF-Adam epochs) ----
// The entropy term and (step) the Adam step on a reduced, rank-summed [loss | gradient] as ONE workgroup: behind the GEMM path's own reduction and behind an
// all-reduce k_finalize cannot carry.  One workgroup so that the entropy of the entry theta is read before any log_std slot is stepped.
__global__ void __launch_bounds__(1024) k_ppo_step(double* __restrict__ gout, int P, int n_params, int na, int step, AdamTail ad) {
    const double coeff = ad.ent_coeff;
    __shared__ float s_h;
    if (threadIdx.x == 0) {
        float h = (float)na * ENTROPY_CONST;                   // the gradient kernels' expression (OP_PPO, column P+1)
        for (int d = 0; d < na; ++d) h += fmaxf(ad.theta[n_params + d], LOG_MIN_STD);
        s_h = h;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P + 1; p += blockDim.x) {
        double t = gout[p];
        if (p == 0) t += -coeff * (double)s_h;
        else if (p - 1 >= n_params && ad.theta[p - 1] > LOG_MIN_STD) t += -coeff;
        gout[p] = t;
        if (p == 0) { if (ad.loss != nullptr) *ad.loss = t; }
        else if (step) tf_adam_elem((float)t, ad.theta, ad.m, ad.v, p - 1, ad.lr_t, ad.b1, ad.b2, ad.eps);
    }
}

int launch_ppo_loss_grad(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, double* out, hipStream_t st) {
    UpdCall u; int rc = make_call(c, OP_PPO, b, &u, pr); if (rc) return rc;
    u.out = out;
    if ((rc = run_update(c, u, st))) return rc;
    if (policy_gemm_applicable(c, b->N, false)) {            // (its own reduction: the entropy term follows as a launch)
        AdamTail ad = {}; ad.theta = c->d_theta.p; ad.ent_coeff = u.ent_coeff;
        hipLaunchKernelGGL(k_ppo_step, dim3(1), dim3(1024), 0, st, out, c->pd.P, c->pd.pol.n_params, c->pd.na, 0, ad);
        HIP_TRY(c, hipGetLastError());
    }
    return METRPO_OK;
}

// n_epochs x (gradient kernel + reduction with the entropy term and the Adam step in its tail); the old distribution is the batch's throughout, theta moves.
// Nothing here reads the device: the bias-corrected step sizes of all epochs are host arithmetic on the step count.
int run_ppo_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, int n_epochs, double* d_losses, hipStream_t st) {
    const int P = c->pd.P;
    if (!pr) return set_err(c, METRPO_ENULL, "ppo_update: params NULL");
    if (n_epochs < 0) return set_err(c, METRPO_EINVAL, "ppo_update: n_epochs must be >= 0");
    if (!(pr->lr >= 0.0) || !(pr->beta1 >= 0.0 && pr->beta1 < 1.0) || !(pr->beta2 >= 0.0 && pr->beta2 < 1.0) || !(pr->eps >= 0.0))
        return set_err(c, METRPO_EINVAL, "ppo_update: need lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0");
    UpdCall u; int rc = make_call(c, OP_PPO, b, &u, pr); if (rc) return rc;
    if ((rc = ensure_policy_adam(c))) return rc;
    float* am = (float*)c->d_pol_adam.p;
    double* gout = c->d_cg.p;                               // [1 + P] of the CG workspace (no update is open across this call)
    const UpdFusion f = update_fusion(c, b->N, false);      // as run_vpg_update: the ranks must agree on it
    const bool fused = f.carries_next_step();
    u.out = gout; u.scope.exchange_in_tail = f.exchange_in_tail;
    if (!fused) u.ent_in_reduction = false;                 // (the plain reduction k_finalize<false, false>: the stand-alone step adds the term, behind the ranks' sum)
    for (int e = 0; e < n_epochs; ++e) {
        const int t1 = c->pol_adam_t + 1;                   // launch_policy_adam's bias correction (bptt.hip)
        const double lr_t = pr->lr * std::sqrt(1.0 - std::pow(pr->beta2, (double)t1)) / (1.0 - std::pow(pr->beta1, (double)t1));
        const AdamTail ad = {c->d_theta.p, am, am + P, (float)lr_t, (float)pr->beta1, (float)pr->beta2, (float)pr->eps, d_losses ? d_losses + e : nullptr, u.ent_coeff};
        u.adam = fused ? &ad : nullptr;
        if ((rc = run_update(c, u, st))) return rc;
        if (!fused) {
            if ((c->xg_world > 1 || c->nccl_comm) && (rc = comm_allreduce_f64(c, gout, P + 1, st))) return rc;
            hipLaunchKernelGGL(k_ppo_step, dim3(1), dim3(1024), 0, st, gout, P, c->pd.pol.n_params, c->pd.na, 1, ad);
        }
        HIP_TRY(c, hipGetLastError());
        c->pol_adam_t = t1;
    }
    return METRPO_OK;
}

// ---- 'ppo' with use_kl_penalty (ppo.py:120-121): loss += kl_penalty * max(0, mean_kl - step_size), semantics in include/metrpo.h ----
// The [loss, mean KL] pair(s) the OP_LOSSKL reduction writes and the OP_PPOKL kernels read.
static int ensure_ppo_kl(metrpo_ctx* c, int n_pairs) { return ws_grow(c, c->d_ppo_kl, sizeof(double) * 2 * (size_t)std::max(1, n_pairs)); }

// OP_LOSSKL at the ctx theta + its reduction into pair[0..1]; summed over the ranks when `global` (in the reduction's tail where the scope says so, else by a
// stand-alone all-reduce).  pair[1] = mean KL: every rank's share is over inv_n_global, so the ranks' sum is the global mean.
static int ppo_kl_mean_kl(metrpo_ctx* c, const metrpo_batch* b, double* pair, bool exchange_in_tail, bool global, hipStream_t st) {
    UpdCall u; int rc = make_call(c, OP_LOSSKL, b, &u); if (rc) return rc;
    u.out = pair; u.scope.exchange_in_tail = exchange_in_tail;
    if ((rc = run_update(c, u, st))) return rc;
    if (global && !(exchange_in_tail && c->xg_world > 1) && (c->xg_world > 1 || c->nccl_comm)) return comm_allreduce_f64(c, pair, 2, st);
    return METRPO_OK;
}

int launch_ppo_kl_loss_grad(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, const metrpo_ppo_kl_params* kp, const double* d_mean_kl, double* out, hipStream_t st) {
    UpdCall u; int rc = make_call(c, OP_PPOKL, b, &u, pr, kp); if (rc) return rc;
    if (d_mean_kl == nullptr) {                              // computed here: the same launches metrpo_loss_kl makes, summed over an attached communicator's ranks
        if ((rc = ensure_ppo_kl(c, 1)) || (rc = ppo_kl_mean_kl(c, b, c->d_ppo_kl.p, false, true, st))) return rc;
        d_mean_kl = c->d_ppo_kl.p + 1;
    }
    u.k.mean_kl = d_mean_kl; u.out = out;
    if ((rc = run_update(c, u, st))) return rc;
    if (policy_gemm_applicable(c, b->N, false)) {            // (its own reduction: the entropy term follows as a launch, as in launch_ppo_loss_grad)
        AdamTail ad = {}; ad.theta = c->d_theta.p; ad.ent_coeff = u.ent_coeff;
        hipLaunchKernelGGL(k_ppo_step, dim3(1), dim3(1024), 0, st, out, c->pd.P, c->pd.pol.n_params, c->pd.na, 0, ad);
        HIP_TRY(c, hipGetLastError());
    }
    return METRPO_OK;
}

// run_ppo_update with, in front of each epoch's gradient launch, the OP_LOSSKL launch and reduction that leave the global mean KL of the theta entering the epoch
// in pair e of d_ppo_kl; the OP_PPOKL kernels read it there and take the gate themselves.  Nothing here reads the device.
int run_ppo_kl_update(metrpo_ctx* c, const metrpo_batch* b, const metrpo_ppo_params* pr, const metrpo_ppo_kl_params* kp, int n_epochs, double* d_losses, double* d_mean_kls,
                      hipStream_t st) {
    const int P = c->pd.P;
    if (!pr) return set_err(c, METRPO_ENULL, "ppo_kl_update: params NULL");
    if (n_epochs < 0) return set_err(c, METRPO_EINVAL, "ppo_kl_update: n_epochs must be >= 0");
    if (!(pr->lr >= 0.0) || !(pr->beta1 >= 0.0 && pr->beta1 < 1.0) || !(pr->beta2 >= 0.0 && pr->beta2 < 1.0) || !(pr->eps >= 0.0))
        return set_err(c, METRPO_EINVAL, "ppo_kl_update: need lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0");
    UpdCall u; int rc = make_call(c, OP_PPOKL, b, &u, pr, kp); if (rc) return rc;
    if ((rc = ensure_policy_adam(c)) || (rc = ensure_ppo_kl(c, n_epochs))) return rc;
    float* am = (float*)c->d_pol_adam.p;
    double* gout = c->d_cg.p;                               // [1 + P] of the CG workspace (no update is open across this call)
    const UpdFusion f = update_fusion(c, b->N, false);      // as run_ppo_update: the ranks must agree on it
    const bool fused = f.carries_next_step();
    u.out = gout; u.scope.exchange_in_tail = f.exchange_in_tail;
    if (!fused) u.ent_in_reduction = false;
    for (int e = 0; e < n_epochs; ++e) {
        double* pair = c->d_ppo_kl.p + 2 * (size_t)e;
        if ((rc = ppo_kl_mean_kl(c, b, pair, f.exchange_in_tail, true, st))) return rc;
        u.k.mean_kl = pair + 1;
        const int t1 = c->pol_adam_t + 1;                   // launch_policy_adam's bias correction (bptt.hip)
        const double lr_t = pr->lr * std::sqrt(1.0 - std::pow(pr->beta2, (double)t1)) / (1.0 - std::pow(pr->beta1, (double)t1));
        const AdamTail ad = {c->d_theta.p, am, am + P, (float)lr_t, (float)pr->beta1, (float)pr->beta2, (float)pr->eps, d_losses ? d_losses + e : nullptr, u.ent_coeff};
        u.adam = fused ? &ad : nullptr;
        if ((rc = run_update(c, u, st))) return rc;
        if (!fused) {                                       // the stand-alone sequence of run_ppo_update, unchanged
            if ((c->xg_world > 1 || c->nccl_comm) && (rc = comm_allreduce_f64(c, gout, P + 1, st))) return rc;
            hipLaunchKernelGGL(k_ppo_step, dim3(1), dim3(1024), 0, st, gout, P, c->pd.pol.n_params, c->pd.na, 1, ad);
        }
        HIP_TRY(c, hipGetLastError());
        c->pol_adam_t = t1;
    }
    if (d_mean_kls && n_epochs > 0)                         // column 1 of the pairs, one strided device-to-device copy behind the last epoch
        HIP_TRY(c, hipMemcpy2DAsync(d_mean_kls, sizeof(double), c->d_ppo_kl.p + 1, 2 * sizeof(double), sizeof(double), (size_t)n_epochs, hipMemcpyDeviceToDevice, st));
    return METRPO_OK;
}
