// MFMA path of the per-model DETERMINISTIC rollout of build_policy_graph (model_based_rl.py:106-151) for the small-MLP shapes
// (dynamics 2x64 relu, policy 2x32 tanh): forward sweep (= per-model validation costs, metrpo_validation_cost, and the
// stored trajectory of the BPTT update) and reverse sweep (adjoint of the policy mean for every (model, t, env); bptt.hip has
// the generic-width version and the description of the recursion).
//
// Mapping: grid.y = model i, a WAVE owns one tile of 16 envs of that model for the whole horizon (no cross-wave traffic, no
// barriers after the prologue).  Every layer and every layer-adjoint is a TRANSPOSED MFMA chain (v_mfma_f32_16x16x4_f32):
//   forward   H^T[unit][env]  = W^T . X^T      A = W^T fragments, B = activations in D layout of the previous layer
//   adjoint   dX^T[in][env]   = W . dH^T       A = W   fragments, B = deltas      in D layout of the next     layer
// so activations and deltas never leave registers between layers.  Constant factors are folded into the fragments: diff_std
// into the first adjoint layer, 1/in_std and the column drop into the last one, which is split into a state part (rows = state
// dims: lands in the layout of the residual path) and an action part (rows = action dims).
// The forward dynamics head is dyn_head_mfma.h's (register-resident fragments; the layout is described there); its adjoint is
// dyn_head_adjoint.h's DynHeadAdjoint and the policy's two tanh layers and input adjoint are pol_head_mfma.h's PolHeadAdjoint, both on
// fragment tables in an LDS image shared by the 4 waves of a workgroup (same model).  What this file states itself: the image's
// composition (DetL), the mean's last layer, the clip and its gate, and the cost adjoint in D layout (profiles/r28_score_bodies.txt:
// factoring that block out cost its sibling kernels registers).
#include "dyn_head_adjoint.h"
#include "pol_head_mfma.h"

enum { DET_FWD = 0, DET_BWD = 1 };

template <int ENV>
struct DetL {
    using C = Cfg<ENV, 64, 32>;
    using Pol = PolHeadAdjoint<C>;
    using Adj = DynHeadAdjoint<C>;
    static constexpr int NS = C::NS, NA = C::NA, OUT_CB = C::OUT_CB;
    // LDS image (floats): the policy's fragment tables and hidden bias rows (pol_head_mfma.h) | the mean's last forward layer [k-step][64 lanes] and its
    // bias row, this file's own | the dynamics adjoint tables (dyn_head_adjoint.h) | the three dynamics bias rows
    static constexpr int O_PF2 = Pol::FLOATS, O_BP2 = O_PF2 + 8 * 64, O_ADJ = O_BP2 + 16, O_BD0 = O_ADJ + Adj::FLOATS, O_BD1 = O_BD0 + 64,
                         O_BD2 = O_BD1 + 64, IMG = O_BD2 + 16 * OUT_CB;
    static constexpr int LOC_P = O_ADJ - O_PF2, LOCAL = LOC_P + (IMG - O_BD0);       // the rows that k_det_mfma fills itself
    static_assert(IMG == 64 * (2 * C::NS_KS + 16 + 8 + 2 * Pol::RK + 16 + 8 * OUT_CB)       // policy tables: PF0 PF1 PF2 PB2 PB1 PB0
                         + 64 * (16 * OUT_CB + 64 + 16 * OUT_CB + 16)                    // dynamics adjoint tables: DB2 DB1 DAS DAA
                         + 64 + 64 + 16 * OUT_CB + 32 + 32 + 16,                         // the six bias rows
                  "the image holds what it held when this file laid out every table itself");
    static constexpr int WV = ((16 * NS * 2 + 16 * NA + 3) / 4) * 4;     // per wave: ST | NX | ACT
    static constexpr int TOTAL = IMG + 4 * WV;
};

// STOCH ('bptt-stochastic', bptt.hip): mu becomes mean + eps exp(log_std) before the clip in both sweeps (lane (c, q) draws chunk q of env c,
// bptt_eps4), so the reverse sweep's clip gate sees the forward sweep's pre-clip action; the deterministic instantiations never read nz.
template <int ENV, int MODE, bool STOCH>
__global__ void __launch_bounds__(256, 2) k_det_mfma(int K, int B, int T, double gamma, const float* __restrict__ dynp,
                                                    const float* __restrict__ theta, const float* __restrict__ norm,
                                                    const float* __restrict__ s0, float* __restrict__ XS, float* __restrict__ WT,
                                                    float* __restrict__ GM, double* __restrict__ cost_part, BpttNoise nz) {
    using L = DetL<ENV>;
    using C = typename L::C;
    constexpr int NS = C::NS, NA = C::NA, OUT_CB = C::OUT_CB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int model = blockIdx.y;
    const int b0 = (blockIdx.x * 4 + wave) * 16, b = b0 + c;
    const bool active = b < B;
    const float* __restrict__ pk = dynp + (size_t)model * C::PD;
    float* IMG = lds;
    float* ST = lds + L::IMG + wave * L::WV; float* NX = ST + 16 * NS; float* ACT = NX + 16 * NS;

    // ---------------- LDS image: the shared heads' tables, then this file's own rows; each element written by one thread ----------------
    L::Pol::fill(IMG, theta, tid, 256);
    L::Adj::fill(IMG + L::O_ADJ, pk, norm, tid, 256);
    for (int j = tid; j < L::LOCAL; j += 256) {
        const int i = (j < L::LOC_P) ? L::O_PF2 + j : L::O_BD0 + (j - L::LOC_P);
        float w = 0.0f;
        const int ln = i & 63, cc = ln & 15, qq = ln >> 4;
        if (i < L::O_BP2) { const int kk = (i - L::O_PF2) >> 6; if (cc < NA) w = theta[C::pW2 + chained_in(kk, qq) * NA + cc]; }
        else if (i < L::O_ADJ) { const int d = i - L::O_BP2; if (d < NA) w = theta[C::pb2 + d]; }
        else if (i < L::O_BD1) w = pk[C::db0 + (i - L::O_BD0)];
        else if (i < L::O_BD2) w = pk[C::db1 + (i - L::O_BD1)];
        else { const int u = i - L::O_BD2; if (u < NS) w = pk[C::db2 + u]; }
        IMG[i] = w;
    }
    const typename L::Pol pol = {IMG, lane};
    const typename L::Adj adj = {IMG + L::O_ADJ, lane};
    // ---------------- register-resident forward dynamics fragments ----------------
    DynHeadFrags<C, MODE == DET_FWD> head;                                   // the reverse sweep recomputes layers 0 and 1 only
    DynInNorm<C> in;
    DynOutNorm<C> out;
    head.load(pk, c, q);
    in.load(norm, q);
    out.load(norm, q);
    const size_t xs_model = (size_t)model * (T + 1) * B * NS;
    float sd[4];                                                             // exp(log_std) of the action dims 4q .. 4q+3 (STOCH)
#pragma unroll
    for (int r = 0; r < 4; ++r) sd[r] = (STOCH && 4 * q + r < NA) ? expf(nz.log_std[4 * q + r]) : 0.0f;
    __syncthreads();

    // one step of the forward computations shared by both modes: policy chain -> clip -> ACT; dynamics layers 0, 1
    f32x4 p0[2], p1[2], mu, h0[4], h1[4];
    int nsat[4] = {0, 0, 0, 0};                                              // STOCH forward: |u| == 1 count of (env c, dim 4q + r) over t
    auto step_forward = [&](int t) {
        pol.hidden(p0, p1, ST, c);
        f32x4 m0 = *(const f32x4*)&IMG[L::O_BP2 + 4 * q], m1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; kk += 2) {
            m0 = MFMA16(IMG[L::O_PF2 + kk * 64 + lane], p1[kk >> 2][kk & 3], m0);
            m1 = MFMA16(IMG[L::O_PF2 + (kk + 1) * 64 + lane], p1[(kk + 1) >> 2][(kk + 1) & 3], m1);
        }
        mu = m0 + m1;
        if (STOCH && 4 * q < NA) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (active) bptt_eps4(nz, model, t, B, b, NA, q, e);
#pragma unroll
            for (int r = 0; r < 4; ++r) mu[r] = fmaf(e[r], sd[r], mu[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 4 * q + r;
            if (d < NA) {
                const float u = fminf(fmaxf(mu[r], -1.0f), 1.0f);                                       // :128
                ACT[c * NA + d] = u;
                if (STOCH && MODE == DET_FWD && fabsf(u) == 1.0f) ++nsat[r];                                 // :129
            }
        }
        wave_lds_sync();
        float xin[C::NIN_KS];
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) xin[s] = in.get(ST, NS, ACT, c, s);
        head.layer0(h0, IMG + L::O_BD0, xin, ReluFmax());
        head.layer1(h1, IMG + L::O_BD1, h0, ReluFmax());
    };
    const int lim = min(16, max(0, B - b0)) * NS;                            // floats of this tile in one [B][ns] slice

    if constexpr (MODE == DET_FWD) {
        // ------------------------------------------------ forward sweep ------------------------------------------------
        for (int i = lane; i < 16 * NS; i += 64) ST[i] = (i < lim) ? s0[(size_t)b0 * NS + i] : 0.0f;
        wave_lds_sync();
        double acc = 0.0, g = 1.0;
        float dones = 0.0f;
        for (int t = 0; t < T; ++t) {
            if (XS != nullptr) for (int i = lane; i < lim; i += 64) XS[xs_model + ((size_t)t * B + b0) * NS + i] = ST[i];
            step_forward(t);
            f32x4 oa[OUT_CB], ob[OUT_CB];
            head.layer2(oa, ob, IMG + L::O_BD2, h1);
#pragma unroll
            for (int cb = 0; cb < OUT_CB; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int dim = 16 * cb + 4 * q + r;
                    if (dim < NS) NX[c * NS + dim] = out.apply(cb, r, oa[cb][r] + ob[cb][r], ST[c * NS + dim]);
                }
            wave_lds_sync();
            if (q == 0) {                                        // one lane per env: cost, dones, weight
                const float cst = env_cost(ENV, NS, NA, EnvVec{NX + c * NS, 1}, EnvVec{ACT + c * NA, 1});
                const float live = 1.0f - dones;
                if (ENV == METRPO_ENV_ANT) dones = fmaxf(dones, env_done_scan(ENV, NS, EnvVec{NX + c * NS, 1}) ? 1.0f : 0.0f);
                if (active) {
                    acc += g * (double)(cst * live);
                    if (WT != nullptr) WT[((size_t)model * T + t) * B + b] = (float)(g * (double)live / ((double)B * (double)K));
                }
            }
            g *= gamma;
            for (int i = lane; i < 16 * NS; i += 64) ST[i] = NX[i];
            wave_lds_sync();
        }
        if (XS != nullptr) for (int i = lane; i < lim; i += 64) XS[xs_model + ((size_t)T * B + b0) * NS + i] = ST[i];
        if (STOCH && nz.n_sat != nullptr && active)                          // one add per (model, env, dim): the models share a cell
#pragma unroll
            for (int r = 0; r < 4; ++r) if (4 * q + r < NA && nsat[r] != 0) atomicAdd(&nz.n_sat[(size_t)b * NA + 4 * q + r], nsat[r]);
        // deterministic cost reduction: lanes -> wave (shuffles) -> one slot per (model, tile)
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) cost_part[(size_t)model * (gridDim.x * 4) + blockIdx.x * 4 + wave] = acc / (double)B;
    } else {
        // ------------------------------------------------ reverse sweep ------------------------------------------------
        f32x4 lam[OUT_CB];
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb) lam[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = T - 1; t >= 0; --t) {
            for (int i = lane; i < 16 * NS; i += 64) {
                ST[i] = (i < lim) ? XS[xs_model + ((size_t)t * B + b0) * NS + i] : 0.0f;
                NX[i] = (i < lim) ? XS[xs_model + ((size_t)(t + 1) * B + b0) * NS + i] : 0.0f;
            }
            const float w = active ? WT[((size_t)model * T + t) * B + b] : 0.0f;
            wave_lds_sync();
            step_forward(t);
            // ---- cost adjoint in D layout: G = lambda_{t+1} + w dc/dx_next (state dims), gU = w dc/du (action dims) ----
            f32x4 G[OUT_CB], gU;
            env_cost_adjoint_d<ENV, NS, NA>(G, gU, lam, w, NX + c * NS, ACT + c * NA, q);
            // ---- dynamics adjoint: gS = G + state rows of F^T G (the residual identity), gU += action rows ----
            f32x4 gS[OUT_CB];
            adj.run(gS, gU, G, h0, h1);
            // ---- clip gate (tf.clip_by_value passes the gradient inside [min, max]) and the mean-adjoint output ----
            f32x4 gm;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 4 * q + r;
                gm[r] = (d < NA && mu[r] >= -1.0f && mu[r] <= 1.0f) ? gU[r] : 0.0f;
                if (d < NA && active) GM[(((size_t)model * (T + 1) + t) * B + b) * NA + d] = gm[r];
            }
            // ---- policy input adjoint: gS += J_pi(x_t)^T gm ----
            pol.run(gS, gm, p0, p1);
#pragma unroll
            for (int cb = 0; cb < OUT_CB; ++cb) lam[cb] = gS[cb];                     // lambda_t
            wave_lds_sync();
        }
    }
}

// fixed-order sum of the per-tile cost partials of one model
// err (may be NULL): time-out cell of the launch that wrote the partials (val_err_cell: the resident validation launches; cleared in front of them).  A
// resident validation launch whose grid was not co-resident leaves invalid partial sums; callers of metrpo_validation_cost read no error cell, so the
// costs themselves carry the failure: NaN instead of plausible garbage feeding model selection and early stopping.  Every other producer of partials
// passes NULL: an unrelated rollout's sticky time-out must not turn valid costs into NaN.
__global__ void k_det_cost_reduce(int n_part, const double* __restrict__ part, double* __restrict__ costs, const double* __restrict__ err) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n_part; ++i) s += part[(size_t)blockIdx.x * n_part + i];
        if (err != nullptr && *err != 0.0) s = __builtin_nan("");
        costs[blockIdx.x] = s;
    }
}

// costs[k] = the n_part partials of model k added in index order (also the generic forward kernels' block sums: rollout_generic.hip, bptt.hip)
int launch_det_cost_reduce(metrpo_ctx* c, int n_part, const double* part, double* costs, hipStream_t st, const double* err) {
    hipLaunchKernelGGL(k_det_cost_reduce, dim3(c->pd.K), dim3(64), 0, st, n_part, part, costs, err);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

// -------------------------------------------------------------------------------------------------
typedef void (*det_kernel_t)(int, int, int, double, const float*, const float*, const float*, const float*, float*, float*, float*, double*, BpttNoise);
struct DetEntry { int env; det_kernel_t fwd, bwd, fwd_s, bwd_s; int lds_floats; };       // _s: the 'bptt-stochastic' sweeps
#define DENTRY(E) {E, k_det_mfma<E, DET_FWD, false>, k_det_mfma<E, DET_BWD, false>, k_det_mfma<E, DET_FWD, true>, k_det_mfma<E, DET_BWD, true>, DetL<E>::TOTAL}
static const DetEntry kDet[] = {DENTRY(METRPO_ENV_SWIMMER), DENTRY(METRPO_ENV_HALF_CHEETAH), DENTRY(METRPO_ENV_HOPPER), DENTRY(METRPO_ENV_SNAKE),
                                DENTRY(METRPO_ENV_ANT)};

// table index or -1: same shape conditions as the MFMA rollouts (dynamics 2x64 relu, policy 2x32 tanh, known env dims)
int det_mfma_select(const metrpo_ctx* c) {
    const ProblemDesc& pd = c->pd;
    const bool exact = c->mfma_cfg >= 0 && pd.dyn.n_layers == 3 && pd.dyn.dims[1] == 64 && pd.dyn.dims[2] == 64;
    const bool padded = c->coop_cfg < 0 && c->coop_pad_cfg >= 0;            // two hidden layers of at most 64 units: the zero-padded copy in the 64 x 64 layout (api.hip)
    if ((!exact && !padded) || pd.pol.n_layers != 3 || pd.pol.dims[1] != 32 || pd.pol.dims[2] != 32)
        return -1;
    for (int i = 0; i < (int)(sizeof(kDet) / sizeof(kDet[0])); ++i)
        if (kDet[i].env == pd.env) return i;
    return -1;
}

// part: >= K * tiles4 doubles of scratch (tiles4 = 4 * ceil(B/64)).  XS / WT may be NULL (validation cost only).
// nz: the 'bptt-stochastic' noise (NULL: deterministic)
int launch_det_forward(metrpo_ctx* c, int idx, const float* s0, int B, int T, double gamma, float* XS, float* WT, double* part, double* costs,
                       hipStream_t st, const BpttNoise* nz) {
    const DetEntry& en = kDet[idx];
    const det_kernel_t fwd = nz ? en.fwd_s : en.fwd;
    const size_t sh = sizeof(float) * (size_t)en.lds_floats;
    if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    const int gx = (B + 63) / 64;
    const float* dyn = c->d_dyn.p;
    if (c->det_padded) { const int rc = launch_pad_dyn(c, st); if (rc) return rc; dyn = c->d_dyn_pad.p; }
    hipLaunchKernelGGL(fwd, dim3(gx, c->pd.K), dim3(256), sh, st, c->pd.K, B, T, gamma, dyn, c->d_theta.p, c->d_norm.p, s0, XS, WT,
                       (float*)nullptr, part, nz ? *nz : BpttNoise{});
    hipLaunchKernelGGL(k_det_cost_reduce, dim3(c->pd.K), dim3(64), 0, st, gx * 4, part, costs, (const double*)nullptr);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int launch_det_backward(metrpo_ctx* c, int idx, int B, int T, const float* XS, const float* WT, float* GM, hipStream_t st, const BpttNoise* nz) {
    const DetEntry& en = kDet[idx];
    const det_kernel_t bwd = nz ? en.bwd_s : en.bwd;
    const size_t sh = sizeof(float) * (size_t)en.lds_floats;
    if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    const float* dyn = c->d_dyn.p;
    if (c->det_padded) { const int rc = launch_pad_dyn(c, st); if (rc) return rc; dyn = c->d_dyn_pad.p; }
    hipLaunchKernelGGL(bwd, dim3((B + 63) / 64, c->pd.K), dim3(256), sh, st, c->pd.K, B, T, 1.0, dyn, c->d_theta.p, c->d_norm.p,
                       (const float*)nullptr, const_cast<float*>(XS), const_cast<float*>(WT), GM, (double*)nullptr, nz ? *nz : BpttNoise{});
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}
