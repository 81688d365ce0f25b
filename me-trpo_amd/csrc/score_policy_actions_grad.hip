// metrpo_score_policy_actions_grad (include/metrpo.h): for every head k and candidate b the gradient of the head's CLOSED-LOOP return
//   R = -sum_t w_t cost_tf(s_t, clip(a_t), s_t+1),   a_t = pi(s_t) + noise_t sigma,   w_t = gamma^t alive_t        (metrpo_score_policy_actions' ret)
// with respect to the noise sequences (d_grad [K][T][B][na]) and the start state (d_lam0 [K][B][ns]).  Reverse recursion from lambda_T = 0:
//   G = lambda_t+1 - w_t dc/dx_next;  gU = -w_t dc/du + (action rows of F^T G);  gm = gU gated by -1 <= a_t <= 1;  grad_t = gm (* sigma in std units)
//   lambda_t = G + (state rows of F^T G) + J_pi(s_t)^T gm
// metrpo_score_actions_grad's recursion (score_actions_grad.hip) with the policy path: the last term, and the action of step t is the head's own.
//
// Fused path: TWO stream-ordered launches per chunk of candidates (the second sees the first one's stores without any in-kernel fence).
//   k_spag_fwd  k_score_policy_actions' mapping and step, statement for statement (score_policy_actions.hip: PolWaveHead::mean, the fmaf with sigma, the
//               clip, DynWaveHead::step, cost and done), so ret, len and act_out carry that kernel's bits.  Per step it additionally stores the tile's state
//               block into XS [K][T+1][Bc][ns] as one linear store, the fp32 weight into WT [K][T][Bc] and the head's UNCLIPPED action into AW [K][T][Bc][na]:
//               the reverse sweep's clip gate and recomputed dynamics layers read the very a_t the forward sweep formed.
//   k_spag_bwd  k_sagr<ENV, SAGR_BWD>'s structure: a workgroup is 4 waves = four 16-candidate tiles of the SAME head (blockIdx.y), launch bound (256, 2);
//               one LDS image of the head's adjoint tables (dyn_head_adjoint.h) AND the policy's forward and adjoint tables (pol_head_mfma.h:
//               PolHeadAdjoint), 41 KB swimmer .. 55 KB Ant, with the waves' buffers 47 .. 73 KB a workgroup (SpagL: two fit a CU's 160 KB);
//               layers 0 and 1 of the head recomputed from XS[t] and AW[t]; the cost adjoint in D layout (k_sagr's statements; a shared
//               function costs instantiations of both kernels registers: profiles/r28_score_bodies.txt); DynHeadAdjoint::run; the clip gate on AW[t]; the store of grad[k][t]; then the policy's two hidden layers recomputed from XS[t] and its
//               three-chain input adjoint accumulated INTO gS.  The prefetch is k_sagr's: one state block, one action block (now per head, from AW: the
//               tile's rows of a step are one linear run there too) and one weight per step, issued at the top of step t, committed behind it; two state
//               buffers alternate.
//   Edge tile and chunks as in score_actions_grad.hip: rows at and beyond the chunk's end are zeros in LDS, never read from or written to memory; the
//   forward sweep computes rows of a later chunk that share its last tile and drops them, so chunking changes no bit.
//
// Generic path (every other shape, and force_generic): k_spag_gen_fwd / k_spag_gen_bwd, one thread per (candidate, head) with activations in LDS
// columns -- k_sagr_gen_fwd / k_sagr_gen_bwd with the policy in the loop (both on sact_sum.h's GradBufs and device_common.h's net_hidden and net_vjp and env_model.h's env_cost_adjoint): the forward is k_policy_actions' and k_step's arithmetic (rollout_generic.hip;
// sigma by __expf as there), so ret, len and act_out carry the bits of metrpo_score_policy_actions' generic path; the reverse is k_bptt_backward's policy
// VJP (bptt.hip) behind the clip gate.  Block size by lds_block_size (metrpo_internal.h).  Same outputs, workspace, chunking.
//
// Terminal value (sact_sum.h: TermVal), as in score_actions_grad.hip: the forward sweeps add the term behind the loop and STORE w_T into WE [K][Bc] (one more slice
// of WT, only while a value is set; stored, not re-derived); the reverse sweeps start from lambda_T = w_T dV/ds_T formed from the stored XS[T] tile.  The seed
// enters step T-1 through G and so reaches J_pi(s_T-1) like any lambda.  k_spag_gen_fwd<TV> takes the value as a template parameter (the runtime test reserved
// a stack slot there); k_spag_fwd, k_spag_bwd and k_spag_gen_bwd test the pointer, runtime-uniform: none of them loses a register or a wave to it.
// The MLP form (metrpo_set_terminal_value_mlp): k_spag_gen_fwd<TV_MLP> and k_spag_fwd<.., MLP> evaluate it behind their loop; its seed comes from k_tv_mlp_seed
// (score_actions_grad.hip), launched between the sweeps, and k_spag_bwd<.., SEEDED> / k_spag_gen_bwd<SEEDED> read it in front of their loop.
//
// Workspace: ctx->d_spag = XS | WT | AW (| WE) of one chunk, within 2^26 floats (args.chunk > 0 overrides).  d_grad_mean: k_sagr_mean.  No atomics anywhere.
#include "dyn_tile_step.h"
#include "dyn_head_adjoint.h"
#include "pol_head_mfma.h"
#include "sact_sum.h"
#include <algorithm>
#include <cmath>

struct SpagK {
    int B, T, per;            // per = B / S: candidates per start state
    int stop;                 // 1: a candidate stops counting behind its first done
    int in_std;               // 1: the noise is in units of the policy's std
    int c0, n;                // the chunk: candidates c0 .. c0 + n - 1; XS / WT / AW hold n columns
    double gamma;
    const float* init_obs; const float* noise;
    float* XS; float* WT; float* AW;      // [K][T+1][n][ns], [K][T][n], [K][T][n][na]
    float* WE;                            // [K][n]: w_T, one more slice of WT, only while a terminal value is set
    TermVal tv;                           // the context's terminal value; unset: all NULL
    float* ret; int32_t* len; float* act_out;
    float* grad; float* lam0;             // [K][T][B][na], optional [K][B][ns]
};

// ------------------------------------------------ forward sweep: k_score_policy_actions' step, storing ------------------------------------------------
// MLP: the terminal value is the two-layer net (sact_sum.h) -- a template parameter; without it the kernel it was, with the runtime test for the quadratic form
template <int ENV, bool NOISE, bool MLP = false>
__global__ void __launch_bounds__(64) k_spag_fwd(SpagK r, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm) {
    using C = Cfg<ENV, 64, 32>;
    constexpr int NS = C::NS, NA = C::NA, NST = cdiv(16 * NS, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, e = lane & 15, q = lane >> 4;
    const int b0 = r.c0 + blockIdx.x * 16, k = blockIdx.y, b = b0 + e;
    const int nrows = min(16, r.B - b0);                      // rows of this tile inside the batch
    const int end = r.c0 + r.n;                               // ... and inside the chunk: the rows that are stored
    const bool mine = b < end;
    const int lim = min(16, end - b0) * NS;
    const int lc = b - r.c0;
    float* W = lds;
    float* ST = W + C::W_ST;  float* NX = W + C::W_NX;

    DynWaveHead<C> head;
    head.load(dynp + (size_t)k * C::PD, norm, W + C::W_BD0, W + C::W_BD1, W + C::W_BD2, lane);
    PolWaveHead<C> pol;
    pol.load(theta, W + C::W_BP0, W + C::W_BP1, W + C::W_BP2, lane);
    float sig[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) sig[rr] = (NOISE && r.in_std && 4 * q + rr < NA) ? expf(fmaxf(theta[C::pLS + 4 * q + rr], LOG_MIN_STD)) : 1.0f;
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = lane + 64 * j;
        const int row = i / NS, col = i - row * NS;
        if (i < 16 * NS) ST[i] = (row < nrows) ? r.init_obs[(size_t)((b0 + row) / r.per) * NS + col] : 0.0f;
    }
    NoiseTile<C> nz;
    if (NOISE) {
        nz.init(r.noise, r.B, r.T, b0, nrows, lane, W, C::W_ACT, al4(C::W_TOTAL));
        nz.prefetch(0);
        nz.commit(0);
    }
    wave_lds_sync();
    float* xs_k = r.XS + ((size_t)k * (r.T + 1) * r.n + (b0 - r.c0)) * NS;       // + t n NS: the tile's rows of slice t, linear
    for (int i = lane; i < lim; i += 64) xs_k[i] = ST[i];
    loop_invariant_loads_done();

    SactSum acc;
    for (int t = 0; t < r.T; ++t) {
        float* ACT = NOISE ? nz.cur(t) : W + C::W_ACT;       // the step's noise rows, overwritten by the clipped action
        if (NOISE) nz.prefetch(t + 1);                         // committed behind the matrix instructions
        const f32x4 mu = pol.mean(ST, e);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int d = 4 * q + rr;
            if (d < NA) {
                float a = mu[rr];
                if (NOISE) a = fmaf(ACT[e * NA + d], sig[rr], a);
                if (mine) {
                    r.AW[(((size_t)k * r.T + t) * r.n + lc) * NA + d] = a;
                    if (r.act_out != nullptr) r.act_out[(((size_t)k * r.T + t) * r.B + b) * NA + d] = a;
                }
                ACT[e * NA + d] = fminf(fmaxf(a, -1.0f), 1.0f);            // np.clip(actions, *bounds), env_helpers.py:599
            }
        }
        wave_lds_sync();
        f32x4 nx[C::OUT_CB];
        head.step(nx, ST, NS, ACT, e);
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) NX[e * NS + dim] = nx[cb][rr];
            }
        if (NOISE) nz.commit(t + 1);
        wave_lds_sync();
        const float cost = env_cost(ENV, NS, NA, EnvVec{NX + e * NS, 1}, EnvVec{ACT + e * NA, 1});
        const bool dn = env_done_scan(ENV, NS, EnvVec{NX + e * NS, 1});
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NS) ST[i] = NX[i];
        }
        wave_lds_sync();
        const float w = acc.step(-cost, dn, r.gamma, r.stop);
        if (q == 0 && mine) r.WT[((size_t)k * r.T + t) * r.n + lc] = w;
        float* dst = xs_k + (size_t)(t + 1) * r.n * NS;
        for (int i = lane; i < lim; i += 64) dst[i] = ST[i];
    }
    if (q == 0 && mine) {                                      // rounded to fp32 once, here
        if constexpr (MLP) r.WE[(size_t)k * r.n + lc] = acc.terminal(r.tv.mlp_value(ST + e * NS, 1, NS, b, r.per));
        else if (r.tv.set()) r.WE[(size_t)k * r.n + lc] = acc.terminal(r.tv.value(ST + e * NS, 1, NS, b, r.per));      // ST holds s_T behind the loop
        const size_t kb = (size_t)k * r.B + b;
        if (r.ret != nullptr) r.ret[kb] = (float)acc.sum;
        if (r.len != nullptr) r.len[kb] = acc.n;
    }
}

// LDS of the reverse sweep (floats): the head's adjoint tables | its bias rows of layers 0, 1 | the policy's tables and hidden bias rows |
// per wave: two state buffers, the clipped and the raw action block
template <int ENV>
struct SpagL {
    using C = Cfg<ENV, 64, 32>;
    using A = DynHeadAdjoint<C>;
    using P = PolHeadAdjoint<C>;
    static constexpr int O_BD0 = A::FLOATS, O_BD1 = O_BD0 + 64, O_POL = O_BD1 + 64, IMG = O_POL + P::FLOATS;
    static constexpr int SB = al4(16 * C::NS), AB = al4(16 * C::NA), WV = 2 * SB + 2 * AB;
    static constexpr int TOTAL = IMG + 4 * WV;
    static_assert(2 * TOTAL * 4 <= 160 * 1024, "two workgroups of the reverse sweep share a CU's LDS");
};

// ------------------------------------------------ reverse sweep ------------------------------------------------
// SEEDED: the MLP form -- lambda_T is read from the workspace behind WE, where k_tv_mlp_seed (score_actions_grad.hip) wrote it; without it the kernel it was
template <int ENV, bool SEEDED = false>
__global__ void __launch_bounds__(256, 2) k_spag_bwd(SpagK r, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm) {
    using L = SpagL<ENV>;
    using C = typename L::C;
    constexpr int NS = C::NS, NA = C::NA, OUT_CB = C::OUT_CB, NST = cdiv(16 * NS, 64), NLD = cdiv(16 * NA, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float* __restrict__ pk = dynp + (size_t)k * C::PD;
    L::A::fill(lds, pk, norm, tid, 256);
    L::P::fill(lds + L::O_POL, theta, tid, 256);
    for (int i = tid; i < 64; i += 256) { lds[L::O_BD0 + i] = pk[C::db0 + i]; lds[L::O_BD1 + i] = pk[C::db1 + i]; }
    DynHeadFrags<C, false> head;                                             // layers 0 and 1 only
    DynInNorm<C> in;
    head.load(pk, c, q);
    in.load(norm, q);
    // d noise / d a: 1, or the forward sweep's sigma where the noise is in units of the policy's std
    float sig[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) sig[rr] = (r.in_std && 4 * q + rr < NA) ? expf(fmaxf(theta[C::pLS + 4 * q + rr], LOG_MIN_STD)) : 1.0f;
    __syncthreads();                                                         // the only barrier: the tables are read-only from here on
    const int l0 = (blockIdx.x * 4 + wave) * 16;                             // the tile's first column of the chunk
    if (l0 >= r.n) return;
    const typename L::A adj = {lds, lane};
    const typename L::P padj = {lds + L::O_POL, lane};
    float* W = lds + L::IMG + wave * L::WV;
    float* ACT = W + 2 * L::SB; float* ARAW = ACT + L::AB;
    const int nrows = min(16, r.n - l0), lim = nrows * NS, nact = nrows * NA;
    const int lc = l0 + c, b = r.c0 + lc;                                    // this lane's column of the chunk / candidate of the batch
    const bool active = c < nrows;
    const float* __restrict__ xs_k = r.XS + ((size_t)k * (r.T + 1) * r.n + l0) * NS;      // + t n NS: the tile's rows of slice t, linear
    const float* __restrict__ wt_k = r.WT + (size_t)k * r.T * r.n + min(lc, r.n - 1);     // + t n
    const float* __restrict__ aw_k = r.AW + ((size_t)k * r.T * r.n + l0) * NA;            // + t n NA: the tile's action block of step t, linear
    float xs_nx[NST], a_nx[NLD], w_nx;
    // the loads of step t's rows (clamped into the tile's block: straight-line loads, nothing out of bounds) and their commit into LDS
    auto prefetch_state = [&](int t) {                                       // t = 0 .. T
        const float* __restrict__ xs = xs_k + (size_t)t * r.n * NS;
#pragma unroll
        for (int j = 0; j < NST; ++j) xs_nx[j] = xs[min(lane + 64 * j, lim - 1)];
    };
    auto prefetch = [&](int t) {                                             // t = 0 .. T - 1
        prefetch_state(t);
        const float* __restrict__ an = aw_k + (size_t)t * r.n * NA;
#pragma unroll
        for (int j = 0; j < NLD; ++j) a_nx[j] = an[min(lane + 64 * j, nact - 1)];
        w_nx = wt_k[(size_t)t * r.n];
    };
    auto commit_state = [&](float* dst) {
#pragma unroll
        for (int j = 0; j < NST; ++j) { const int i = lane + 64 * j; if (i < 16 * NS) dst[i] = (i < lim) ? xs_nx[j] : 0.0f; }
    };
    auto commit_act = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NA) { const float a = (i < nact) ? a_nx[j] : 0.0f; ARAW[i] = a; ACT[i] = fminf(fmaxf(a, -1.0f), 1.0f); }
        }
    };
    // x_T into buffer T & 1, then the rows of step T - 1
    prefetch_state(r.T);
    commit_state(W + (r.T & 1) * L::SB);
    prefetch(r.T - 1);
    commit_state(W + ((r.T - 1) & 1) * L::SB);
    commit_act();
    float w = active ? w_nx : 0.0f;
    wave_lds_sync();
    f32x4 lam[OUT_CB];
#pragma unroll
    for (int cb = 0; cb < OUT_CB; ++cb) lam[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the terminal value's seed, lambda_T = w_T dV/ds_T, from the x_T tile in lambda's own layout; w_T is the forward sweep's (WE)
    if constexpr (SEEDED) {
        const float* __restrict__ seed = tv_mlp_seed_of(r.WE, r.n, (int)gridDim.y) + ((size_t)k * r.n + min(lc, r.n - 1)) * NS;
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) lam[cb][rr] = active ? seed[dim] : 0.0f;
            }
    } else if (r.tv.set()) {
        const float* XT = W + (r.T & 1) * L::SB;
        const float wT = active ? r.WE[(size_t)k * r.n + min(lc, r.n - 1)] : 0.0f;
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) lam[cb][rr] = wT * r.tv.grad(dim, XT[c * NS + dim]);
            }
    }
    loop_invariant_loads_done();
    for (int t = r.T - 1; t >= 0; --t) {
        const float* ST = W + (t & 1) * L::SB;
        float* NX = W + ((t + 1) & 1) * L::SB;
        prefetch(max(t - 1, 0));                                             // committed behind the matrix instructions
        f32x4 h0[4], h1[4];
        float xin[C::NIN_KS];
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) xin[s] = in.get(ST, NS, ACT, c, s);
        head.layer0(h0, lds + L::O_BD0, xin, ReluBits());
        head.layer1(h1, lds + L::O_BD1, h0, ReluBits());
        // ---- cost adjoint of the RETURN in D layout: G = lambda_t+1 - w dc/dx_next (state dims), gU = -w dc/du (action dims) ----
        f32x4 G[OUT_CB], gU;
        env_cost_adjoint_d<ENV, NS, NA>(G, gU, lam, -w, NX + c * NS, ACT + c * NA, q);
        // ---- the head's adjoint chains, the clip gate on the head's own a_t and the store ----
        f32x4 gS[OUT_CB];
        adj.run(gS, gU, G, h0, h1);
        f32x4 gm;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int d = 4 * q + rr;
            gm[rr] = 0.0f;
            if (d < NA) {
                const float a = ARAW[c * NA + d];
                gm[rr] = (a >= -1.0f && a <= 1.0f) ? gU[rr] : 0.0f;
                if (active) r.grad[(((size_t)k * r.T + t) * r.B + b) * NA + d] = gm[rr] * sig[rr];
            }
        }
        // ---- the policy path: hidden layers of pi(s_t) recomputed, J_pi^T gm into gS ----
        f32x4 p0[2], p1[2];
        padj.hidden(p0, p1, ST, c);
        padj.run(gS, gm, p0, p1);
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb) lam[cb] = gS[cb];                // lambda_t
        wave_lds_sync();                                                     // every read of ST / NX / ACT / ARAW of this step is done
#pragma unroll
        for (int j = 0; j < NST; ++j) asm volatile("" ::"v"(xs_nx[j]));      // taken on every path (ActTile::commit): no wait at the loop's top
#pragma unroll
        for (int j = 0; j < NLD; ++j) asm volatile("" ::"v"(a_nx[j]));
        commit_state(NX);                                                    // x_t-1 takes x_t+1's place
        commit_act();
        w = active ? w_nx : 0.0f;
        wave_lds_sync();
    }
    if (r.lam0 != nullptr && active)
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) r.lam0[((size_t)k * r.B + b) * NS + dim] = lam[cb][rr];
            }
}

// -------------------------------------------------------------------------------------------------
// Generic path (sact_sum.h: GradBufs with the policy's rows).
// TV: with a terminal value -- a template parameter, so that the instantiation without one is the kernel it was (the runtime test costs it a stack slot)
template <int TV>
__global__ void k_spag_gen_fwd(ProblemDesc pd, SpagK r, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int lc = blockIdx.x * blockDim.x + tid, k = blockIdx.y, b = r.c0 + lc;
    const bool active = lc < r.n;
    const int ns = pd.ns, na = pd.na;
    GradBufs e = grad_carve(lds, pd, LD, true);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_mean = norm + 2 * (ns + na); const float* diff_std = diff_mean + ns;
    const float* __restrict__ pk = dynp + (size_t)k * pd.dyn.n_params;
    const float* __restrict__ log_std = theta + pd.pol.n_params;
    float* xs = r.XS + (size_t)k * (r.T + 1) * r.n * ns;
    for (int i = 0; i < ns; ++i) {
        const float v = active ? r.init_obs[(size_t)(b / r.per) * ns + i] : 0.0f;
        e.S[i * LD + tid] = v;
        if (active) xs[(size_t)lc * ns + i] = v;
    }
    SactSum acc;
    for (int t = 0; t < r.T; ++t) {
        const float* m = mlp_col(pd.pol, theta, e.S, e.GA, e.GB, LD, tid);
        for (int d = 0; d < na; ++d) {                       // k_policy_actions' action (noise in std units: its eps) or k_spol_act's mean + noise
            float a = m[d * LD + tid];
            if (r.noise != nullptr && active) {
                const float z = r.noise[((size_t)t * r.B + b) * na + d];
                a = r.in_std ? fmaf(z, __expf(fmaxf(log_std[d], LOG_MIN_STD)), a) : a + z;
            }
            if (active) {
                r.AW[(((size_t)k * r.T + t) * r.n + lc) * na + d] = a;
                if (r.act_out != nullptr) r.act_out[(((size_t)k * r.T + t) * r.B + b) * na + d] = a;
            }
            e.UR[d * LD + tid] = a;
        }
        for (int d = 0; d < na; ++d) e.U[d * LD + tid] = active ? fminf(fmaxf(e.UR[d * LD + tid], -1.0f), 1.0f) : 0.0f;
        for (int i = 0; i < ns; ++i) e.X[i * LD + tid] = (e.S[i * LD + tid] - in_mean[i]) / in_std[i];
        for (int d = 0; d < na; ++d) e.X[(ns + d) * LD + tid] = (e.U[d * LD + tid] - in_mean[ns + d]) / in_std[ns + d];
        float* out = mlp_col(pd.dyn, pk, e.X + pd.n_drop * LD, e.GA, e.GB, LD, tid);
        for (int i = 0; i < ns; ++i) e.XN[i * LD + tid] = fmaf(diff_std[i], out[i * LD + tid], diff_mean[i]) + e.S[i * LD + tid];
        const float cst = env_cost(pd.env, ns, na, env_col(e.XN, LD, tid), env_col(e.U, LD, tid));
        const bool dn = env_done_scan(pd.env, ns, env_col(e.XN, LD, tid));
        const float w = acc.step(-cst, dn, r.gamma, r.stop);
        if (active) {
            r.WT[((size_t)k * r.T + t) * r.n + lc] = w;
            for (int i = 0; i < ns; ++i) xs[((size_t)(t + 1) * r.n + lc) * ns + i] = e.XN[i * LD + tid];
        }
        for (int i = 0; i < ns; ++i) e.S[i * LD + tid] = e.XN[i * LD + tid];
    }
    if (active) {
        if (TV) r.WE[(size_t)k * r.n + lc] = acc.terminal(r.tv.template value_of<TV>(e.S + tid, LD, ns, b, r.per));      // S holds s_T behind the loop
        if (r.ret != nullptr) r.ret[(size_t)k * r.B + b] = (float)acc.sum;
        if (r.len != nullptr) r.len[(size_t)k * r.B + b] = acc.n;
    }
}

// SEEDED: as k_spag_bwd's
template <bool SEEDED>
__global__ void k_spag_gen_bwd(ProblemDesc pd, SpagK r, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int lc = blockIdx.x * blockDim.x + tid, k = blockIdx.y, b = r.c0 + lc;
    const bool active = lc < r.n;
    const int ns = pd.ns, na = pd.na;
    const NetDesc& dn = pd.dyn; const NetDesc& pn = pd.pol;
    GradBufs e = grad_carve(lds, pd, LD, true);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_std = norm + 2 * (ns + na) + ns;
    const float* __restrict__ pk = dynp + (size_t)k * dn.n_params;
    const float* __restrict__ log_std = theta + pn.n_params;
    const float* xs = r.XS + (size_t)k * (r.T + 1) * r.n * ns;
    for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = 0.0f;
    if constexpr (SEEDED) {
        const float* seed = tv_mlp_seed_of(r.WE, r.n, (int)gridDim.y) + ((size_t)k * r.n + lc) * ns;
        if (active) for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = seed[i];
    } else if (r.tv.set() && active) {                       // the terminal value's seed: lambda_T = w_T dV/ds_T; it reaches J_pi through G like any lambda
        const float wT = r.WE[(size_t)k * r.n + lc];
        for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = wT * r.tv.grad(i, xs[((size_t)r.T * r.n + lc) * ns + i]);
    }
    for (int t = r.T - 1; t >= 0; --t) {
        for (int i = 0; i < ns; ++i) {
            e.S[i * LD + tid] = active ? xs[((size_t)t * r.n + lc) * ns + i] : 0.0f;
            e.XN[i * LD + tid] = active ? xs[((size_t)(t + 1) * r.n + lc) * ns + i] : 0.0f;
        }
        const float w = active ? r.WT[((size_t)k * r.T + t) * r.n + lc] : 0.0f;
        // ---- recompute the step: the policy's hidden layers, the stored action and its clip, normalise, the head's hidden layers (all outputs kept) ----
        net_hidden(pn, theta, e.S, e.PH, LD, tid);
        for (int d = 0; d < na; ++d) {
            const float a = active ? r.AW[(((size_t)k * r.T + t) * r.n + lc) * na + d] : 0.0f;
            e.UR[d * LD + tid] = a;
            e.U[d * LD + tid] = fminf(fmaxf(a, -1.0f), 1.0f);
        }
        for (int i = 0; i < ns; ++i) e.X[i * LD + tid] = (e.S[i * LD + tid] - in_mean[i]) / in_std[i];
        for (int d = 0; d < na; ++d) e.X[(ns + d) * LD + tid] = (e.U[d * LD + tid] - in_mean[ns + d]) / in_std[ns + d];
        net_hidden(dn, pk, e.X + pd.n_drop * LD, e.DH, LD, tid);
        // ---- adjoints of the return: G = lambda_t+1 - w dc/dx_next; gU_cost = -w dc/du (in X's place: the normalised input is dead) ----
        float* G = e.LAM;
        float* gUc = e.X;
        env_cost_adjoint(pd.env, ns, na, e.XN, e.U, -w, gUc, G, LD, tid);
        for (int i = 0; i < ns; ++i) e.GA[i * LD + tid] = diff_std[i] * G[i * LD + tid];
        float* da = net_vjp(dn, pk, e.DH, e.GA, e.GB, LD, tid);
        float* db = (da == e.GA) ? e.GB : e.GA;
        // da = adjoint of the (dropped) normalised input [nin].  State part: residual + normaliser -> gS (x_next is dead now); action part -> gm behind the gate
        for (int i = 0; i < ns; ++i) {
            float v = G[i * LD + tid];
            if (i >= pd.n_drop) v += da[(i - pd.n_drop) * LD + tid] / in_std[i];
            e.XN[i * LD + tid] = v;
        }
        for (int d = 0; d < na; ++d) {
            const float gu = gUc[d * LD + tid] + da[(ns - pd.n_drop + d) * LD + tid] / in_std[ns + d];
            const float a = e.UR[d * LD + tid];
            const float gm = (a >= -1.0f && a <= 1.0f) ? gu : 0.0f;                 // tf.clip_by_value gradient
            db[d * LD + tid] = gm;
            if (active) r.grad[(((size_t)k * r.T + t) * r.B + b) * na + d] = r.in_std ? gm * __expf(fmaxf(log_std[d], LOG_MIN_STD)) : gm;
        }
        // ---- the policy path: J_pi(s_t)^T gm with the stored activations ----
        const float* pa = net_vjp(pn, theta, e.PH, db, da, LD, tid);
        for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = e.XN[i * LD + tid] + pa[i * LD + tid];       // lambda_t
    }
    if (r.lam0 != nullptr && active)
        for (int i = 0; i < ns; ++i) r.lam0[((size_t)k * r.B + b) * ns + i] = e.LAM[i * LD + tid];
}

// -------------------------------------------------------------------------------------------------
typedef void (*spag_kernel_t)(SpagK, const float*, const float*, const float*);
struct SpagEntry { int env; spag_kernel_t fwd[2][2], bwd[2]; int fwd_floats, bwd_floats; };      // fwd[the value is the MLP][noise], bwd[the value is the MLP]
#define GENTRY(ENVID) {ENVID, {{k_spag_fwd<ENVID, false>, k_spag_fwd<ENVID, true>}, {k_spag_fwd<ENVID, false, true>, k_spag_fwd<ENVID, true, true>}},   \
                       {k_spag_bwd<ENVID>, k_spag_bwd<ENVID, true>}, pol_wave_floats<ENVID>(), SpagL<ENVID>::TOTAL}
static const SpagEntry kSpag[] = {FUSED_HEAD_ENVS(GENTRY)};

int run_score_policy_actions_grad(metrpo_ctx* c, const metrpo_score_policy_actions_grad_args* a, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const size_t ns = pd.ns, na = pd.na, B = a->B, T = a->T, K = pd.K;
    bool padded = false;
    const SpagEntry* en = a->force_generic ? nullptr : fused_head_entry(kSpag, c, 65535, &padded);      // the heads are gridDim.y; the class holds the 2 x 32 tanh policy
    // ---- a chunk's workspace (floats): XS [K][T + 1][Bc][ns] | WT [K][T][Bc] | AW [K][T][Bc][na] | (a terminal value is set) WE [K][Bc] | (it is the MLP) its seed [K][Bc][ns];
    // within 2^26 floats unless args.chunk says otherwise ----
    const TermVal tv = ctx_term_val(c);
    const bool mlp = ctx_tv_kind(c) == TV_MLP;
    const size_t per_cand = K * ((T + 1) * ns + T + T * na + (tv.w1 ? 1 : 0) + (mlp ? ns : 0));
    const size_t Bc = score_chunk(B, per_cand, (size_t)a->chunk);
    const size_t o_wt = (K * (T + 1) * Bc * ns + 3) & ~(size_t)3, o_aw = (o_wt + K * T * Bc + 3) & ~(size_t)3;
    const size_t o_we = o_aw + K * T * Bc * na;
    { const int rc = ws_grow(c, c->d_spag, sizeof(float) * (o_we + (tv.w1 ? K * Bc : 0) + (mlp ? K * Bc * ns : 0))); if (rc) return rc; }
    float* ws = (float*)c->d_spag.p;
    SpagK r = {};
    r.B = a->B; r.T = a->T; r.per = a->B / a->S; r.stop = a->stop_at_done ? 1 : 0; r.in_std = a->noise_in_std ? 1 : 0; r.gamma = a->gamma;
    r.init_obs = a->d_init_obs; r.noise = a->d_noise; r.XS = ws; r.WT = ws + o_wt; r.AW = ws + o_aw; r.WE = tv.w1 ? ws + o_we : nullptr; r.tv = tv;
    r.ret = a->d_ret; r.len = a->d_len; r.act_out = a->d_act_out; r.grad = a->d_grad; r.lam0 = a->d_lam0;
    const float* dyn = c->d_dyn.p;
    size_t sh_f = 0, sh_b = 0;
    int bs = 64;
    spag_kernel_t fwd = nullptr;
    void (*gen_fwd)(ProblemDesc, SpagK, const float*, const float*, const float*) = nullptr;
    void (*gen_bwd)(ProblemDesc, SpagK, const float*, const float*, const float*) = nullptr;
    if (en != nullptr) {
        { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
        fwd = en->fwd[mlp ? 1 : 0][a->d_noise != nullptr ? 1 : 0];
        sh_f = sizeof(float) * (size_t)en->fwd_floats; sh_b = sizeof(float) * (size_t)en->bwd_floats;
        int rc = allow_dynamic_lds(c, (const void*)fwd, sh_f);
        if (!rc) rc = allow_dynamic_lds(c, (const void*)en->bwd[mlp ? 1 : 0], sh_b);
        if (rc) return rc;
    } else {
        const size_t fpt = grad_gen_floats(pd, true);
        if ((bs = lds_block_size(fpt)) == 0) return set_err(c, METRPO_EUNSUPPORTED, "score_policy_actions_grad: layer widths exceed the LDS budget of the generic kernel");
        sh_f = sh_b = fpt * bs * sizeof(float);
        gen_fwd = mlp ? k_spag_gen_fwd<TV_MLP> : (tv.w1 ? k_spag_gen_fwd<TV_QUAD> : k_spag_gen_fwd<TV_NONE>);
        gen_bwd = mlp ? k_spag_gen_bwd<true> : k_spag_gen_bwd<false>;
        int rc = allow_dynamic_lds(c, (const void*)gen_fwd, sh_f);
        if (!rc) rc = allow_dynamic_lds(c, (const void*)gen_bwd, sh_b);
        if (rc) return rc;
    }
    for (size_t c0 = 0; c0 < B; c0 += Bc) {
        r.c0 = (int)c0; r.n = (int)std::min(Bc, B - c0);
        if (en != nullptr) {
            hipLaunchKernelGGL(fwd, dim3((r.n + 15) / 16, (unsigned)K), dim3(64), sh_f, st, r, dyn, c->d_theta.p, c->d_norm.p);
            if (mlp) launch_tv_mlp_seed(tv, r.XS, r.WE, tv_mlp_seed_of(r.WE, r.n, (int)K), (int)K, r.T, r.n, (int)ns, st);
            hipLaunchKernelGGL(en->bwd[mlp ? 1 : 0], dim3((r.n + 63) / 64, (unsigned)K), dim3(256), sh_b, st, r, dyn, c->d_theta.p, c->d_norm.p);
        } else {
            const dim3 grid((r.n + bs - 1) / bs, (unsigned)K);
            hipLaunchKernelGGL(gen_fwd, grid, dim3(bs), sh_f, st, pd, r, dyn, c->d_theta.p, c->d_norm.p);
            if (mlp) launch_tv_mlp_seed(tv, r.XS, r.WE, tv_mlp_seed_of(r.WE, r.n, (int)K), (int)K, r.T, r.n, (int)ns, st);
            hipLaunchKernelGGL(gen_bwd, grid, dim3(bs), sh_b, st, pd, r, dyn, c->d_theta.p, c->d_norm.p);
        }
        HIP_TRY(c, hipGetLastError());
    }
    if (a->d_grad_mean != nullptr) {
        launch_sagr_mean(a->d_grad, T * B * na, (int)K, a->d_grad_mean, st);
        HIP_TRY(c, hipGetLastError());
    }
    c->last_spag_kernel = en != nullptr ? 1 : 0;
    return METRPO_OK;
}
