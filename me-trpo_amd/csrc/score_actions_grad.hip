// metrpo_score_actions_grad (include/metrpo.h): for every head k and candidate b the gradient of the head's predicted discounted RETURN
//   R = -sum_t w_t cost_tf(s_t, clip(a_t), s_t+1),   w_t = gamma^t alive_t        (metrpo_score_actions' ret: model_based_rl.py:122-141 under supplied actions)
// with respect to the UNCLIPPED candidate actions a_t (d_grad [K][T][B][na]) and the start state (d_lam0 [K][B][ns]).  Reverse recursion from lambda_T = 0:
//   G = lambda_t+1 - w_t dc/dx_next;  gU = -w_t dc/du + (action rows of F^T G);  lambda_t = G + (state rows of F^T G);  grad_t = gU gated by -1 <= a_t <= 1
// The conventions are the BPTT sweep's (bptt.hip): relu'(h) = [h > 0], env_model.h's adjoint terms, the alive mask a constant of the differentiation.
//
// Fused path: TWO stream-ordered launches of k_sagr<ENV, MODE> (the second launch sees the first one's stores without any in-kernel fence), per chunk of
// candidates.  This is k_det_mfma's structure (bptt_mfma.hip) with the policy chain removed; the departures from it are marked (*).
//   SAGR_FWD  k_score_actions' mapping and body: one wave per (16-candidate tile, head), one-wave workgroups, dyn_tile_step.h's tile_rollout -- so s', r, ret
//             and len carry that kernel's bits -- with a sink that keeps SactSum's sum per lane and additionally stores, per step, the tile's state block
//             into XS [K][T+1][Bc][ns] as one linear store and the fp32 weight into WT [K][T][Bc].  ret / len are written once behind the loop.
//   SAGR_BWD  a workgroup is 4 waves = four 16-candidate tiles of the SAME head (blockIdx.y), launch bound (256, 2): the head's adjoint fragment tables
//             (dyn_head_adjoint.h: 28 KB swimmer .. 36 KB Ant) are one LDS image per workgroup; one per wave would cap a CU at four or five waves.
//             Per step t = T-1 .. 0: layers 0 and 1 recomputed on DynHeadFrags<C, false> from XS[t] (same statements, same bits as the forward sweep, so
//             the relu masks are the forward's), cost adjoint in D layout, the three adjoint chains, clip gate, store of grad[k][t], lambda in registers.
//         (*) prefetch: x_t+1 of step t IS x_t of step t + 1, so a step loads ONE state block, XS[t-1], plus the action block and weight of step t-1.  They
//             are issued at the top of step t and wait in registers (<= 8 + 2 + 1 per lane) behind the step's matrix instructions; at the end of the step
//             they are committed into the state buffer that x_t+1 has just vacated (two state buffers alternate) and into the one action buffer.  A second
//             LDS action buffer is therefore not needed: nothing reads the buffers between the last use of step t and the commit.
//   Edge tile: rows at and beyond the chunk's end are zeros in LDS, never read from or written to memory (the forward sweep computes rows of a later chunk
//   that share its last tile and drops them: rows are independent columns of the matrix instructions, so chunking changes no bit).  The start rows are
//   gathered per row (a tile may straddle two start states).
//
// Generic path (every other shape, and force_generic): k_sagr_gen_fwd / k_sagr_gen_bwd, one thread per (candidate, head) with activations in LDS
// columns (sact_sum.h: GradBufs; device_common.h: net_hidden, net_vjp; env_model.h: env_cost_adjoint) -- k_bptt_forward / k_bptt_backward (bptt.hip) with the policy removed; block size by
// lds_block_size (metrpo_internal.h).  Same outputs, workspace, chunking.
//
// Terminal value (metrpo_set_terminal_value; sact_sum.h: TermVal): the forward sweeps add gamma^T alive_T V(s_T) to the sum behind the loop (score_actions.hip's
// statement, so ret keeps that call's bits) and STORE w_T = alive_T ? (float)gamma^T : 0 into WE [K][Bc], one more slice of WT that exists only while a value is
// set -- stored, not re-derived: the reverse sweep would have to redo the done test of s_T and the float64 discount to form it.  The reverse sweeps start from
// lambda_T = w_T dV/ds_T, formed from the stored XS[T] tile in lambda's own layout (fused: the x_T buffer in LDS, behind its commit) instead of 0.  The forward
// sweeps take the value as a template parameter (k_sagr<.., SAGR_FWD, TV>, k_sagr_gen_fwd<TV>), the reverse sweeps by the runtime-uniform pointer test.
// The MLP form (metrpo_set_terminal_value_mlp) is TV_MLP of the same parameter in the forward sweeps; its seed is formed by a launch of its own between the two
// sweeps (k_tv_mlp_seed: XS[T], WE -> seed [K][Bc][ns] behind WE), and the reverse sweeps' TV_MLP / SEEDED instantiations read it in front of their loop.
//
// Workspace: ctx->d_sagr = XS | WT (| WE) of one chunk, within 2^26 floats (score_chunk, metrpo_internal.h; args.chunk > 0 overrides).  d_grad_mean: k_sagr_mean, a small
// launch over d_grad adding in head order (k_sact_aggregate's style).  No atomics anywhere: repeated calls are bit-identical.
#include "dyn_tile_step.h"
#include "dyn_head_adjoint.h"
#include "sact_sum.h"
#include <algorithm>
#include <cmath>

enum { SAGR_FWD = 0, SAGR_BWD = 1 };

struct SagrK {
    int B, T, per;            // per = B / S: candidates per start state
    int stop;                 // 1: a candidate stops counting behind its first done
    int c0, n;                // the chunk: candidates c0 .. c0 + n - 1; XS / WT hold n columns
    double gamma;
    const float* init_obs; const float* actions;
    float* XS; float* WT;     // [K][T+1][n][ns], [K][T][n]
    float* WE;                // [K][n]: w_T, one more slice of WT, only while a terminal value is set
    TermVal tv;               // the context's terminal value; unset: all NULL
    float* ret; int32_t* len; // [K][B], optional
    float* grad; float* lam0; // [K][T][B][na], optional [K][B][ns]
};

// tile_rollout's sink of the forward sweep: b0 is the tile's first candidate in the batch, the chunk's column is b - c0
template <int NS, int TV>
struct SagrSink {
    const SagrK& r;
    int k;
    SactSum acc;
    __device__ __forceinline__ int lim(int b0) const { return min(16, r.c0 + r.n - b0) * NS; }      // floats of the tile's rows inside the chunk
    __device__ __forceinline__ void rows(int t, const float* ST, int b0, int lane) const {
        float* dst = r.XS + (((size_t)k * (r.T + 1) + t) * r.n + (b0 - r.c0)) * NS;
        const int l = lim(b0);
        for (int i = lane; i < l; i += 64) dst[i] = ST[i];
    }
    __device__ __forceinline__ void start(const float* ST, int b0, int, int lane) const { rows(0, ST, b0, lane); }
    __device__ __forceinline__ void step(int t, const float* ST, float cost, bool dn, int b0, int, int lane) {
        const float w = acc.step(-cost, dn, r.gamma, r.stop);
        const int b = b0 + (lane & 15);
        if ((lane >> 4) == 0 && b < r.c0 + r.n) r.WT[((size_t)k * r.T + t) * r.n + (b - r.c0)] = w;
        rows(t + 1, ST, b0, lane);
    }
    // ST: the tile's rows behind the loop, s_T.  The terminal value once per lane, in front of the single rounding; its weight w_T into WE
    __device__ __forceinline__ void finish(int b0, int lane, const float* ST) {
        const int b = b0 + (lane & 15);
        if ((lane >> 4) == 0 && b < r.c0 + r.n) {
            if (TV) r.WE[(size_t)k * r.n + (b - r.c0)] = acc.terminal(r.tv.template value_of<TV>(ST + (lane & 15) * NS, 1, NS, b, r.per));
            const size_t kb = (size_t)k * r.B + b;
            if (r.ret != nullptr) r.ret[kb] = (float)acc.sum;
            if (r.len != nullptr) r.len[kb] = acc.n;
        }
    }
};

// LDS of the reverse sweep (floats): adjoint tables | bias rows of layers 0, 1 | per wave: two state buffers, the clipped and the raw action block
template <int ENV>
struct SagrL {
    using C = Cfg<ENV, 64, 32>;
    using A = DynHeadAdjoint<C>;
    static constexpr int O_BD0 = A::FLOATS, O_BD1 = O_BD0 + 64, IMG = O_BD1 + 64;
    static constexpr int SB = al4(16 * C::NS), AB = al4(16 * C::NA), WV = 2 * SB + 2 * AB;
    static constexpr int TOTAL = IMG + 4 * WV;
};

// TV: the forward sweep with a terminal value.  A template parameter there, not the runtime-uniform pointer test of the other kernels: the test's
// operands live in scalar registers across the step loop, the Ant instantiation has none to spare, and what spills costs it a wave per SIMD.
// TV is the value's kind (sact_sum.h: TV_NONE, TV_QUAD, TV_MLP).  The reverse sweep knows two: TV_NONE, the kernel it was, with the runtime test for the quadratic
// form; TV_MLP, which reads lambda_T from the workspace behind WE (k_tv_mlp_seed below wrote it: the net's 64 hidden values have no room beside this sweep's fragments).
template <int ENV, int MODE, int TV = TV_NONE>
__global__ void __launch_bounds__(MODE == SAGR_FWD ? 64 : 256, MODE == SAGR_FWD ? 1 : 2)
k_sagr(SagrK r, const float* __restrict__ dynp, const float* __restrict__ norm) {
    using L = SagrL<ENV>;
    using C = typename L::C;
    constexpr int NS = C::NS, NA = C::NA, OUT_CB = C::OUT_CB, NST = cdiv(16 * NS, 64), NLD = cdiv(16 * NA, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int k = blockIdx.y;
    if constexpr (MODE == SAGR_FWD) {
        // ------------------------------------------------ forward sweep: k_score_actions' body, a storing sink ------------------------------------------------
        const int b0 = r.c0 + blockIdx.x * 16;
        const TileRollK tr = {r.B, r.T, r.per, r.init_obs, r.actions, k, 0, nullptr};
        SagrSink<NS, TV> sink = {r, k};
        tile_rollout<ENV, true>(lds, tr, 1, b0, dynp, norm, sink);
        sink.finish(b0, threadIdx.x & 63, lds + C::W_ST);
    } else {
        // ------------------------------------------------ reverse sweep ------------------------------------------------
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const int c = lane & 15, q = lane >> 4;
        const float* __restrict__ pk = dynp + (size_t)k * C::PD;
        L::A::fill(lds, pk, norm, tid, 256);
        for (int i = tid; i < 64; i += 256) { lds[L::O_BD0 + i] = pk[C::db0 + i]; lds[L::O_BD1 + i] = pk[C::db1 + i]; }
        DynHeadFrags<C, false> head;                                             // layers 0 and 1 only
        DynInNorm<C> in;
        head.load(pk, c, q);
        in.load(norm, q);
        __syncthreads();                                                         // the only barrier: the tables are read-only from here on
        const int l0 = (blockIdx.x * 4 + wave) * 16;                             // the tile's first column of the chunk
        if (l0 >= r.n) return;
        const typename L::A adj = {lds, lane};
        float* W = lds + L::IMG + wave * L::WV;
        float* ACT = W + 2 * L::SB; float* ARAW = ACT + L::AB;
        const int nrows = min(16, r.n - l0), lim = nrows * NS, nact = nrows * NA;
        const int lc = l0 + c, b = r.c0 + lc;                                    // this lane's column of the chunk / candidate of the batch
        const bool active = c < nrows;
        const float* __restrict__ xs_k = r.XS + ((size_t)k * (r.T + 1) * r.n + l0) * NS;      // + t n NS: the tile's rows of slice t, linear
        const float* __restrict__ wt_k = r.WT + (size_t)k * r.T * r.n + min(lc, r.n - 1);     // + t n
        const float* __restrict__ act_b = r.actions + (size_t)(r.c0 + l0) * NA;                // + t B NA: the tile's action block of step t, linear
        float xs_nx[NST], a_nx[NLD], w_nx;
        // the loads of step t's rows (clamped into the tile's block: straight-line loads, nothing out of bounds) and their commit into LDS
        auto prefetch_state = [&](int t) {                                       // t = 0 .. T
            const float* __restrict__ xs = xs_k + (size_t)t * r.n * NS;
#pragma unroll
            for (int j = 0; j < NST; ++j) xs_nx[j] = xs[min(lane + 64 * j, lim - 1)];
        };
        auto prefetch = [&](int t) {                                             // t = 0 .. T - 1
            prefetch_state(t);
            const float* __restrict__ an = act_b + (size_t)t * r.B * NA;
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
        if constexpr (TV == TV_MLP) {
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
            // ---- the head's adjoint chains, the clip gate (tf.clip_by_value passes the gradient inside [min, max]) and the store ----
            f32x4 gS[OUT_CB];
            adj.run(gS, gU, G, h0, h1);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int d = 4 * q + rr;
                if (d < NA && active) {
                    const float a = ARAW[c * NA + d];
                    r.grad[(((size_t)k * r.T + t) * r.B + b) * NA + d] = (a >= -1.0f && a <= 1.0f) ? gU[rr] : 0.0f;
                }
            }
#pragma unroll
            for (int cb = 0; cb < OUT_CB; ++cb) lam[cb] = gS[cb];                // lambda_t
            wave_lds_sync();                                                     // every read of NX / ACT / ARAW of this step is done
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
}

// -------------------------------------------------------------------------------------------------
// Generic path (sact_sum.h: GradBufs without the policy's rows).
// TV: with a terminal value -- a template parameter, so that the instantiation without one is the kernel it was (the runtime test costs it a stack slot)
template <int TV>
__global__ void k_sagr_gen_fwd(ProblemDesc pd, SagrK r, const float* __restrict__ dynp, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int lc = blockIdx.x * blockDim.x + tid, k = blockIdx.y, b = r.c0 + lc;
    const bool active = lc < r.n;
    const int ns = pd.ns, na = pd.na;
    GradBufs e = grad_carve(lds, pd, LD, false);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_mean = norm + 2 * (ns + na); const float* diff_std = diff_mean + ns;
    const float* __restrict__ pk = dynp + (size_t)k * pd.dyn.n_params;
    float* xs = r.XS + (size_t)k * (r.T + 1) * r.n * ns;
    for (int i = 0; i < ns; ++i) {
        const float v = active ? r.init_obs[(size_t)(b / r.per) * ns + i] : 0.0f;
        e.S[i * LD + tid] = v;
        if (active) xs[(size_t)lc * ns + i] = v;
    }
    SactSum acc;
    for (int t = 0; t < r.T; ++t) {
        for (int d = 0; d < na; ++d) e.U[d * LD + tid] = active ? fminf(fmaxf(r.actions[((size_t)t * r.B + b) * na + d], -1.0f), 1.0f) : 0.0f;
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

// SEEDED: the MLP form -- lambda_T is read from the workspace behind WE (k_tv_mlp_seed); without it the kernel it was
template <bool SEEDED>
__global__ void k_sagr_gen_bwd(ProblemDesc pd, SagrK r, const float* __restrict__ dynp, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = blockDim.x, tid = threadIdx.x;
    const int lc = blockIdx.x * blockDim.x + tid, k = blockIdx.y, b = r.c0 + lc;
    const bool active = lc < r.n;
    const int ns = pd.ns, na = pd.na;
    const NetDesc& dn = pd.dyn;
    GradBufs e = grad_carve(lds, pd, LD, false);
    const float* in_mean = norm; const float* in_std = norm + (ns + na);
    const float* diff_std = norm + 2 * (ns + na) + ns;
    const float* __restrict__ pk = dynp + (size_t)k * dn.n_params;
    const float* xs = r.XS + (size_t)k * (r.T + 1) * r.n * ns;
    for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = 0.0f;
    if constexpr (SEEDED) {
        const float* seed = tv_mlp_seed_of(r.WE, r.n, (int)gridDim.y) + ((size_t)k * r.n + lc) * ns;
        if (active) for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = seed[i];
    } else if (r.tv.set() && active) {                       // the terminal value's seed: lambda_T = w_T dV/ds_T
        const float wT = r.WE[(size_t)k * r.n + lc];
        for (int i = 0; i < ns; ++i) e.LAM[i * LD + tid] = wT * r.tv.grad(i, xs[((size_t)r.T * r.n + lc) * ns + i]);
    }
    for (int t = r.T - 1; t >= 0; --t) {
        for (int i = 0; i < ns; ++i) {
            e.S[i * LD + tid] = active ? xs[((size_t)t * r.n + lc) * ns + i] : 0.0f;
            e.XN[i * LD + tid] = active ? xs[((size_t)(t + 1) * r.n + lc) * ns + i] : 0.0f;
        }
        const float w = active ? r.WT[((size_t)k * r.T + t) * r.n + lc] : 0.0f;
        // ---- recompute the step: clip, normalise, the hidden layers (all outputs kept) ----
        for (int d = 0; d < na; ++d) {
            const float a = active ? r.actions[((size_t)t * r.B + b) * na + d] : 0.0f;
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
        const float* da = net_vjp(dn, pk, e.DH, e.GA, e.GB, LD, tid);
        // da = adjoint of the (dropped) normalised input [nin].  Action part -> the gated gradient; state part: residual + normaliser -> lambda_t
        for (int d = 0; d < na; ++d) {
            const float gu = gUc[d * LD + tid] + da[(ns - pd.n_drop + d) * LD + tid] / in_std[ns + d];
            const float a = e.UR[d * LD + tid];
            if (active) r.grad[(((size_t)k * r.T + t) * r.B + b) * na + d] = (a >= -1.0f && a <= 1.0f) ? gu : 0.0f;    // tf.clip_by_value gradient
        }
        for (int i = 0; i < ns; ++i) {
            float v = G[i * LD + tid];
            if (i >= pd.n_drop) v += da[(i - pd.n_drop) * LD + tid] / in_std[i];
            e.LAM[i * LD + tid] = v;
        }
    }
    if (r.lam0 != nullptr && active)
        for (int i = 0; i < ns; ++i) r.lam0[((size_t)k * r.B + b) * ns + i] = e.LAM[i * LD + tid];
}

// d_grad_mean [n] from d_grad [K][n] (n = T B na): summed in head order, divided by K (k_sact_aggregate's mean)
__global__ void __launch_bounds__(256) k_sagr_mean(const float* __restrict__ grad, size_t n, int K, float* __restrict__ mean) {
    const float fK = (float)K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = 0.0f;
        for (int k = 0; k < K; ++k) s += grad[(size_t)k * n + i];
        mean[i] = s / fK;
    }
}

// ... for score_policy_actions_grad.hip as well (metrpo_internal.h); it reports no error of its own
void launch_sagr_mean(const float* grad, size_t n, int K, float* mean, hipStream_t st) {
    hipLaunchKernelGGL(k_sagr_mean, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, grad, n, K, mean);
}

// The MLP terminal value's seed of one chunk, between the forward and the reverse sweep: one thread per (column of the chunk, head k = blockIdx.y),
// seed [K][n][ns] = w_T dV/ds_T from the stored slice T of XS and the stored w_T (WE).  The reverse sweeps find it behind WE (sact_sum.h: tv_mlp_seed_of).
__global__ void __launch_bounds__(64) k_tv_mlp_seed(TermVal tv, const float* __restrict__ XS, const float* __restrict__ WE, float* __restrict__ seed, int T, int n, int ns) {
    const int lc = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (lc >= n) return;
    const float* sT = XS + (((size_t)k * (T + 1) + T) * n + lc) * ns;
    const float wT = WE[(size_t)k * n + lc];
    float g0[TVM];
    tv.mlp_adjoint(sT, 1, ns, g0);
    float* out = seed + ((size_t)k * n + lc) * ns;
    for (int d = 0; d < ns; ++d) out[d] = wT * tv.mlp_grad(d, sT[d], g0);
}
void launch_tv_mlp_seed(const TermVal& tv, const float* XS, const float* WE, float* seed, int K, int T, int n, int ns, hipStream_t st) {
    hipLaunchKernelGGL(k_tv_mlp_seed, dim3((n + 63) / 64, (unsigned)K), dim3(64), 0, st, tv, XS, WE, seed, T, n, ns);
}

// -------------------------------------------------------------------------------------------------
typedef void (*sagr_kernel_t)(SagrK, const float*, const float*);
struct SagrEntry { int env; sagr_kernel_t fwd[3], bwd[2]; int fwd_floats, bwd_floats; };      // fwd[the terminal value's kind], bwd[it is the MLP]
#define GENTRY(ENVID) {ENVID, {k_sagr<ENVID, SAGR_FWD>, k_sagr<ENVID, SAGR_FWD, TV_QUAD>, k_sagr<ENVID, SAGR_FWD, TV_MLP>}, {k_sagr<ENVID, SAGR_BWD>, k_sagr<ENVID, SAGR_BWD, TV_MLP>},   \
                       act_wave_floats<ENVID>(), SagrL<ENVID>::TOTAL}
static const SagrEntry kSagr[] = {FUSED_HEAD_ENVS(GENTRY)};

int run_score_actions_grad(metrpo_ctx* c, const metrpo_score_actions_grad_args* a, hipStream_t st) {
    const ProblemDesc& pd = c->pd;
    const size_t ns = pd.ns, B = a->B, T = a->T, K = pd.K;
    bool padded = false;
    const SagrEntry* en = a->force_generic ? nullptr : fused_head_entry(kSagr, c, 65535, &padded);      // the heads are gridDim.y
    // ---- a chunk's workspace (floats): XS [K][T + 1][Bc][ns] | WT [K][T][Bc] | (a terminal value is set) WE [K][Bc] | (it is the MLP) its seed [K][Bc][ns];
    // within 2^26 floats unless args.chunk says otherwise ----
    const TermVal tv = ctx_term_val(c);
    const int kind = ctx_tv_kind(c);
    const bool mlp = kind == TV_MLP;
    const size_t per_cand = K * ((T + 1) * ns + T + (tv.w1 ? 1 : 0) + (mlp ? ns : 0));
    const size_t Bc = score_chunk(B, per_cand, (size_t)a->chunk);
    const size_t o_wt = (K * (T + 1) * Bc * ns + 3) & ~(size_t)3;
    const size_t o_we = o_wt + K * T * Bc;
    { const int rc = ws_grow(c, c->d_sagr, sizeof(float) * (o_we + (tv.w1 ? K * Bc : 0) + (mlp ? K * Bc * ns : 0))); if (rc) return rc; }
    float* ws = (float*)c->d_sagr.p;
    SagrK r = {};
    r.B = a->B; r.T = a->T; r.per = a->B / a->S; r.stop = a->stop_at_done ? 1 : 0; r.gamma = a->gamma;
    r.init_obs = a->d_init_obs; r.actions = a->d_actions; r.XS = ws; r.WT = ws + o_wt; r.WE = tv.w1 ? ws + o_we : nullptr; r.tv = tv;
    r.ret = a->d_ret; r.len = a->d_len; r.grad = a->d_grad; r.lam0 = a->d_lam0;
    const float* dyn = c->d_dyn.p;
    size_t sh_f = 0, sh_b = 0;
    int bs = 64;
    void (*gen_fwd)(ProblemDesc, SagrK, const float*, const float*) = nullptr;
    void (*gen_bwd)(ProblemDesc, SagrK, const float*, const float*) = nullptr;
    if (en != nullptr) {
        { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
        sh_f = sizeof(float) * (size_t)en->fwd_floats; sh_b = sizeof(float) * (size_t)en->bwd_floats;
        { const int rc = allow_dynamic_lds(c, (const void*)en->bwd[mlp ? 1 : 0], sh_b); if (rc) return rc; }
    } else {
        const size_t fpt = grad_gen_floats(pd, false);
        if ((bs = lds_block_size(fpt)) == 0) return set_err(c, METRPO_EUNSUPPORTED, "score_actions_grad: layer widths exceed the LDS budget of the generic kernel");
        sh_f = sh_b = fpt * bs * sizeof(float);
        gen_fwd = mlp ? k_sagr_gen_fwd<TV_MLP> : (tv.w1 ? k_sagr_gen_fwd<TV_QUAD> : k_sagr_gen_fwd<TV_NONE>);
        gen_bwd = mlp ? k_sagr_gen_bwd<true> : k_sagr_gen_bwd<false>;
        int rc = allow_dynamic_lds(c, (const void*)gen_fwd, sh_f);
        if (!rc) rc = allow_dynamic_lds(c, (const void*)gen_bwd, sh_b);
        if (rc) return rc;
    }
    for (size_t c0 = 0; c0 < B; c0 += Bc) {
        r.c0 = (int)c0; r.n = (int)std::min(Bc, B - c0);
        if (en != nullptr) {
            hipLaunchKernelGGL(en->fwd[kind], dim3((r.n + 15) / 16, (unsigned)K), dim3(64), sh_f, st, r, dyn, c->d_norm.p);
            if (mlp) launch_tv_mlp_seed(tv, r.XS, r.WE, tv_mlp_seed_of(r.WE, r.n, (int)K), (int)K, r.T, r.n, (int)ns, st);
            hipLaunchKernelGGL(en->bwd[mlp ? 1 : 0], dim3((r.n + 63) / 64, (unsigned)K), dim3(256), sh_b, st, r, dyn, c->d_norm.p);
        } else {
            const dim3 grid((r.n + bs - 1) / bs, (unsigned)K);
            hipLaunchKernelGGL(gen_fwd, grid, dim3(bs), sh_f, st, pd, r, dyn, c->d_norm.p);
            if (mlp) launch_tv_mlp_seed(tv, r.XS, r.WE, tv_mlp_seed_of(r.WE, r.n, (int)K), (int)K, r.T, r.n, (int)ns, st);
            hipLaunchKernelGGL(gen_bwd, grid, dim3(bs), sh_b, st, pd, r, dyn, c->d_norm.p);
        }
        HIP_TRY(c, hipGetLastError());
    }
    if (a->d_grad_mean != nullptr) {
        launch_sagr_mean(a->d_grad, T * B * pd.na, (int)K, a->d_grad_mean, st);
        HIP_TRY(c, hipGetLastError());
    }
    c->last_sagr_kernel = en != nullptr ? 1 : 0;
    return METRPO_OK;
}
