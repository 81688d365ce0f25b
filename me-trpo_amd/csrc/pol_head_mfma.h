// The mean net of the 2 x 32 tanh policy ([rllab] GaussianMLPPolicy.get_actions, the mean half) for a tile of 16 envs, TRANSPOSED on
// v_mfma_f32_16x16x4_f32 in the fragment layout of dyn_head_mfma.h: the one-time fragment and bias load and the per-step chain (tanh_fast and the two
// accumulators of the last layer included) of a wave that evaluates the whole policy itself, stated once as a type.  Users: k_rollout_mfma (rollout_mfma.hip),
// k_score_policy_actions (score_policy_actions.hip) and k_spag_fwd (score_policy_actions_grad.hip).  The wide-net pre-steps (big_prepost.h, mlp_persist.h,
// det_gemm.hip, the post roles of rollout_resident.hip) run the chain on an image in LDS: policy_chain2.h.  rollout_coop_body.h and policy_chain3.h pipeline
// it differently and state their own.
//   PolWaveHead     a wave's policy: weight fragments in registers (swimmer 6 + 16 + 8, Ant 16 + 16 + 8), its three bias rows in LDS;
//                   mean() = the mean's action dims 4 q .. 4 q + 3 of env e in D layout
//   NoiseTile       the tile's noise block, double-buffered in LDS and committed unclipped (ActTile's prefetch)
//   PolHeadAdjoint  the policy's input adjoint J_pi(s)^T gm on fragment tables in LDS (at the end of this file; score_policy_actions_grad.hip)
// No LDS is declared here: every pointer into it is the caller's.  Lane l = (e = l & 15, q = l >> 4).
#pragma once
#include "dyn_head_mfma.h"
#include "dyn_tile_step.h"

// per-wave LDS (floats) of a tile that runs the policy AND a dynamics head under supplied noise: Cfg<>'s whole W_* layout -- ST | NX | ACT | dynamics
// biases | policy biases at W_BP0 .. W_BP2 (act_wave_floats<> reuses W_BP0 as its second action buffer; here the bias rows are needed) -- and the second
// noise buffer behind W_TOTAL
template <int ENV> constexpr int pol_wave_floats() { return al4(Cfg<ENV, 64, 32>::W_TOTAL) + al4(16 * Cfg<ENV, 64, 32>::NA); }

template <class C>
struct PolWaveHead {
    static constexpr int NS = C::NS, NA = C::NA, PH = C::pW1 - C::pb0;           // hidden width of the policy (Cfg<>'s flat layout: b0 has PH entries)
    float wp0[C::NS_KS][C::PH_CB], wp1[C::PH_CB * 4][C::PH_CB], wp2[C::PH_CB * 4];
    const float *bp0, *bp1, *bp2;                // the wave's own LDS rows: [BP] [BP] [16]
    int q;

    // theta: the flat policy parameters (Cfg<>'s pW0 .. pb2); bias rows -> LDS, padded entries zero
    __device__ __forceinline__ void load(const float* __restrict__ theta, float* bp0_, float* bp1_, float* bp2_, int lane) {
        const int e = lane & 15;
        q = lane >> 4;
#pragma unroll
        for (int s = 0; s < C::NS_KS; ++s)
#pragma unroll
            for (int cb = 0; cb < C::PH_CB; ++cb) {
                const int i = 4 * s + q, o = 16 * cb + e;
                wp0[s][cb] = (i < NS && o < PH) ? theta[C::pW0 + i * PH + o] : 0.0f;
            }
#pragma unroll
        for (int kk = 0; kk < C::PH_CB * 4; ++kk) {
            const int i = chained_in(kk, q);
#pragma unroll
            for (int cb = 0; cb < C::PH_CB; ++cb) {
                const int o = 16 * cb + e;
                wp1[kk][cb] = (i < PH && o < PH) ? theta[C::pW1 + i * PH + o] : 0.0f;
            }
            wp2[kk] = (i < PH && e < NA) ? theta[C::pW2 + i * NA + e] : 0.0f;
        }
        for (int i = lane; i < C::BP; i += 64) {
            bp0_[i] = (i < PH) ? theta[C::pb0 + i] : 0.0f;
            bp1_[i] = (i < PH) ? theta[C::pb1 + i] : 0.0f;
        }
        if (lane < 16) bp2_[lane] = (lane < NA) ? theta[C::pb2 + lane] : 0.0f;
        bp0 = bp0_; bp1 = bp1_; bp2 = bp2_;
    }
    // mean = MLP(s) of env e from its LDS state row ST[e * NS ..]: register r is action dim 4 q + r (zero on the padded dims)
    __device__ __forceinline__ f32x4 mean(const float* ST, int e) const {
        f32x4 p0[C::PH_CB], p1[C::PH_CB];
#pragma unroll
        for (int cb = 0; cb < C::PH_CB; ++cb) p0[cb] = *(const f32x4*)&bp0[16 * cb + 4 * q];
#pragma unroll
        for (int s = 0; s < C::NS_KS; ++s) {
            const int f = 4 * s + q;
            const float x = (f < NS) ? ST[e * NS + f] : 0.0f;
#pragma unroll
            for (int cb = 0; cb < C::PH_CB; ++cb) p0[cb] = MFMA16(wp0[s][cb], x, p0[cb]);
        }
#pragma unroll
        for (int cb = 0; cb < C::PH_CB; ++cb) {
            p1[cb] = *(const f32x4*)&bp1[16 * cb + 4 * q];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p0[cb][rr] = tanh_fast(p0[cb][rr]);
        }
#pragma unroll
        for (int kk = 0; kk < C::PH_CB * 4; ++kk)
#pragma unroll
            for (int cb = 0; cb < C::PH_CB; ++cb) p1[cb] = MFMA16(wp1[kk][cb], p0[kk >> 2][kk & 3], p1[cb]);
#pragma unroll
        for (int cb = 0; cb < C::PH_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p1[cb][rr] = tanh_fast(p1[cb][rr]);
        f32x4 m0 = *(const f32x4*)&bp2[4 * q], m1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < C::PH_CB * 4; kk += 2) {              // two accumulators: half the dependent chain
            m0 = MFMA16(wp2[kk], p1[kk >> 2][kk & 3], m0);
            m1 = MFMA16(wp2[kk + 1], p1[(kk + 1) >> 2][(kk + 1) & 3], m1);
        }
        return m0 + m1;
    }
};

// The noise block of a tile ([16][NA] of d_noise [T][B][na] at rows b0 ..): ActTile's two LDS buffers and its prefetch, committed UNCLIPPED (the
// action is clipped where it is formed).  Rows at and beyond nrows are zero noise and are never read from memory.
template <class C>
struct NoiseTile : ActTile<C> {
    using A = ActTile<C>;
    __device__ __forceinline__ void commit(int t) {
        float* dst = A::cur(t);
#pragma unroll
        for (int j = 0; j < A::NLD; ++j) asm volatile("" ::"v"(A::a_nx[j]));   // the loaded values are taken on every path (ActTile::commit)
#pragma unroll
        for (int j = 0; j < A::NLD; ++j) {
            const int i = A::lane + 64 * j;
            if (i < 16 * A::NA) dst[i] = (i < A::nact) ? A::a_nx[j] : 0.0f;
        }
    }
};

// The policy's INPUT adjoint for a tile of 16 envs, on the same transposed chains: given the adjoint gm of the (pre-clip) mean (D layout: register r of lane
// (e, q) is action dim 4 q + r of env e) it adds J_pi(s)^T gm into gS (D layout of the state, as DynHeadAdjoint returns it).  Users: k_det_mfma (bptt_mfma.hip:
// both sweeps take hidden() as the policy's two tanh layers, and form the mean's last layer from a table of their own behind this image; the reverse sweep
// calls run() behind the clip gate) and k_spag_bwd (score_policy_actions_grad.hip).
//   hidden()  p0, p1 = the two tanh layers of env e from its LDS state row: PolWaveHead::mean's statements on LDS fragments (the mean itself is not formed)
//   run()     e1 = W2 . gm * (1 - p1^2);  e0 = W1 . e1 * (1 - p0^2);  gS += W0 . e0
// The fragment tables and the two hidden bias rows are one LDS image shared by the waves of a workgroup.
template <class C>
struct PolHeadAdjoint {
    static constexpr int NS = C::NS, NA = C::NA, OUT_CB = C::OUT_CB, NS_KS = C::NS_KS, PH = 32;
    static_assert(C::PH_CB == 2 && C::pW1 - C::pb0 == PH, "the tables are laid out for the 2 x 32 policy");
    static constexpr int RK = (NA < 4) ? NA : 4;                       // k-steps of the first adjoint layer that are not padding
    // table (floats): [k-step][col-block][64 lanes] per layer, then the bias rows of the hidden layers
    static constexpr int O_PF0 = 0, O_PF1 = O_PF0 + NS_KS * 2 * 64, O_PB2 = O_PF1 + 8 * 2 * 64, O_PB1 = O_PB2 + RK * 2 * 64, O_PB0 = O_PB1 + 8 * 2 * 64,
                         O_BP0 = O_PB0 + 8 * OUT_CB * 64, O_BP1 = O_BP0 + PH, FLOATS = O_BP1 + PH;
    const float* tab;
    int lane;

    // every thread of the workgroup calls it (nthr threads, thread tid); each element is written by one thread; the caller's barrier follows
    static __device__ __forceinline__ void fill(float* tab, const float* __restrict__ theta, int tid, int nthr) {
        for (int i = tid; i < FLOATS; i += nthr) {
            float w = 0.0f;
            const int ln = i & 63, cc = ln & 15, qq = ln >> 4;
            if (i < O_PF1) { const int f = i >> 6, s = f >> 1, cb = f & 1, in = 4 * s + qq; if (in < NS) w = theta[C::pW0 + in * PH + 16 * cb + cc]; }
            else if (i < O_PB2) { const int f = (i - O_PF1) >> 6, kk = f >> 1, cb = f & 1; w = theta[C::pW1 + chained_in(kk, qq) * PH + 16 * cb + cc]; }
            else if (i < O_PB1) { const int f = (i - O_PB2) >> 6, r = f >> 1, cb = f & 1, d = 4 * qq + r; if (d < NA) w = theta[C::pW2 + (16 * cb + cc) * NA + d]; }
            else if (i < O_PB0) { const int f = (i - O_PB1) >> 6, kk = f >> 1, cb = f & 1; w = theta[C::pW1 + (16 * cb + cc) * PH + chained_in(kk, qq)]; }
            else if (i < O_BP0) { const int f = (i - O_PB0) >> 6, kk = f / OUT_CB, cb = f % OUT_CB, dim = 16 * cb + cc; if (dim < NS) w = theta[C::pW0 + dim * PH + chained_in(kk, qq)]; }
            else if (i < O_BP1) w = theta[C::pb0 + (i - O_BP0)];
            else w = theta[C::pb1 + (i - O_BP1)];
            tab[i] = w;
        }
    }

    __device__ __forceinline__ float frag(int off, int ks, int cb, int ncb) const { return tab[off + (ks * ncb + cb) * 64 + lane]; }

    __device__ __forceinline__ void hidden(f32x4 (&p0)[2], f32x4 (&p1)[2], const float* ST, int e) const {
        const int q = lane >> 4;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) p0[cb] = *(const f32x4*)&tab[O_BP0 + 16 * cb + 4 * q];
#pragma unroll
        for (int s = 0; s < NS_KS; ++s) {
            const int f = 4 * s + q;
            const float x = (f < NS) ? ST[e * NS + f] : 0.0f;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) p0[cb] = MFMA16(frag(O_PF0, s, cb, 2), x, p0[cb]);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            p1[cb] = *(const f32x4*)&tab[O_BP1 + 16 * cb + 4 * q];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p0[cb][rr] = tanh_fast(p0[cb][rr]);
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) p1[cb] = MFMA16(frag(O_PF1, kk, cb, 2), p0[kk >> 2][kk & 3], p1[cb]);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p1[cb][rr] = tanh_fast(p1[cb][rr]);
    }

    __device__ __forceinline__ void run(f32x4 (&gS)[OUT_CB], const f32x4& gm, const f32x4 (&p0)[2], const f32x4 (&p1)[2]) const {
        f32x4 e1[2], e0[2];
        e1[0] = e1[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < RK; ++r)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) e1[cb] = MFMA16(frag(O_PB2, r, cb, 2), gm[r], e1[cb]);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            e0[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) e1[cb][r] *= fmaf(-p1[cb][r], p1[cb][r], 1.0f);
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) e0[cb] = MFMA16(frag(O_PB1, kk, cb, 2), e1[kk >> 2][kk & 3], e0[cb]);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) e0[cb][r] *= fmaf(-p0[cb][r], p0[cb][r], 1.0f);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int cb = 0; cb < OUT_CB; ++cb) gS[cb] = MFMA16(frag(O_PB0, kk, cb, OUT_CB), e0[kk >> 2][kk & 3], gS[cb]);
    }
};
