// The mean net of the 2 x 32 tanh policy ([rllab] GaussianMLPPolicy.get_actions, the mean half) for a tile of 16 envs, TRANSPOSED on
// v_mfma_f32_16x16x4_f32 in the fragment layout of dyn_head_mfma.h: the statements of rollout_mfma.hip's policy chain (its one-time fragment and bias
// load and its per-step chain, tanh_fast and the two accumulators of the last layer included) stated once as a type.  score_policy_actions.hip is
// its first user; the kernels that carry their own copy of the chain keep it.
//   PolWaveHead     a wave's policy: weight fragments in registers (swimmer 6 + 16 + 8, Ant 16 + 16 + 8), its three bias rows in LDS;
//                   mean() = the mean's action dims 4 q .. 4 q + 3 of env e in D layout
// No LDS is declared here: every pointer into it is the caller's.  Lane l = (e = l & 15, q = l >> 4).
#pragma once
#include "dyn_head_mfma.h"

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
