// Transposed MFMA chain of the 2 x 32 tanh policies (every shipped params file except Humanoid) on a fragment image in LDS: the two-hidden-layer
// sibling of policy_chain3.h.  One wave per 16-env tile, every layer's D fragment is the next layer's B operand, 30 matrix instructions.  The
// image's layout, the gather that fills it from theta and the chain are stated here once for the wide-net pre-steps: k_big_pre_mfma
// (rollout_gemm.hip) and the persistent stream-K rollout's closing role (big_prepost.h, mlp_persist.h), k_dg_pre_mfma (det_gemm.hip) and the two
// post roles of rollout_resident.hip.
// The 2 x 32 chains that still stand alone: PolWaveHead::mean on register fragments and PolHeadAdjoint::hidden on its own table order
// (pol_head_mfma.h), the cooperative rollout's body (rollout_coop_body.h), and the three-hidden-layer policy_chain3.h.
#pragma once
#include "mfma_common.h"

// C = Cfg<ENV, 64, 32>.  Lane l = (env c = l & 15, quarter q = l >> 4).
// LDS image (floats): W0 fragments [NS_KS][2][64] | W1 fragments [8][2][64] | Wout fragments [8][64] | b0 [32] | b1 [32] | bout [16]
template <class C>
struct P2 {
    static constexpr int NS = C::NS, NA = C::NA, PH = 32, NS_KS = C::NS_KS;
    static constexpr int O_PF1 = NS_KS * 2 * 64, O_PF2 = O_PF1 + 16 * 64, O_B0 = O_PF2 + 8 * 64, O_B1 = O_B0 + 32, O_B2 = O_B1 + 32, IMG = O_B2 + 16;
    static_assert(IMG % 4 == 0, "whatever follows the image in LDS stays 16-byte aligned");
    // value of image entry i (a gather from the flat policy vector, rllab order); 0 for every i >= IMG
    static __device__ __forceinline__ float entry(const float* __restrict__ theta, int i) {
        float w = 0.0f;
        const int ln = i & 63, cc = ln & 15, qq = ln >> 4;
        if (i < O_PF1) { const int f = i >> 6, s_ = f >> 1, cb = f & 1, in = 4 * s_ + qq; if (in < NS) w = theta[C::pW0 + in * PH + 16 * cb + cc]; }
        else if (i < O_PF2) { const int f = (i - O_PF1) >> 6, kk = f >> 1, cb = f & 1; w = theta[C::pW1 + (16 * (kk >> 2) + 4 * qq + (kk & 3)) * PH + 16 * cb + cc]; }
        else if (i < O_B0) { const int kk = (i - O_PF2) >> 6; if (cc < NA) w = theta[C::pW2 + (16 * (kk >> 2) + 4 * qq + (kk & 3)) * NA + cc]; }
        else if (i < O_B1) w = theta[C::pb0 + (i - O_B0)];
        else if (i < O_B2) w = theta[C::pb1 + (i - O_B1)];
        else { const int d = i - O_B2; if (d < NA) w = theta[C::pb2 + d]; }
        return w;
    }
    // the image into LDS by nthr threads (the caller's barrier follows)
    static __device__ __forceinline__ void fill(float* lds, const float* __restrict__ theta, int tid, int nthr) {
        for (int i = tid; i < IMG; i += nthr) lds[i] = entry(theta, i);
    }
    // mean of the policy for the wave's 16 envs: mu[r] = action dim 4 q + r of env c.  x(s_) = this lane's B value of layer 0's k-step s_:
    // state dim 4 s_ + q of env c, zero beyond NS.
    template <class X>
    static __device__ __forceinline__ f32x4 mean(const float* img, int lane, X x) {
        const int q = lane >> 4;
        f32x4 p0[2], p1[2];
        p0[0] = *(const f32x4*)&img[O_B0 + 4 * q]; p0[1] = *(const f32x4*)&img[O_B0 + 16 + 4 * q];
#pragma unroll
        for (int s_ = 0; s_ < NS_KS; ++s_) {
            const float xs = x(s_);
            p0[0] = MFMA16(img[(s_ * 2 + 0) * 64 + lane], xs, p0[0]);
            p0[1] = MFMA16(img[(s_ * 2 + 1) * 64 + lane], xs, p0[1]);
        }
        p1[0] = *(const f32x4*)&img[O_B1 + 4 * q]; p1[1] = *(const f32x4*)&img[O_B1 + 16 + 4 * q];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p0[cb][rr] = tanh_fast(p0[cb][rr]);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            p1[0] = MFMA16(img[O_PF1 + (kk * 2 + 0) * 64 + lane], p0[kk >> 2][kk & 3], p1[0]);
            p1[1] = MFMA16(img[O_PF1 + (kk * 2 + 1) * 64 + lane], p0[kk >> 2][kk & 3], p1[1]);
        }
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) p1[cb][rr] = tanh_fast(p1[cb][rr]);
        f32x4 m0 = *(const f32x4*)&img[O_B2 + 4 * q], m1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; kk += 2) {
            m0 = MFMA16(img[O_PF2 + kk * 64 + lane], p1[kk >> 2][kk & 3], m0);
            m1 = MFMA16(img[O_PF2 + (kk + 1) * 64 + lane], p1[(kk + 1) >> 2][(kk + 1) & 3], m1);
        }
        return m0 + m1;
    }
    // the same on the wave's LDS state tile ST [16][NS]
    static __device__ __forceinline__ f32x4 mean_tile(const float* img, const float* ST, int lane) {
        const int c = lane & 15, q = lane >> 4;
        return mean(img, lane, [&](int s_) { const int f = 4 * s_ + q; return (f < NS) ? ST[c * NS + f] : 0.0f; });
    }
};
