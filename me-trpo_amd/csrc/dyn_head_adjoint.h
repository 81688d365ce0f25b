// The adjoint of one dynamics head of dyn_head_mfma.h for a tile of 16 envs, on the same transposed v_mfma_f32_16x16x4_f32 chains: given the adjoint G of
// the head's de-normalised next state (D layout: register [cb][r] of lane (e, q) is state dim 16 cb + 4 q + r of env e) and the recomputed hidden
// activations h0, h1 of the step, it returns
//   gS = G + (state rows of F^T G)       the residual identity x' = x + ... is the initial value of the last chain
//   gU += (action rows of F^T G)         lane (e, q), register r = action dim 4 q + r of env e
// with F the head's Jacobian including both normalisers and the column drop.  Users: the reverse sweeps k_det_mfma<DET_BWD> (bptt_mfma.hip), k_sagr<.., SAGR_BWD>
// (score_actions_grad.hip) and k_spag_bwd (score_policy_actions_grad.hip); each places the table in its own LDS image and calls fill() in front of its barrier.
//   adjoint   dX^T[in][env] = W . dH^T      A = W fragments (an LDS table shared by the waves of a workgroup), B = deltas in D layout of the next layer
// Constant factors are folded into the fragments: diff_std into the first adjoint layer, 1/in_std and the column drop into the last one, which is split
// into a state part (rows = state dims: lands in the layout of the residual path) and an action part (rows = action dims).  relu'(h) = [h > 0].
// The hidden width is the 64 of the fused kernels' layout (narrower nets come zero-padded: a padded unit has h = 0 and passes nothing).
#pragma once
#include "dyn_head_mfma.h"

template <class C>
struct DynHeadAdjoint {
    static constexpr int NS = C::NS, NA = C::NA, NDROP = C::NDROP, OUT_CB = C::OUT_CB, DH = 64;
    static_assert(C::DYN_H == 64 && C::DH_CB == 4, "the adjoint tables are laid out for the 64-unit layout");
    // table (floats): [k-step][col-block][64 lanes] per layer
    static constexpr int O_DB2 = 0, O_DB1 = O_DB2 + 4 * OUT_CB * 4 * 64, O_DAS = O_DB1 + 16 * 4 * 64, O_DAA = O_DAS + 16 * OUT_CB * 64,
                         FLOATS = O_DAA + 16 * 64;
    const float* tab;
    int lane;

    // every thread of the workgroup calls it (nthr threads, thread tid); each element is written by one thread; the caller's barrier follows
    static __device__ __forceinline__ void fill(float* tab, const float* __restrict__ pk, const float* __restrict__ norm, int tid, int nthr) {
        const float* in_std = norm + (NS + NA);
        const float* dstd_p = norm + 2 * (NS + NA) + NS;
        for (int i = tid; i < FLOATS; i += nthr) {
            float w = 0.0f;
            const int ln = i & 63, cc = ln & 15, qq = ln >> 4;
            if (i < O_DB1) {                     // first adjoint layer: k-steps (cb, r) over state dims, diff_std folded in
                const int f = (i - O_DB2) >> 6, ks = f >> 2, cb = f & 3, dim = chained_in(ks, qq);
                if (dim < NS) w = pk[C::dW2 + (16 * cb + cc) * NS + dim] * dstd_p[dim];
            } else if (i < O_DAS) {
                const int f = (i - O_DB1) >> 6, kk = f >> 2, cb = f & 3;
                w = pk[C::dW1 + (16 * cb + cc) * DH + chained_in(kk, qq)];
            } else if (i < O_DAA) {              // last adjoint layer, state rows: column drop and 1/in_std folded in
                const int f = (i - O_DAS) >> 6, kk = f / OUT_CB, cb = f % OUT_CB, dim = 16 * cb + cc;
                if (dim >= NDROP && dim < NS) w = pk[C::dW0 + (dim - NDROP) * DH + chained_in(kk, qq)] / in_std[dim];
            } else {                             // last adjoint layer, action rows
                const int kk = (i - O_DAA) >> 6;
                if (cc < NA) w = pk[C::dW0 + (NS - NDROP + cc) * DH + chained_in(kk, qq)] / in_std[NS + cc];
            }
            tab[i] = w;
        }
    }

    __device__ __forceinline__ float frag(int off, int ks, int cb, int ncb) const { return tab[off + (ks * ncb + cb) * 64 + lane]; }

    // d2 = W2.(diff_std G) * relu'(h1); d1 = W1.d2 * relu'(h0); gS = G + W0s.d1; gU += W0a.d1
    __device__ __forceinline__ void run(f32x4 (&gS)[OUT_CB], f32x4& gU, const f32x4 (&G)[OUT_CB], const f32x4 (&h0)[4], const f32x4 (&h1)[4]) const {
        f32x4 d2[4], d1[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) d2[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4 * OUT_CB; ++ks)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) d2[cb] = MFMA16(frag(O_DB2, ks, cb, 4), G[ks >> 2][ks & 3], d2[cb]);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            d1[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) d2[cb][r] = (h1[cb][r] > 0.0f) ? d2[cb][r] : 0.0f;
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) d1[cb] = MFMA16(frag(O_DB1, kk, cb, 4), d2[kk >> 2][kk & 3], d1[cb]);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) d1[cb][r] = (h0[cb][r] > 0.0f) ? d1[cb][r] : 0.0f;
#pragma unroll
        for (int cb = 0; cb < OUT_CB; ++cb) gS[cb] = G[cb];                           // residual connection x' = x + ...
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
            for (int cb = 0; cb < OUT_CB; ++cb) gS[cb] = MFMA16(frag(O_DAS, kk, cb, OUT_CB), d1[kk >> 2][kk & 3], gS[cb]);
            gU = MFMA16(tab[O_DAA + kk * 64 + lane], d1[kk >> 2][kk & 3], gU);
        }
    }
};
