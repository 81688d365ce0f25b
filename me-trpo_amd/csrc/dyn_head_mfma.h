// One dynamics head of the ensemble (training.py:218-269) for a tile of 16 envs, TRANSPOSED on v_mfma_f32_16x16x4_f32: the one statement of
// what rollout_mfma.hip, bptt_mfma.hip and dyn_tile_step.h (for rollout_actions.hip, score_actions.hip and disagreement.hip) instantiate (all three
// pieces) and rollout_coop_kernel.h (the two normalisers; its layers are split across waves with a fragment layout of its own).
//
// Layout.  Lane l = (e = l & 15, q = l >> 4).  Every layer is H^T[unit][env] = W^T . X^T:
//   A = weights      lane l holds W[in = k-step's input of q][out = 16 cb + e]
//   B = activations  lane l holds x[in = k-step's input of q] of env e
//   D = result       lane l holds units 16 cb + 4 q + r (r = 0..3) of env e
// Layer 0 enumerates its inputs linearly: k-step s contracts inputs 4 s + q.  The D fragment of a layer IS the B operand of the next when that
// layer's k-steps are enumerated as kk = (cb, r) and contract input chained_in(kk, q) -- activations never leave registers between layers.
// f32 MFMA is an exact fmaf chain, so the numerics are plain fp32 and the order of the k-steps on an accumulator is the order of its sums:
// ascending everywhere, layer 2 with even kk on one accumulator and odd kk on a second (half the dependent chain), added at the end.
//
// Everything here is registers: no LDS is declared, biases and state rows are the caller's (pointers passed in).
#pragma once
#include "mfma_common.h"

// input unit that k-step kk of a chained layer contracts in lane group q: the unit the previous layer's D fragment holds in block kk >> 2, register kk & 3
__device__ __forceinline__ constexpr int chained_in(int kk, int q) { return 16 * (kk >> 2) + 4 * q + (kk & 3); }

// the two spellings of the hidden ReLU in use; they differ on NaN and on -0, every kernel keeps its own
struct ReluFmax { __device__ __forceinline__ float operator()(float x) const { return fmaxf(x, 0.0f); } };
struct ReluBits { __device__ __forceinline__ float operator()(float x) const { return relu1(x); } };

// Input side (training.py:228): k-step s of layer 0 contracts network input i = 4 s + q, which is state feature i + n_drop, or action dim
// i - (ns - n_drop), or padding behind NIN.  norm = in_mean[ns + na] | in_std[ns + na] | diff_mean[ns] | diff_std[ns].
template <class C>
struct DynInNorm {
    static constexpr int PAD = -1000000;         // src of a padding input; any other negative src is -(action dim + 1)
    int src[C::NIN_KS];                          // >= 0: state feature
    float mean[C::NIN_KS], rstd[C::NIN_KS];

    __device__ __forceinline__ void load(const float* __restrict__ norm, int q) {
        constexpr int NS = C::NS, NA = C::NA;
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) {
            const int i = 4 * s + q;
            int f = 0;
            if (i < NS - C::NDROP) { f = i + C::NDROP; src[s] = f; }
            else if (i < C::NIN) { f = NS + (i - (NS - C::NDROP)); src[s] = -(i - (NS - C::NDROP)) - 1; }
            else { src[s] = PAD; }
            mean[s] = (i < C::NIN) ? norm[f] : 0.0f;
            rstd[s] = (i < C::NIN) ? 1.0f / norm[(NS + NA) + f] : 1.0f;   // reciprocal: (x - mean) * (1/std), <= 1 ulp from the division
        }
    }
    // normalised layer-0 operand of k-step s for env e; ST rows are st_stride floats apart, ACT rows NA
    __device__ __forceinline__ float get(const float* ST, int st_stride, const float* ACT, int e, int s) const {
        float x = 0.0f;
        if (src[s] >= 0) x = ST[e * st_stride + src[s]];
        else if (src[s] > PAD) x = ACT[e * C::NA + (-src[s] - 1)];
        return (src[s] > PAD) ? (x - mean[s]) * rstd[s] : 0.0f;           // (xgu - in_mean)/in_std
    }
    // the same for a k-step below (NS - NDROP) / 4, whose four inputs are all state features: no select, usable before the action exists
    __device__ __forceinline__ float get_state(const float* ST, int st_stride, int e, int s) const {
        return (ST[e * st_stride + src[s]] - mean[s]) * rstd[s];
    }
};

// Output side (training.py:257), in D layout: register [cb][r] is state dim 16 cb + 4 q + r; zero on the padded dims.
template <class C>
struct DynOutNorm {
    f32x4 dmean[C::OUT_CB], dstd[C::OUT_CB];

    __device__ __forceinline__ void load(const float* __restrict__ norm, int q) {
        constexpr int NS = C::NS, NA = C::NA;
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int dim = 16 * cb + 4 * q + r;
                dmean[cb][r] = (dim < NS) ? norm[2 * (NS + NA) + dim] : 0.0f;
                dstd[cb][r] = (dim < NS) ? norm[2 * (NS + NA) + NS + dim] : 0.0f;
            }
    }
    // diff_mean + diff_std * out + s
    __device__ __forceinline__ float apply(int cb, int r, float o, float s) const { return fmaf(dstd[cb][r], o, dmean[cb][r]) + s; }
    __device__ __forceinline__ f32x4 apply(int cb, f32x4 o, f32x4 s) const {
        f32x4 n;
#pragma unroll
        for (int r = 0; r < 4; ++r) n[r] = apply(cb, r, o[r], s[r]);
        return n;
    }
};

// Register-resident weight fragments of one head and its three layers.  WITH_W2 = false leaves layer 2 out (its fragments are not loaded).
template <class C, bool WITH_W2 = true>
struct DynHeadFrags {
    static constexpr int DH = C::DYN_H, KS = C::DH_CB * 4;                       // hidden width; k-steps of a chained layer
    float wd0[C::NIN_KS][C::DH_CB], wd1[KS][C::DH_CB], wd2[WITH_W2 ? KS : 1][C::OUT_CB];
    int q;

    // pk: the head's W0 b0 W1 b1 W2 b2 (Cfg<>'s dW0 .. db2).  The guards on the hidden width fold away when it is a multiple of 16.
    __device__ __forceinline__ void load(const float* __restrict__ pk, int e, int q_) {
        q = q_;
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s)
#pragma unroll
            for (int cb = 0; cb < C::DH_CB; ++cb) {
                const int i = 4 * s + q, o = 16 * cb + e;
                wd0[s][cb] = (i < C::NIN && o < DH) ? pk[C::dW0 + i * DH + o] : 0.0f;
            }
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int i = chained_in(kk, q);
#pragma unroll
            for (int cb = 0; cb < C::DH_CB; ++cb) {
                const int o = 16 * cb + e;
                wd1[kk][cb] = (i < DH && o < DH) ? pk[C::dW1 + i * DH + o] : 0.0f;
            }
            if constexpr (WITH_W2) {
#pragma unroll
                for (int cb = 0; cb < C::OUT_CB; ++cb) {
                    const int o = 16 * cb + e;
                    wd2[kk][cb] = (i < DH && o < C::NS) ? pk[C::dW2 + i * C::NS + o] : 0.0f;
                }
            }
        }
    }
    // h0 = act(b0 + W0^T x): bias0[DH_CB * 16] enters as the C operand, xin[s] is the operand of k-step s (DynInNorm::get)
    template <class Act>
    __device__ __forceinline__ void layer0(f32x4 (&h0)[C::DH_CB], const float* bias0, const float (&xin)[C::NIN_KS], Act act) const {
#pragma unroll
        for (int cb = 0; cb < C::DH_CB; ++cb) h0[cb] = *(const f32x4*)&bias0[16 * cb + 4 * q];
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) {
            const float x = xin[s];
#pragma unroll
            for (int cb = 0; cb < C::DH_CB; ++cb) h0[cb] = MFMA16(wd0[s][cb], x, h0[cb]);
        }
        activate(h0, act);
    }
    // h1 = act(b1 + W1^T h0)
    template <class Act>
    __device__ __forceinline__ void layer1(f32x4 (&h1)[C::DH_CB], const float* bias1, const f32x4 (&h0)[C::DH_CB], Act act) const {
#pragma unroll
        for (int cb = 0; cb < C::DH_CB; ++cb) h1[cb] = *(const f32x4*)&bias1[16 * cb + 4 * q];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
#pragma unroll
            for (int cb = 0; cb < C::DH_CB; ++cb) h1[cb] = MFMA16(wd1[kk][cb], h0[kk >> 2][kk & 3], h1[cb]);
        activate(h1, act);
    }
    // b2 + W2^T h1 = oa + ob: even k-steps (and the bias, bias2[NSP]) on oa, odd ones on ob
    __device__ __forceinline__ void layer2(f32x4 (&oa)[C::OUT_CB], f32x4 (&ob)[C::OUT_CB], const float* bias2, const f32x4 (&h1)[C::DH_CB]) const {
        static_assert(WITH_W2, "layer 2 needs its fragments");
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb) { oa[cb] = *(const f32x4*)&bias2[16 * cb + 4 * q]; ob[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int kk = 0; kk < KS; kk += 2)
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb) {
                oa[cb] = MFMA16(wd2[kk][cb], h1[kk >> 2][kk & 3], oa[cb]);
                ob[cb] = MFMA16(wd2[kk + 1][cb], h1[(kk + 1) >> 2][(kk + 1) & 3], ob[cb]);
            }
    }

private:
    template <class Act>
    static __device__ __forceinline__ void activate(f32x4 (&h)[C::DH_CB], Act act) {
#pragma unroll
        for (int cb = 0; cb < C::DH_CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[cb][r] = act(h[cb][r]);
    }
};
