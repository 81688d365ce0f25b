// The per-candidate return of metrpo_score_actions and metrpo_score_policy_actions (include/metrpo.h): what score_actions.hip's and
// score_policy_actions.hip's fused kernels carry per lane and what k_sact_reduce applies to a stored trajectory.
// Below it: what the generic kernels of the two gradient files (score_actions_grad.hip, score_policy_actions_grad.hip) share: their LDS columns (a net's hidden layers, its
// vector-Jacobian product are device_common.h's, the cost adjoint is env_model.h's).
#pragma once
#include "device_common.h"

// The terminal value of metrpo_set_terminal_value (include/metrpo.h): LinearFeatureBaseline's form with its time features evaluated at a fixed step,
//   o_d = clip(s_d, -10, 10);  V(s) = bias + sum_d (w1[d] o_d + w2[d] o_d^2)
// w1 == nullptr: no terminal value is set.  The kernels read it once per lane BEHIND the step loop, never inside it.  Who tests the pointer (runtime-uniform):
// both reverse sweeps (k_sagr<.., SAGR_BWD>, k_spag_bwd, k_sagr_gen_bwd, k_spag_gen_bwd), k_spag_fwd and k_sact_reduce.  Who takes `set` as a template parameter
// TV instead: k_score_actions, k_score_policy_actions, k_sagr<.., SAGR_FWD, TV>, k_sagr_gen_fwd, k_spag_gen_fwd (why each: profiles/r26_terminal_value.txt).
// Candidate b uses bias[n_bias > 1 ? b / per : 0] (per = B / S).
// The second form, metrpo_set_terminal_value_mlp's two-layer tanh net, is TV_MLP of that template parameter, and a template parameter of its own in the
// kernels of the first list (MLP / SEEDED; their instantiations without it are the kernels they were: profiles/r33_terminal_mlp.txt).
enum { TV_NONE = 0, TV_QUAD = 1, TV_MLP = 2 };               // metrpo_terminal_value_kind's values
// The MLP form's image in d_tv (floats), hidden widths padded with zeros to TVM: W0 [ns][TVM] | b0 [TVM] | W1 OUT-major [TVM][TVM] | b1 [TVM] | W2 [TVM] | b2, 3 unused | bias [n_bias]
constexpr int TVM = 32;
__host__ __device__ constexpr int tvm_b0(int ns) { return ns * TVM; }
__host__ __device__ constexpr int tvm_w1(int ns) { return tvm_b0(ns) + TVM; }
__host__ __device__ constexpr int tvm_b1(int ns) { return tvm_w1(ns) + TVM * TVM; }
__host__ __device__ constexpr int tvm_w2(int ns) { return tvm_b1(ns) + TVM; }
__host__ __device__ constexpr int tvm_floats(int ns) { return tvm_w2(ns) + TVM + 4; }
struct TermVal {
    const float* w1; const float* w2; const float* bias;      // [ns], [ns], [n_bias]: context-owned copies
    int n_bias;                                               // 1, or S
    __device__ __forceinline__ bool set() const { return w1 != nullptr; }
    __device__ __forceinline__ float bias_of(int b, int per) const { return bias[n_bias > 1 ? b / per : 0]; }
    // V of the state s[0], s[stride], ..: fp32, dims in order
    __device__ __forceinline__ float value(const float* s, int stride, int ns, int b, int per) const {
        float v = bias_of(b, per);
        for (int d = 0; d < ns; ++d) {
            const float o = fminf(fmaxf(s[d * stride], -10.0f), 10.0f);
            v = fmaf(o, fmaf(w2[d], o, w1[d]), v);
        }
        return v;
    }
    // dV/ds_d at s_d: tf.clip_by_value passes the gradient inside [min, max] (the action clip's convention)
    __device__ __forceinline__ float grad(int d, float sd) const { return (sd >= -10.0f && sd <= 10.0f) ? fmaf(2.0f * w2[d], sd, w1[d]) : 0.0f; }

    // ---- the second form, metrpo_set_terminal_value_mlp: a two-layer tanh net on the clipped state,
    //   p0 = tanh(W0^T o + b0);  p1 = tanh(W1^T p0 + b1);  V(s) = bias + (b2 + sum_j W2[j] p1[j])
    // The struct is the same (so no kernel argument moves): w1 points at the context's zero-padded TVM x TVM image (tvm_* below), w2 is NULL, bias and
    // n_bias as above.  WHICH form is set is never tested on the device: it is the template parameter TV (TV_QUAD / TV_MLP) of the forward kernels, and the
    // reverse sweeps read the MLP's seed from the workspace, where k_tv_mlp_seed (score_actions_grad.hip) wrote it.  Every sum starts from its bias and adds
    // by fmaf in input order; the loops over a layer's inputs are compile-time, so layer 0's row is TVM registers; the weights are lane-uniform reads.
    // Padding is exact: tanh_fast(0) = 0 and a zero weight adds an exact zero.
    // layer 0: p0 = tanh(W0^T o + b0), the row of TVM registers both directions start from.  One state dim per trip (never unrolled: a trip is TVM
    // lane-uniform weights and TVM multiply-adds; unrolled over the dims, the weights of every trip would be live at once)
    __device__ __forceinline__ void mlp_layer0(const float* s, int stride, int ns, float (&p0)[TVM]) const {
        const float* W0 = w1; const float* b0 = w1 + tvm_b0(ns);
#pragma unroll
        for (int i = 0; i < TVM; ++i) p0[i] = b0[i];
#pragma unroll 1
        for (int d = 0; d < ns; ++d) {
            const float o = fminf(fmaxf(s[d * stride], -10.0f), 10.0f);
#pragma unroll
            for (int i = 0; i < TVM; ++i) p0[i] = fmaf(W0[d * TVM + i], o, p0[i]);
        }
#pragma unroll
        for (int i = 0; i < TVM; ++i) p0[i] = tanh_fast(p0[i]);
    }
    // unit j of layer 1 from its row of the image (W1 is kept out-major there: the row is contiguous): tanh(b1[j] + sum_i W1[i][j] p0[i]), inputs in order
    __device__ __forceinline__ float mlp_unit1(int ns, int j, const float (&p0)[TVM]) const {
        const float* row = w1 + tvm_w1(ns) + j * TVM;
        float a = w1[tvm_b1(ns) + j];
#pragma unroll
        for (int i = 0; i < TVM; ++i) a = fmaf(row[i], p0[i], a);
        return tanh_fast(a);
    }
    // V: the head from b2 by fmaf in unit order, then added to the candidate's bias.  One unit of layer 1 per trip, used at once: p1 is never a row of registers
    __device__ __forceinline__ float mlp_value(const float* s, int stride, int ns, int b, int per) const {
        float p0[TVM];
        mlp_layer0(s, stride, ns, p0);
        const float* W2 = w1 + tvm_w2(ns);
        float v = W2[TVM];                                    // b2
#pragma unroll 1
        for (int j = 0; j < TVM; ++j) v = fmaf(W2[j], mlp_unit1(ns, j, p0), v);
        return bias_of(b, per) + v;
    }
    // g0 = (W1 (W2 * (1 - p1^2))) * (1 - p0^2): the adjoint of layer 0's pre-activations, from which mlp_grad forms dV/ds_d
    __device__ __forceinline__ void mlp_adjoint(const float* s, int stride, int ns, float (&g0)[TVM]) const {
        float p0[TVM];
        mlp_layer0(s, stride, ns, p0);
        const float* W2 = w1 + tvm_w2(ns);
#pragma unroll
        for (int i = 0; i < TVM; ++i) g0[i] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < TVM; ++j) {
            const float p = mlp_unit1(ns, j, p0);
            const float g1 = W2[j] * fmaf(-p, p, 1.0f);
            const float* row = w1 + tvm_w1(ns) + j * TVM;
#pragma unroll
            for (int i = 0; i < TVM; ++i) g0[i] = fmaf(row[i], g1, g0[i]);
        }
#pragma unroll
        for (int i = 0; i < TVM; ++i) g0[i] *= fmaf(-p0[i], p0[i], 1.0f);
    }
    // dV/ds_d at s_d: the clip gate of grad()
    __device__ __forceinline__ float mlp_grad(int d, float sd, const float (&g0)[TVM]) const {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < TVM; ++i) a = fmaf(w1[d * TVM + i], g0[i], a);
        return (sd >= -10.0f && sd <= 10.0f) ? a : 0.0f;
    }
    // what the forward kernels evaluate behind their loop, by their template parameter
    template <int TV>
    __device__ __forceinline__ float value_of(const float* s, int stride, int ns, int b, int per) const {
        if constexpr (TV == TV_MLP) return mlp_value(s, stride, ns, b, per);
        else return value(s, stride, ns, b, per);
    }
};

// the context's terminal value as the kernels take it (d_tv: w1 | w2 | bias, or the MLP's image | bias); all NULL while none is set
static inline TermVal ctx_term_val(const metrpo_ctx* c) {
    if (c->tv_n_bias < 1) return TermVal{nullptr, nullptr, nullptr, 0};
    const float* p = c->d_tv.p;
    if (c->tv_kind == TV_MLP) return TermVal{p, nullptr, p + tvm_floats(c->pd.ns), c->tv_n_bias};
    return TermVal{p, p + c->pd.ns, p + 2 * c->pd.ns, c->tv_n_bias};
}
// the MLP form's seed lambda_T [K][n][ns] of a chunk of n candidates: behind WE [K][n] in the gradient calls' workspace (K is the grid's y extent in the kernels)
__host__ __device__ inline float* tv_mlp_seed_of(float* WE, int n, int K) { return WE + (size_t)K * n; }
// ... and its kind, the index of every table of kernels below: TV_NONE, TV_QUAD, TV_MLP
static inline int ctx_tv_kind(const metrpo_ctx* c) { return c->tv_n_bias < 1 ? TV_NONE : c->tv_kind; }

// one step of the return: ret += gamma^t alive_t r_t in float64, then the discount, then the mask (model_based_rl.py:134-137: the step that ends an
// episode still counts).  A step that is not counted adds nothing (no 0 * r).  step() hands out the step's weight for the gradient kernels: gamma^t carried
// in float64 by repeated multiplication and rounded to fp32 where it becomes a weight; a step that is not counted has weight 0.  The scorers drop it.
// terminal(v), behind the T-th step: ret += gamma^T alive_T v -- a candidate that met a done, at the last step included, gets no bootstrap; n stands.  It hands
// out w_T = alive_T ? (float)gamma^T : 0, the weight of the reverse recursion's seed lambda_T = w_T dV/ds_T.
struct SactSum {
    double sum = 0.0, disc = 1.0;
    int n = 0;
    bool alive = true;
    __device__ __forceinline__ float step(float rew, bool done, double gamma, int stop) {
        const float w = alive ? (float)disc : 0.0f;
        if (alive) { sum += disc * (double)rew; ++n; }
        disc *= gamma;
        if (stop && done) alive = false;
        return w;
    }
    __device__ __forceinline__ float terminal(float v) {
        if (alive) sum += disc * (double)v;
        return alive ? (float)disc : 0.0f;
    }
};

// -------------------------------------------------------------------------------------------------
// Generic gradient kernels: thread = (column of the chunk, head k = blockIdx.y), activations in LDS columns (device_common.h), LD = blockDim.x.
// PH: the policy's hidden layers, only with `pol` (score_policy_actions_grad.hip)
struct GradBufs { float *S, *XN, *LAM, *U, *UR, *X, *PH, *DH, *GA, *GB; };
__host__ __device__ inline int grad_mw(const ProblemDesc& pd, bool pol) { return max(pol ? max(pd.dyn.max_width, pd.pol.max_width) : pd.dyn.max_width, pd.ns + pd.na); }
__host__ __device__ inline size_t grad_gen_floats(const ProblemDesc& pd, bool pol) {
    return (size_t)(3 * pd.ns + 2 * pd.na + (pd.ns + pd.na) + (pol ? net_hidden_rows(pd.pol) : 0) + net_hidden_rows(pd.dyn) + 2 * grad_mw(pd, pol));
}
__device__ __forceinline__ GradBufs grad_carve(float* lds, const ProblemDesc& pd, int LD, bool pol) {
    GradBufs e;
    e.S = lds; e.XN = e.S + pd.ns * LD; e.LAM = e.XN + pd.ns * LD; e.U = e.LAM + pd.ns * LD; e.UR = e.U + pd.na * LD; e.X = e.UR + pd.na * LD;
    e.PH = e.X + (pd.ns + pd.na) * LD; e.DH = e.PH + (pol ? net_hidden_rows(pd.pol) : 0) * LD; e.GA = e.DH + net_hidden_rows(pd.dyn) * LD; e.GB = e.GA + grad_mw(pd, pol) * LD;
    return e;
}
