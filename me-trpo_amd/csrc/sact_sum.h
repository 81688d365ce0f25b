// The per-candidate return of metrpo_score_actions and metrpo_score_policy_actions (include/metrpo.h): what score_actions.hip's and
// score_policy_actions.hip's fused kernels carry per lane and what k_sact_reduce applies to a stored trajectory.
// Below it: what the generic kernels of the two gradient files (score_actions_grad.hip, score_policy_actions_grad.hip) share: their LDS columns (a net's hidden layers, its
// vector-Jacobian product and the cost adjoint are device_common.h's).
#pragma once
#include "device_common.h"

// The terminal value of metrpo_set_terminal_value (include/metrpo.h): LinearFeatureBaseline's form with its time features evaluated at a fixed step,
//   o_d = clip(s_d, -10, 10);  V(s) = bias + sum_d (w1[d] o_d + w2[d] o_d^2)
// w1 == nullptr: no terminal value is set.  The kernels read it once per lane BEHIND the step loop, never inside it.  Who tests the pointer (runtime-uniform):
// both reverse sweeps (k_sagr<.., SAGR_BWD>, k_spag_bwd, k_sagr_gen_bwd, k_spag_gen_bwd), k_spag_fwd and k_sact_reduce.  Who takes `set` as a template parameter
// TV instead: k_score_actions, k_score_policy_actions, k_sagr<.., SAGR_FWD, TV>, k_sagr_gen_fwd, k_spag_gen_fwd (why each: profiles/r26_terminal_value.txt).
// Candidate b uses bias[n_bias > 1 ? b / per : 0] (per = B / S).
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
};

// the context's terminal value as the kernels take it (d_tv: w1 | w2 | bias); all NULL while none is set
static inline TermVal ctx_term_val(const metrpo_ctx* c) {
    if (c->tv_n_bias < 1) return TermVal{nullptr, nullptr, nullptr, 0};
    const float* p = c->d_tv.p;
    return TermVal{p, p + c->pd.ns, p + 2 * c->pd.ns, c->tv_n_bias};
}

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
