// The per-candidate return of metrpo_score_actions and metrpo_score_policy_actions (include/metrpo.h): what score_actions.hip's and
// score_policy_actions.hip's fused kernels carry per lane and what k_sact_reduce applies to a stored trajectory.
// Below it: what the two gradient files (score_actions_grad.hip, score_policy_actions_grad.hip) share -- the same sum handing out the step's weight, and the
// generic kernels' cost adjoint.
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
// episode still counts).  A step that is not counted adds nothing (no 0 * r).
// terminal(v), behind the T-th step: ret += gamma^T alive_T v -- a candidate that met a done, at the last step included, gets no bootstrap; n stands.
struct SactSum {
    double sum = 0.0, disc = 1.0;
    int n = 0;
    bool alive = true;
    __device__ __forceinline__ void step(float rew, bool done, double gamma, int stop) {
        if (alive) { sum += disc * (double)rew; ++n; }
        disc *= gamma;
        if (stop && done) alive = false;
    }
    __device__ __forceinline__ void terminal(float v) { if (alive) sum += disc * (double)v; }
};

// metrpo_score_actions' step of the return (score_actions.hip: SactSum) with the step's weight handed out: gamma^t carried in float64 by repeated
// multiplication and rounded to fp32 where it becomes a weight; a step that is not counted has weight 0 and adds nothing
struct SagrSum {
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
    // behind the T-th step: SactSum::terminal, handing out w_T = alive_T ? (float)gamma^T : 0, the weight of the reverse recursion's seed lambda_T = w_T dV/ds_T
    __device__ __forceinline__ float terminal(float v) {
        if (alive) sum += disc * (double)v;
        return alive ? (float)disc : 0.0f;
    }
};

// d(w cost)/du -> gU (written), d(w cost)/dx_next -> added into G: bptt.hip's cost_adjoint (:54-78), called with w = -w_t for the gradient of the return
__device__ __forceinline__ void sagr_cost_adjoint(int env, int ns, int na, const float* xn, const float* u, float w, float* gU, float* G, int LD, int tid) {
    float su2 = 0.0f;
    for (int d = 0; d < na; ++d) { const float a = u[d * LD + tid]; su2 = fmaf(a, a, su2); }
    float cu = 0.0f;                                         // gU[d] = cu * u[d]
    switch (env) {
    case METRPO_ENV_SWIMMER: G[5 * LD + tid] -= w; cu = w * 1e-2f * 2.0f / (float)na; break;
    case METRPO_ENV_HALF_CHEETAH: {
        const float inner = xn[9 * LD + tid] - 1e-1f * 0.5f * su2;
        const float p = (inner >= -10.0f && inner <= 10.0f) ? 1.0f : 0.0f;
        G[9 * LD + tid] -= w * p; cu = w * p * 1e-1f; break;
    }
    case METRPO_ENV_ANT: G[15 * LD + tid] -= w; cu = w * 1e-2f; break;
    case METRPO_ENV_HUMANOID: G[(ns - 1) * LD + tid] += w * 2.0f * (xn[(ns - 1) * LD + tid] - 1.5f); cu = w * 2e-5f; break;
    case METRPO_ENV_HOPPER: {
        G[5 * LD + tid] -= w; cu = w * 0.01f;
        if (0.45f - xn[0 * LD + tid] > 0.0f) G[0 * LD + tid] -= w * 10.0f;
        const float a1 = xn[1 * LD + tid];
        if (fabsf(a1) - 0.2f > 0.0f) G[1 * LD + tid] += w * 10.0f * (a1 > 0.0f ? 1.0f : -1.0f);
        for (int i = 2; i < ns; ++i) { const float v = xn[i * LD + tid]; if (fabsf(v) - 100.0f > 0.0f) G[i * LD + tid] += w * (v > 0.0f ? 1.0f : -1.0f); }
        break;
    }
    case METRPO_ENV_SNAKE: G[7 * LD + tid] -= w; cu = w * 1e-2f; break;
    }
    for (int d = 0; d < na; ++d) gU[d * LD + tid] = cu * u[d * LD + tid];
}
