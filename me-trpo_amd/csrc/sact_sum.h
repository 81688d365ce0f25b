// The per-candidate return of metrpo_score_actions and metrpo_score_policy_actions (include/metrpo.h): what score_actions.hip's and
// score_policy_actions.hip's fused kernels carry per lane and what k_sact_reduce applies to a stored trajectory.
// Below it: what the generic kernels of the two gradient files (score_actions_grad.hip, score_policy_actions_grad.hip) share -- their LDS columns, a net's
// hidden layers and its vector-Jacobian product, and the cost adjoint.
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
__host__ __device__ inline int net_hidden_rows(const NetDesc& n) {
    int rows = 0;
    for (int l = 1; l < n.n_layers; ++l) rows += n.dims[l];
    return rows;
}
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
// the hidden layers of a net into `store` (all outputs kept; the output layer is not formed)
__device__ __forceinline__ void net_hidden(const NetDesc& n, const float* __restrict__ params, const float* in, float* store, int LD, int tid) {
    const float* cur = in; float* dst = store;
    for (int l = 0; l < n.n_layers - 1; ++l) {
        dense_col(params + n.w_off[l], params + n.b_off[l], n.dims[l], n.dims[l + 1], n.act[l], cur, dst, LD, tid);
        cur = dst; dst += n.dims[l + 1] * LD;
    }
}
// dout = W . (din * act'(h)) chains of one net, back from `da` (the adjoint of the net's output, n_out rows) to the adjoint of its input; `store` holds the
// hidden layers' outputs in layer order (k_bptt_backward's loops, bptt.hip).  Returns the buffer (da or db) that holds the result.
__device__ __forceinline__ float* net_vjp(const NetDesc& n, const float* __restrict__ params, const float* store, float* da, float* db, int LD, int tid) {
    int off = 0;
    for (int l = 1; l < n.n_layers - 1; ++l) off += n.dims[l];                // rows of the LAST hidden layer in the store
    for (int l = n.n_layers - 1; l >= 0; --l) {
        dense_col_T(params + n.w_off[l], n.dims[l], n.dims[l + 1], da, db, LD, tid);
        if (l > 0) {
            const float* h = store + off * LD;                                 // output of layer l-1 (post-activation)
            for (int j = 0; j < n.dims[l]; ++j) {
                const float hv = h[j * LD + tid];
                const float dact = (n.act[l - 1] == METRPO_ACT_RELU) ? (hv > 0.0f ? 1.0f : 0.0f)
                                  : (n.act[l - 1] == METRPO_ACT_TANH) ? (1.0f - hv * hv) : 1.0f;
                db[j * LD + tid] *= dact;
            }
            if (l > 1) off -= n.dims[l - 1];
        }
        float* tmp = da; da = db; db = tmp;
    }
    return da;
}
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
