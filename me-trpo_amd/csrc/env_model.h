// The environments' reward model: cost (reward = -cost), its adjoint and the termination rule, stated once for every kernel family.
//   envs/com_*_env.py cost_np_vec / cost_tf / is_done -- see include/metrpo.h metrpo_env for file:line
// An environment's constants appear here and nowhere else in csrc/.  Every function is inlined arithmetic on values the caller already holds, so `env` folds
// wherever it is a template or compile-time constant; the generic kernels pass the runtime value.
//
// Device code is compiled with floating-point contraction on.  The cost value leaves it to the compiler, as every kernel always has: which of its products
// fuse differs between the kernel families (a product shared by several heads, or packed with a neighbour, stays a product), and each family keeps its own.
// The adjoint spells its fused multiply-adds out, so it does not depend on the caller.  Its x_next half comes in two forms that round differently, both as the
// kernels have always computed them.  The row form (env_cost_dx_row: the column- and row-layout kernels, which own a whole adjoint row) adds every term into
// the adjoint on its own, the product fused into the sum where there is one: G = fma(w, c, G), and at Hopper's dim 5 with |v| > 100 G -= w; G += +-w.  The
// per-dimension form (env_cost_dx: the D-layout block, svg, the probe) rounds the dimension's sum of terms first and the caller adds it: G += (-w +- w),
// G += round(w c).
#pragma once
#include "metrpo.h"

// state / action vector of one sample behind a pointer and a stride: p[i * ld]
struct EnvVec {
    const float* p; int ld;
    __device__ __forceinline__ float operator()(int i) const { return p[i * ld]; }
};
// column tid of a [dim][LD] tile (LD = 1, tid = 0: a row)
__device__ __forceinline__ EnvVec env_col(const float* p, int LD, int tid) { return EnvVec{p + tid, LD}; }

// the one state dimension every cost reads (Hopper reads the others against their bounds as well)
__host__ __device__ constexpr int env_key_dim(int env, int ns) {
    return (env == METRPO_ENV_SWIMMER || env == METRPO_ENV_HOPPER) ? 5 : (env == METRPO_ENV_HALF_CHEETAH) ? 9 : (env == METRPO_ENV_ANT) ? 15
         : (env == METRPO_ENV_SNAKE) ? 7 : (env == METRPO_ENV_HUMANOID) ? ns - 1 : 0;
}

// ---- cost value ----------------------------------------------------------------------------------------------------------------------------------------
// sum of squared (clipped) actions, in action order
template <class U> __device__ __forceinline__ float env_su2(int na, U u) {
    float su2 = 0.0f;
    for (int d = 0; d < na; ++d) { const float a = u(d); su2 = fmaf(a, a, su2); }
    return su2;
}
// Hopper: one of dims 2 .. ns-1 against its bound, and their sum in the reference's order (the MFMA rollouts reduce the terms across lanes instead)
__device__ __forceinline__ float env_hopper_pen_term(float v) { return fmaxf(fabsf(v) - 100.0f, 0.0f); }
template <class X> __device__ __forceinline__ float env_hopper_pen(int ns, X x) {
    float pen = 0.0f;
    for (int i = 2; i < ns; ++i) pen += env_hopper_pen_term(x(i));
    return pen;
}
// half-cheetah: the clipped quantity
__device__ __forceinline__ float env_cheetah_inner(float key, float su2) { return key - 1e-1f * 0.5f * su2; }
// the cost from its terms: key = x_next[env_key_dim], x0 / x1 / pen are Hopper's (x_next[0], x_next[1], env_hopper_pen), unread elsewhere
__device__ __forceinline__ float env_cost_terms(int env, int na, float key, float x0, float x1, float su2, float pen) {
    switch (env) {
    case METRPO_ENV_SWIMMER: return -(key - 1e-2f * (su2 / (float)na));
    case METRPO_ENV_HALF_CHEETAH: return -fminf(fmaxf(env_cheetah_inner(key, su2), -10.0f), 10.0f);
    case METRPO_ENV_ANT: return -(key - 1e-2f * 0.5f * su2 + 0.05f);
    case METRPO_ENV_HUMANOID: { const float h = key - 1.5f; return h * h + 1e-2f * 1e-3f * su2; }
    case METRPO_ENV_HOPPER: return -(key - 0.01f * 0.5f * su2 - 10.0f * fmaxf(0.45f - x0, 0.0f) - 10.0f * fmaxf(fabsf(x1) - 0.2f, 0.0f) - pen);
    case METRPO_ENV_SNAKE: return -(key - 1e-2f * 0.5f * su2);
    }
    return 0.0f;
}
// the cost of (x_next, u) behind accessors x(i), u(d), with su2 formed here or by the caller
template <class X> __device__ __forceinline__ float env_cost_su2(int env, int ns, int na, X x, float su2) {
    if (env == METRPO_ENV_HOPPER) return env_cost_terms(METRPO_ENV_HOPPER, na, x(env_key_dim(METRPO_ENV_HOPPER, ns)), x(0), x(1), su2, env_hopper_pen(ns, x));
    return env_cost_terms(env, na, x(env_key_dim(env, ns)), 0.0f, 0.0f, su2, 0.0f);
}
template <class X, class U> __device__ __forceinline__ float env_cost(int env, int ns, int na, X x, U u) { return env_cost_su2(env, ns, na, x, env_su2(na, u)); }

// ---- termination ---------------------------------------------------------------------------------------------------------------------------------------
// Ant falls out of 0.2 <= z <= 1.0 or leaves the finite numbers; the other environments end at the horizon only.  z = x_next[2]; every site forms
// all_finite over the state's dims its own way.
__device__ __forceinline__ bool env_done(int env, float z, bool all_finite) { return env == METRPO_ENV_ANT && !((z >= 0.2f) && (z <= 1.0f) && all_finite); }
template <class X> __device__ __forceinline__ bool env_done_scan(int env, int ns, X x) {
    if (env != METRPO_ENV_ANT) return false;
    bool finite = true;
    for (int i = 0; i < ns; ++i) finite = finite && isfinite(x(i));
    return env_done(env, x(2), finite);
}

// ---- cost adjoint: the terms of d(w cost), w the step's weight (the scorers' gradient kernels pass -w_t for the gradient of the return) ---------------------
// half-cheetah: tf.clip_by_value passes the gradient inside [min, max], bounds included; the other environments have no gate
__device__ __forceinline__ bool env_clip_inside(int env, float key, float su2) {
    if (env != METRPO_ENV_HALF_CHEETAH) return true;
    const float inner = env_cheetah_inner(key, su2);
    return inner >= -10.0f && inner <= 10.0f;
}
template <class X> __device__ __forceinline__ bool env_clip_inside_at(int env, int ns, X x, float su2) {      // reads x_next only where there is a gate
    return env != METRPO_ENV_HALF_CHEETAH || env_clip_inside(env, x(env_key_dim(env, ns)), su2);
}
// d(w cost)/du[d] = env_cost_du(..) * u[d]
__device__ __forceinline__ float env_cost_du(int env, int na, bool inside, float w) {
    switch (env) {
    case METRPO_ENV_SWIMMER: return w * 1e-2f * 2.0f / (float)na;
    case METRPO_ENV_HALF_CHEETAH: return inside ? w * 1e-1f : 0.0f;
    case METRPO_ENV_HUMANOID: return w * 2e-5f;
    case METRPO_ENV_HOPPER: return w * 0.01f;
    }
    return w * 1e-2f;                                                   // ant, snake
}
// d cost/dx_next[env_key_dim]'s own term at weight 1; v = x_next[key dim] (read by the humanoid alone).  A value of env outside metrpo_env would take the
// default here and in env_key_dim (the parent's switches did nothing): every context validates env when it is created.
__device__ __forceinline__ float env_cost_dx_key(int env, float v, bool inside) {
    switch (env) {
    case METRPO_ENV_HALF_CHEETAH: return inside ? -1.0f : 0.0f;
    case METRPO_ENV_HUMANOID: return 2.0f * (v - 1.5f);
    }
    return -1.0f;
}
// Hopper: dim's bound term of d(w cost), added into g where v = x_next[dim] is beyond the bound
__device__ __forceinline__ void env_hopper_bound_dx(int dim, float v, float w, float& g) {
#pragma clang fp contract(off)
    if (dim == 0) { if (0.45f - v > 0.0f) g = fmaf(-10.0f, w, g); }
    else if (dim == 1) { if (fabsf(v) - 0.2f > 0.0f) g += w * 10.0f * (v > 0.0f ? 1.0f : -1.0f); }
    else if (fabsf(v) - 100.0f > 0.0f) g += w * (v > 0.0f ? 1.0f : -1.0f);
}
// per-dimension form: d(w cost)/dx_next[dim], the dimension's terms summed
__device__ __forceinline__ float env_cost_dx(int env, int ns, int dim, float v, bool inside, float w) {
#pragma clang fp contract(off)
    if (env != METRPO_ENV_HOPPER) return (dim == env_key_dim(env, ns)) ? w * env_cost_dx_key(env, v, inside) : 0.0f;
    float g = 0.0f;
    if (dim == 5) g -= w;
    env_hopper_bound_dx(dim, v, w, g);
    return g;
}
// row form: every term added into the caller's adjoint row g(i) (a float&) on its own; touches the key dimension only, every dimension for Hopper
template <class X, class G> __device__ __forceinline__ void env_cost_dx_row(int env, int ns, X x, bool inside, float w, G g) {
    const int k = env_key_dim(env, ns);
    g(k) = fmaf(w, env_cost_dx_key(env, (env == METRPO_ENV_HUMANOID) ? x(k) : 0.0f, inside), g(k));
    if (env == METRPO_ENV_HOPPER) {
        env_hopper_bound_dx(0, x(0), w, g(0));
        env_hopper_bound_dx(1, x(1), w, g(1));
        for (int i = 2; i < ns; ++i) env_hopper_bound_dx(i, x(i), w, g(i));
    }
}
// The generic reverse sweeps' cost adjoint on column tid of [dim][LD] tiles: d(w cost)/du -> gU (written), d(w cost)/dx_next -> added into G.
__device__ __forceinline__ void env_cost_adjoint(int env, int ns, int na, const float* xn, const float* u, float w, float* gU, float* G, int LD, int tid) {
    const EnvVec x = env_col(xn, LD, tid), uc = env_col(u, LD, tid);
    const float su2 = env_su2(na, uc);
    const bool inside = env_clip_inside_at(env, ns, x, su2);
    env_cost_dx_row(env, ns, x, inside, w, [&](int i) -> float& { return G[i * LD + tid]; });
    const float cu = env_cost_du(env, na, inside, w);
    for (int d = 0; d < na; ++d) gU[d * LD + tid] = cu * uc(d);
}

// The reverse sweeps' cost adjoint in the MFMA D layout (lane (c, q) owns state dims 16 cb + 4 q + r of env c and action dims 4 q + r):
// G = lam + d(w cost)/dx_next, gU = d(w cost)/du.  nx / act: env c's rows of the step's next state and clipped action.
template <int ENV, int NS, int NA, int OUT_CB, class V4>
__device__ __forceinline__ void env_cost_adjoint_d(V4 (&G)[OUT_CB], V4& gU, const V4 (&lam)[OUT_CB], float w, const float* nx, const float* act, int q) {
    constexpr int KD = env_key_dim(ENV, NS);
    const bool inside = env_clip_inside_at(ENV, NS, EnvVec{nx, 1}, env_su2(NA, EnvVec{act, 1}));
#pragma unroll
    for (int cb = 0; cb < OUT_CB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dim = 16 * cb + 4 * q + r;
            G[cb][r] = lam[cb][r];
            if ((ENV == METRPO_ENV_HOPPER) ? dim < NS : dim == KD) G[cb][r] += env_cost_dx(ENV, NS, dim, nx[dim], inside, w);
        }
    const float cu = env_cost_du(ENV, NA, inside, w);
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int d = 4 * q + r; gU[r] = (d < NA) ? cu * act[d] : 0.0f; }
}
