// 'l-bfgs' policy update (model_based_rl.py:391-398, :1197-1202): L-BFGS-B 3.0 on an unbounded problem (nbd = 0 everywhere) as scipy's
// minimize(method='L-BFGS-B') drives it, by reverse communication: k_lbfgs_step consumes f and g at the point it asked for last and
// leaves the next point to evaluate plus scipy's task code.  tests/lbfgs_ref.py restates the same state machine in NumPy, step for step:
//
//   direction   no stored pair: the Cauchy point at theta = 1, z = x + (-g); else z = x + (-H g) (two-loop recursion over the last m pairs,
//               H0 = I / theta, theta = y.y / s.y of the newest pair); d = z - x, as mainlb forms it
//   search      lnsrlb + MINPACK-2 dcsrch / dcstep (ftol 1e-3, gtol 0.9, xtol 0.1, stpmin 0, stpmax 1e10); first step min(1/|d|, 1e10) at
//               iteration 0, 1 afterwards; the trial is z when stp == 1, else stp * d + t; a WARNING outcome is accepted
//   failure     g.d >= 0 at the start or the (maxls + 1)-th trial: x, g, f back to the start; ABNORMAL with no pair, else drop the pairs
//   NEW_X       nit += 1, then scipy's wrapper limits (nit >= maxiter, nfev > maxfun), then setulb's tests (max|g| <= gtol, the relative
//               reduction of f), then the pair (skipped when s.y <= eps * (-g_old.d * stp))
//
// One workgroup of 1024 threads per call.  The scalar logic runs on thread 0 against a copy of the state in LDS; every vector operation and
// reduction uses the whole block in a fixed order (strided per-thread partial sums, then the wave and block sums of device_common.h), so a
// run is bitwise reproducible.  Floating-point contraction is off in this file: the products and sums round as the NumPy restatement's do.
#include "metrpo_internal.h"
#include "device_common.h"
#include "cg_device.h"
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace {

constexpr int LB_THREADS = 1024;
constexpr double LB_EPS = 2.220446049250313e-16;
constexpr double LS_FTOL = 1e-3, LS_GTOL = 0.9, LS_XTOL = 0.1, STPMAX = 1e10;
enum { PH_START = 0, PH_SEARCH = 1, PH_DONE = 2 };
enum { LS_FG = 0, LS_CONV = 1, LS_WARN = 2 };
constexpr int LB_SLOTS = 17;          // pinned publish slots: lookahead <= 16 in flight
constexpr int LB_SLOT_DOUBLES = 17;   // ls_publish layout: 14 values, the stamp at [16]

// the scalar state of one minimisation (thread 0 owns it; the block reads it from the LDS copy)
struct LbScal {
    double f, fold, gd, gdold, stp, theta, tol, gtol, f_last;
    double finit, ginit, gtest, width, width1, stx, fx, gx, sty, fy, gy, stmin, stmax;   // dcsrch
    int brackt, stage;
    int phase, col, head, ifun, iback, nit, nfev, same, task, task_code;
    int n, m, maxls, maxiter, maxfun;
    int bcast_i;      // a branch decision of thread 0 for the whole block
    double bcast_d;   // a reduction result of thread 0 for the whole block
    double pub[14];   // what a step publishes: task, task_code, nit, nfev, f_last
};

// device memory of the state: LbScal | sy[m] | alpha[m] | x | g | d | z | t | r | xe | S[m][n] | Y[m][n]
struct LbView {
    LbScal* sc; double *sy, *al, *x, *g, *d, *z, *t, *r, *xe, *S, *Y;
};
inline size_t lb_scal_doubles() { return (sizeof(LbScal) + sizeof(double) - 1) / sizeof(double); }
inline size_t lb_doubles(int n, int m) { return lb_scal_doubles() + 2 * (size_t)m + 7 * (size_t)n + 2 * (size_t)m * n; }
LbView lb_view(double* base, int n, int m) {
    LbView v; v.sc = (LbScal*)base;
    double* p = base + lb_scal_doubles();
    v.sy = p; p += m; v.al = p; p += m;
    v.x = p; p += n; v.g = p; p += n; v.d = p; p += n; v.z = p; p += n; v.t = p; p += n; v.r = p; p += n; v.xe = p; p += n;
    v.S = p; p += (size_t)m * n; v.Y = p;
    return v;
}

// ---- block-wide reductions, result broadcast to every thread through the LDS state
__device__ double blk_dot(const double* a, const double* b, int n, LbScal& s, double* sh) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += LB_THREADS) acc += a[i] * b[i];
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) s.bcast_d = r;
    __syncthreads();
    const double out = s.bcast_d;
    __syncthreads();
    return out;
}
__device__ double blk_absmax(const double* a, int n, LbScal& s, double* sh) {
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += LB_THREADS) m = fmax(m, fabs(a[i]));
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, WAVE));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int i = 0; i < LB_THREADS / 64; ++i) r = fmax(r, sh[i]);
        s.bcast_d = r;
    }
    __syncthreads();
    const double out = s.bcast_d;
    __syncthreads();
    return out;
}
// every element equal (the evaluation cache of scipy's ScalarFunction)
__device__ int blk_equal(const double* a, const double* b, int n, LbScal& s) {
    if (threadIdx.x == 0) s.bcast_i = 1;
    __syncthreads();
    int ne = 0;
    for (int i = threadIdx.x; i < n; i += LB_THREADS) ne |= (a[i] != b[i]);
    if (ne) s.bcast_i = 0;      // (a benign race: every writer stores 0)
    __syncthreads();
    const int out = s.bcast_i;
    __syncthreads();
    return out;
}

// ---- MINPACK-2 dcstep / dcsrch (thread 0)
__device__ void dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double& stp, double fp, double dp,
                       int& brackt, double stpmin, double stpmax) {
    const double sgnd = dp * (dx / fabs(dx));
    double stpf;
    if (fp > fx) {
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp < stx) gamma = -gamma;
        const double p = (gamma - dx) + theta, q = ((gamma - dx) + gamma) + dp, r = p / q;
        const double stpc = stx + r * (stp - stx);
        const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
        stpf = (fabs(stpc - stx) < fabs(stpq - stx)) ? stpc : stpc + (stpq - stpc) / 2.0;
        brackt = 1;
    } else if (sgnd < 0.0) {
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dx, r = p / q;
        const double stpc = stp + r * (stx - stp);
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        stpf = (fabs(stpc - stp) > fabs(stpq - stp)) ? stpc : stpq;
        brackt = 1;
    } else if (fabs(dp) < fabs(dx)) {
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt(fmax(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta, q = (gamma + (dx - dp)) + gamma, r = p / q;
        double stpc;
        if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
        else if (stp > stx) stpc = stpmax;
        else stpc = stpmin;
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (brackt) {
            stpf = (fabs(stpc - stp) < fabs(stpq - stp)) ? stpc : stpq;
            if (stp > stx) stpf = fmin(stp + 0.66 * (sty - stp), stpf);
            else stpf = fmax(stp + 0.66 * (sty - stp), stpf);
        } else {
            stpf = (fabs(stpc - stp) > fabs(stpq - stp)) ? stpc : stpq;
            stpf = fmin(stpmax, stpf);
            stpf = fmax(stpmin, stpf);
        }
    } else {
        if (brackt) {
            const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
            const double s = fmax(fmax(fabs(theta), fabs(dy)), fabs(dp));
            double gamma = s * sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
            if (stp > sty) gamma = -gamma;
            const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dy, r = p / q;
            stpf = stp + r * (sty - stp);
        } else if (stp > stx) stpf = stpmax;
        else stpf = stpmin;
    }
    if (fp > fx) { sty = stp; fy = fp; dy = dp; }
    else {
        if (sgnd < 0.0) { sty = stx; fy = fx; dy = dx; }
        stx = stp; fx = fp; dx = dp;
    }
    stp = stpf;
}
__device__ void dcsrch_start(LbScal& s, double f, double g, double stp) {
    s.stp = stp; s.brackt = 0; s.stage = 1;
    s.finit = f; s.ginit = g; s.gtest = LS_FTOL * g;
    s.width = STPMAX - 0.0; s.width1 = s.width / 0.5;
    s.stx = 0.0; s.fx = f; s.gx = g;
    s.sty = 0.0; s.fy = f; s.gy = g;
    s.stmin = 0.0; s.stmax = stp + 4.0 * stp;
}
__device__ int dcsrch_step(LbScal& s, double f, double g) {
    double stp = s.stp;
    const double gtest = s.gtest, ftest = s.finit + stp * gtest;
    if (s.stage == 1 && f <= ftest && g >= 0.0) s.stage = 2;
    int task = LS_FG;
    if (s.brackt && (stp <= s.stmin || stp >= s.stmax)) task = LS_WARN;
    if (s.brackt && s.stmax - s.stmin <= LS_XTOL * s.stmax) task = LS_WARN;
    if (stp == STPMAX && f <= ftest && g <= gtest) task = LS_WARN;
    if (stp == 0.0 && (f > ftest || g >= gtest)) task = LS_WARN;
    if (f <= ftest && fabs(g) <= LS_GTOL * (-s.ginit)) task = LS_CONV;
    if (task != LS_FG) return task;
    if (s.stage == 1 && f <= s.fx && f > ftest) {
        const double fm = f - stp * gtest;
        double fxm = s.fx - s.stx * gtest, fym = s.fy - s.sty * gtest;
        const double gm = g - gtest;
        double gxm = s.gx - gtest, gym = s.gy - gtest;
        dcstep(s.stx, fxm, gxm, s.sty, fym, gym, stp, fm, gm, s.brackt, s.stmin, s.stmax);
        s.fx = fxm + s.stx * gtest; s.fy = fym + s.sty * gtest;
        s.gx = gxm + gtest; s.gy = gym + gtest;
    } else {
        dcstep(s.stx, s.fx, s.gx, s.sty, s.fy, s.gy, stp, f, g, s.brackt, s.stmin, s.stmax);
    }
    if (s.brackt) {
        if (fabs(s.sty - s.stx) >= 0.66 * s.width1) stp = s.stx + 0.5 * (s.sty - s.stx);
        s.width1 = s.width;
        s.width = fabs(s.sty - s.stx);
        s.stmin = fmin(s.stx, s.sty); s.stmax = fmax(s.stx, s.sty);
    } else {
        s.stmin = stp + 1.1 * (stp - s.stx);
        s.stmax = stp + 4.0 * (stp - s.stx);
    }
    stp = fmin(fmax(stp, 0.0), STPMAX);
    if ((s.brackt && (stp <= s.stmin || stp >= s.stmax)) || (s.brackt && s.stmax - s.stmin <= LS_XTOL * s.stmax)) stp = s.stx;
    s.stp = stp;
    return LS_FG;
}

// x, g, f back to the start of the search (thread 0 has set nothing yet; all threads)
__device__ void lb_restore(const LbView& v, LbScal& s, int n) {
    for (int i = threadIdx.x; i < n; i += LB_THREADS) { v.x[i] = v.t[i]; v.g[i] = v.r[i]; }
    if (threadIdx.x == 0) s.f = s.fold;
    __syncthreads();
}

// direction + lnsrlb's first entry; returns 1 with the first trial step in s.stp, 0 on a line-search failure (g.d >= 0)
__device__ int lb_search_start(const LbView& v, LbScal& s, int n, double* sh) {
    const int m = s.m;
    if (s.col == 0) {
        for (int i = threadIdx.x; i < n; i += LB_THREADS) { const double z = v.x[i] + (-v.g[i]); v.z[i] = z; v.d[i] = z - v.x[i]; }
        __syncthreads();
    } else {
        // two-loop recursion on q (kept in d), newest pair first
        for (int i = threadIdx.x; i < n; i += LB_THREADS) v.d[i] = -v.g[i];
        __syncthreads();
        for (int j = s.col - 1; j >= 0; --j) {
            const int k = (s.head + j) % m;
            const double a = blk_dot(v.S + (size_t)k * n, v.d, n, s, sh) / v.sy[k];
            if (threadIdx.x == 0) v.al[k] = a;
            for (int i = threadIdx.x; i < n; i += LB_THREADS) v.d[i] = v.d[i] - a * v.Y[(size_t)k * n + i];
            __syncthreads();
        }
        const double theta = s.theta;
        for (int i = threadIdx.x; i < n; i += LB_THREADS) v.d[i] = v.d[i] / theta;
        __syncthreads();
        for (int j = 0; j < s.col; ++j) {
            const int k = (s.head + j) % m;
            const double b = blk_dot(v.Y + (size_t)k * n, v.d, n, s, sh) / v.sy[k];
            const double a = v.al[k];
            for (int i = threadIdx.x; i < n; i += LB_THREADS) v.d[i] = v.d[i] + v.S[(size_t)k * n + i] * (a - b);
            __syncthreads();
        }
        for (int i = threadIdx.x; i < n; i += LB_THREADS) { const double z = v.x[i] + v.d[i]; v.z[i] = z; v.d[i] = z - v.x[i]; }
        __syncthreads();
    }
    const double dtd = blk_dot(v.d, v.d, n, s, sh);
    const double gd = blk_dot(v.g, v.d, n, s, sh);
    for (int i = threadIdx.x; i < n; i += LB_THREADS) { v.t[i] = v.x[i]; v.r[i] = v.g[i]; }
    if (threadIdx.x == 0) {
        const double dnorm = sqrt(dtd);
        const double stp = (s.nit == 0) ? fmin(1.0 / dnorm, STPMAX) : 1.0;
        s.fold = s.f; s.ifun = 0; s.iback = 0;
        s.gd = gd; s.gdold = gd;
        s.bcast_i = (gd >= 0.0) ? 0 : 1;
        if (s.bcast_i) {
            dcsrch_start(s, s.f, gd, stp);
            s.ifun = 1; s.iback = 0;      // (maxls >= 1: the first trial is always allowed)
        }
    }
    __syncthreads();
    const int ok = s.bcast_i;
    __syncthreads();
    return ok;
}

// the trial point of the current s.stp into x, the evaluation cache flag, x_eval and the float32 policy image
__device__ void lb_emit(const LbView& v, LbScal& s, int n, double* x_eval, float* theta32) {
    const double stp = s.stp;
    for (int i = threadIdx.x; i < n; i += LB_THREADS) v.x[i] = (stp == 1.0) ? v.z[i] : stp * v.d[i] + v.t[i];
    __syncthreads();
    const int same = blk_equal(v.x, v.xe, n, s);
    for (int i = threadIdx.x; i < n; i += LB_THREADS) {
        const double xi = v.x[i];
        v.xe[i] = xi;
        if (x_eval) x_eval[i] = xi;
        if (theta32) theta32[i] = (float)xi;
    }
    if (threadIdx.x == 0) { s.same = same; s.task = 3; s.task_code = 0; }
    __syncthreads();
}
__device__ void lb_finish(const LbView& v, LbScal& s, int n, int task, int code, double* x_eval, float* theta32) {
    for (int i = threadIdx.x; i < n; i += LB_THREADS) {
        const double xi = v.x[i];
        if (x_eval) x_eval[i] = xi;
        if (theta32) theta32[i] = (float)xi;
    }
    if (threadIdx.x == 0) { s.phase = PH_DONE; s.task = task; s.task_code = code; }
    __syncthreads();
}

// a search from the current iterate, restarting once from the Cauchy direction after a failure with stored pairs
__device__ void lb_search(const LbView& v, LbScal& s, int n, double* sh, double* x_eval, float* theta32) {
    for (;;) {
        if (lb_search_start(v, s, n, sh)) { lb_emit(v, s, n, x_eval, theta32); return; }
        lb_restore(v, s, n);
        const int col = s.col;
        __syncthreads();                // (every thread has read col before thread 0 clears it)
        if (col == 0) { lb_finish(v, s, n, 8, 0, x_eval, theta32); return; }
        if (threadIdx.x == 0) { s.col = 0; s.head = 0; s.theta = 1.0; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(LB_THREADS) k_lbfgs_begin(LbView v, int n, const double* __restrict__ x0, const float* __restrict__ x0f,
                                                            LbScal init, double* x_eval) {
    for (int i = threadIdx.x; i < n; i += LB_THREADS) {
        const double xi = x0 ? x0[i] : (double)x0f[i];
        v.x[i] = xi; v.xe[i] = xi;
        if (x_eval) x_eval[i] = xi;
    }
    if (threadIdx.x == 0) *v.sc = init;
}

// One reverse-communication step.  f: *fin, or (policy mode, fin == NULL) the mean of costs[0..K) in model order; round_f32: f and g
// rounded to float32 first.  pub: this step's pinned publish slot (NULL: none).
__global__ void __launch_bounds__(LB_THREADS) k_lbfgs_step(LbView v, const double* __restrict__ fin, const double* __restrict__ costs, int K,
                                                           const double* __restrict__ gin, int round_f32, double* x_eval, float* theta32,
                                                           int32_t* task_out, double* pub, unsigned long long stamp) {
    __shared__ LbScal s;
    __shared__ double sh[16];
    if (threadIdx.x == 0) s = *v.sc;
    __syncthreads();
    const int n = s.n, phase = s.phase;      // (read by every thread before thread 0 changes either: the next barrier is below)
    if (phase != PH_DONE) {
        // consume f and g at the point asked for last
        for (int i = threadIdx.x; i < n; i += LB_THREADS) { const double gi = gin[i]; v.g[i] = round_f32 ? (double)(float)gi : gi; }
        if (threadIdx.x == 0) {
            double f;
            if (fin) f = *fin;
            else { double acc = 0.0; for (int k = 0; k < K; ++k) acc += costs[k]; f = acc / (double)K; }
            if (round_f32) f = (double)(float)f;
            s.f = f; s.f_last = f;
            if (!s.same) s.nfev += 1;
        }
        __syncthreads();
        if (phase == PH_START) {
            if (threadIdx.x == 0) s.phase = PH_SEARCH;
            __syncthreads();
            if (blk_absmax(v.g, n, s, sh) <= s.gtol) lb_finish(v, s, n, 4, 401, x_eval, theta32);
            else lb_search(v, s, n, sh, x_eval, theta32);
        } else {
            const double gd = blk_dot(v.g, v.d, n, s, sh);
            if (threadIdx.x == 0) {
                s.gd = gd;
                int act = dcsrch_step(s, s.f, gd);        // LS_FG: another trial; else a new iterate
                if (act == LS_FG) { s.ifun += 1; s.iback = s.ifun - 1; act = (s.iback >= s.maxls) ? -1 : LS_FG; }
                s.bcast_i = act;
            }
            __syncthreads();
            const int act = s.bcast_i;
            __syncthreads();
            if (act == LS_FG) lb_emit(v, s, n, x_eval, theta32);
            else if (act == -1) {
                lb_restore(v, s, n);
                const int col = s.col;
                __syncthreads();
                if (col == 0) lb_finish(v, s, n, 8, 0, x_eval, theta32);
                else {
                    if (threadIdx.x == 0) { s.col = 0; s.head = 0; s.theta = 1.0; }
                    __syncthreads();
                    lb_search(v, s, n, sh, x_eval, theta32);
                }
            } else {
                // NEW_X: the wrapper's counters, setulb's tests, the pair
                if (threadIdx.x == 0) {
                    s.nit += 1;
                    s.bcast_i = (s.nit >= s.maxiter) ? 504 : (s.nfev > s.maxfun) ? 502 : 0;
                }
                __syncthreads();
                const int lim = s.bcast_i;
                __syncthreads();
                if (lim) lb_finish(v, s, n, 5, lim, x_eval, theta32);
                else if (blk_absmax(v.g, n, s, sh) <= s.gtol) lb_finish(v, s, n, 4, 401, x_eval, theta32);
                else if (s.fold - s.f <= s.tol * fmax(fmax(fabs(s.fold), fabs(s.f)), 1.0)) lb_finish(v, s, n, 4, 402, x_eval, theta32);
                else {
                    const double stp = s.stp;
                    const double dr = (stp == 1.0) ? s.gd - s.gdold : (s.gd - s.gdold) * stp;
                    const double ddum = (stp == 1.0) ? -s.gdold : -s.gdold * stp;
                    if (!(dr <= LB_EPS * ddum)) {
                        const int m = s.m;
                        const int k = (s.col < m) ? (s.head + s.col) % m : s.head;
                        double* Sk = v.S + (size_t)k * n;
                        double* Yk = v.Y + (size_t)k * n;
                        for (int i = threadIdx.x; i < n; i += LB_THREADS) {
                            Yk[i] = v.g[i] - v.r[i];
                            Sk[i] = (stp == 1.0) ? v.d[i] : stp * v.d[i];
                        }
                        __syncthreads();
                        const double rr = blk_dot(Yk, Yk, n, s, sh);
                        if (threadIdx.x == 0) {
                            v.sy[k] = dr;
                            if (s.col < m) s.col += 1; else s.head = (s.head + 1) % m;
                            s.theta = rr / dr;
                        }
                        __syncthreads();
                    }
                    lb_search(v, s, n, sh, x_eval, theta32);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        if (task_out) { task_out[0] = s.task; task_out[1] = s.task_code; }
        s.pub[0] = s.task; s.pub[1] = s.task_code; s.pub[2] = s.nit; s.pub[3] = s.nfev; s.pub[4] = s.f_last;
        for (int i = 5; i < 14; ++i) s.pub[i] = 0.0;
        *v.sc = s;
    }
    __syncthreads();
    if (pub != nullptr) ls_publish(v.sc->pub, pub, stamp);
}

}  // namespace

int lbfgs_begin(metrpo_ctx* c, int n, const double* x0, const float* x0f, const metrpo_lbfgs_opts* o, double* x_eval, hipStream_t st) {
    int rc;
    if ((rc = ws_grow(c, c->d_lb, sizeof(double) * lb_doubles(n, o->m)))) return rc;
    LbScal s = {};
    s.theta = 1.0; s.gtol = o->gtol;
    s.tol = (o->ftol / LB_EPS) * LB_EPS;          // scipy passes factr = ftol / eps; setulb tests against factr * epsmch
    s.phase = PH_START; s.task = 3;
    s.n = n; s.m = o->m; s.maxls = o->maxls; s.maxiter = o->maxiter; s.maxfun = o->maxfun;
    const LbView v = lb_view(c->d_lb.p, n, o->m);
    hipLaunchKernelGGL(k_lbfgs_begin, dim3(1), dim3(LB_THREADS), 0, st, v, n, x0, x0f, s, x_eval);
    HIP_TRY(c, hipGetLastError());
    c->lb_n = n; c->lb_m = o->m; c->lb_open = 1;
    return METRPO_OK;
}

int lbfgs_iterate(metrpo_ctx* c, const double* f, const double* g, double* x_eval, int32_t* task, hipStream_t st) {
    const LbView v = lb_view(c->d_lb.p, c->lb_n, c->lb_m);
    hipLaunchKernelGGL(k_lbfgs_step, dim3(1), dim3(LB_THREADS), 0, st, v, f, (const double*)nullptr, 0, g, 0, x_eval, (float*)nullptr, task,
                       (double*)nullptr, 0ull);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

// The 'l-bfgs' branch: evaluations (metrpo_bptt_grad's sweeps, unchanged) and steps alternate on the stream; the host keeps `lookahead`
// of them in flight and reads the task each step published into its pinned slot, oldest first.  Evaluations enqueued after the step that
// ended the run see a frozen state and the final policy: they cost time, not correctness.
int run_lbfgs_policy(metrpo_ctx* c, const float* init, int B, int T, double gamma, const metrpo_lbfgs_opts* o, metrpo_lbfgs_result* out,
                     hipStream_t st) {
    const int P = c->pd.P, K = c->pd.K;
    int rc;
    if (!c->h_lb) {
        HIP_TRY(c, hipHostMalloc((void**)&c->h_lb, sizeof(double) * LB_SLOTS * LB_SLOT_DOUBLES));
        memset(c->h_lb, 0, sizeof(double) * LB_SLOTS * LB_SLOT_DOUBLES);
    }
    // the evaluation's outputs live after the state: costs [K] | grad [P]
    const size_t state = lb_doubles(P, o->m);
    if ((rc = ws_grow(c, c->d_lb, sizeof(double) * (state + K + P)))) return rc;
    if ((rc = lbfgs_begin(c, P, nullptr, c->d_theta.p, o, nullptr, st))) return rc;
    const LbView v = lb_view(c->d_lb.p, P, o->m);
    double* costs = c->d_lb.p + state;
    double* grad = costs + K;
    const unsigned long long base = c->lb_stamp;
    long long enq = 0, done_n = 0;
    int task = 3, code = 0;
    while (task == 3) {
        while (enq - done_n < o->lookahead) {
            if ((rc = launch_bptt_grad(c, init, B, T, gamma, costs, grad, st))) return rc;
            double* slot = c->h_lb + (size_t)(enq % LB_SLOTS) * LB_SLOT_DOUBLES;
            hipLaunchKernelGGL(k_lbfgs_step, dim3(1), dim3(LB_THREADS), 0, st, v, (const double*)nullptr, (const double*)costs, K, (const double*)grad,
                               o->round_f32 ? 1 : 0, (double*)nullptr, c->d_theta.p, (int32_t*)nullptr, slot, base + (unsigned long long)enq + 1);
            HIP_TRY(c, hipGetLastError());
            ++enq;
        }
        // the oldest step's task word (a busy wait as in metrpo_trpo_update_end, bounded; a stalled stream is synchronised to surface its fault)
        const double* slot = c->h_lb + (size_t)(done_n % LB_SLOTS) * LB_SLOT_DOUBLES;
        volatile unsigned long long* stamp = (volatile unsigned long long*)(slot + 16);
        const unsigned long long want = base + (unsigned long long)done_n + 1;
        const auto t0 = std::chrono::steady_clock::now();
        long spins = 0;
        while (*stamp != want) {
            if ((++spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                HIP_TRY(c, hipStreamSynchronize(st));
                if (*stamp != want) { c->lb_stamp = base + (unsigned long long)enq; return set_err(c, METRPO_EHIP, "lbfgs_policy: a step's task never arrived"); }
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        task = (int)slot[0]; code = (int)slot[1];
        ++done_n;
    }
    c->lb_stamp = base + (unsigned long long)enq;
    (void)code;
    if ((rc = lbfgs_get_result(c, out, st))) return rc;  // (synchronises: the evaluations still in flight, and the final state)
    if (c->mfma_cfg >= 0 && (rc = mfma_prepare_policy(c, st))) return rc;
    return METRPO_OK;
}

int lbfgs_get_result(metrpo_ctx* c, metrpo_lbfgs_result* out, hipStream_t st) {
    HIP_TRY(c, hipStreamSynchronize(st));
    LbScal s;
    HIP_TRY(c, hipMemcpy(&s, c->d_lb.p, sizeof(LbScal), hipMemcpyDeviceToHost));
    out->fun = s.f_last; out->nit = s.nit; out->nfev = s.nfev; out->task = s.task; out->task_code = s.task_code; out->pad_ = 0;
    out->status = (s.task == 4) ? 0 : ((s.nfev > s.maxfun || s.nit >= s.maxiter) ? 1 : 2);
    return METRPO_OK;
}
