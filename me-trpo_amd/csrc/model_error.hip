// metrpo_model_error / metrpo_model_error_windows (include/metrpo.h): the h-step open-loop prediction error of the dynamics ensemble against recorded
// real trajectories -- env_helpers.py:96-172 evaluate_model_predictions and :175-269 get_error_distribution of the reference, whose call sites
// (model_based_rl.py:619-651) sit commented out because on TF sessions the diagnostic costs more than the training it diagnoses.
//
// The reference rolls every horizon h out separately from the windows Os[:, :-h] (:143-156).  A deterministic rollout does not depend on how long it
// will run, so here ONE rollout of hmax = max(hs) steps from every window start serves all horizons: the state after h steps is row h of the
// trajectory.  k_window_starts gathers the starts, the rollout is metrpo_rollout's own dispatch (or, with known_actions, metrpo_rollout_actions' on the
// recorded actions, gathered per window by k_window_actions), k_pred_error compares and reduces in one pass.
//
// Both kernels are bandwidth-bound.  Trajectory tensors are time-major [h][W][ns]: the ns floats of 64 consecutive windows are one contiguous range of
// 64 * ns floats, and so are the recorded states they are compared against (consecutive windows of a trajectory are consecutive rows of Os), so a
// wave walks such a range with consecutive lanes on consecutive floats -- the pattern of k_gae and the Gram kernel on [T][B][w] (process.hip).
#include "metrpo_internal.h"
#include <algorithm>

namespace {

constexpr int ME_WG = 256;                                  // windows per workgroup = threads per workgroup
constexpr int ME_MAX_H = METRPO_MODEL_ERROR_MAX_HORIZONS;

// window w of a batch with Tw windows per trajectory -> row of Os [n][T+1][ns] it starts at
__device__ __forceinline__ long long window_row(int w, int Tw, int T, int& t) {
    const int i = w / Tw;
    t = w - i * Tw;
    return (long long)i * (T + 1) + t;
}

// d_init_obs [W][ns] <- Os[i, t] for window w = i * Tw + t.  One flat range: consecutive lanes read consecutive floats of a source row and write one
// contiguous, fully coalesced output range (subsample.hip's layout).
__global__ void __launch_bounds__(ME_WG) k_window_starts(const float* __restrict__ Os, float* __restrict__ dst, int W, int Tw, int T, int ns) {
    const long long n = (long long)W * ns;
    for (long long e = (long long)blockIdx.x * ME_WG + threadIdx.x; e < n; e += (long long)gridDim.x * ME_WG) {
        const int w = (int)(e / ns), j = (int)(e - (long long)w * ns);
        int t;
        const long long row = window_row(w, Tw, T, t);
        dst[e] = Os[row * ns + j];
    }
}

// known_actions: d_act [hmax][W][na] <- As[i, min(t + s, T - 1)] for every step s of the rollout in ONE launch (a window whose step s lies beyond its
// trajectory serves no horizon > s; the clamp keeps the read inside As).  Unclipped: metrpo_rollout_actions clips (env_helpers.py:216, :599).
__global__ void __launch_bounds__(ME_WG) k_window_actions(const float* __restrict__ As, float* __restrict__ dst, int W, int Tw, int T, int na, int hmax) {
    const long long per = (long long)W * na, n = per * hmax;
    for (long long e = (long long)blockIdx.x * ME_WG + threadIdx.x; e < n; e += (long long)gridDim.x * ME_WG) {
        const int s = (int)(e / per);
        const long long r = e - (long long)s * per;
        const int w = (int)(r / na), j = (int)(r - (long long)w * na);
        const int i = w / Tw, t = w - i * Tw;
        const int ts = min(t + s, T - 1);
        dst[e] = As[((long long)i * T + ts) * na + j];
    }
}

struct PredErrK {
    const float* obs;          // [hmax][W][ns] state BEFORE step s
    const float* rew;          // [hmax][W]
    const uint8_t* done;       // [hmax][W]
    const float* last_obs;     // [W][ns] state after step hmax - 1
    const float* Os;           // [n][T+1][ns]
    const float* Rs;           // [n][T]
    float* state_diff;         // [n_h][W][ns]
    float* cost_diff;          // [n_h][W]
    uint8_t* valid;            // [n_h][W]
    double* sums;              // [n_h][4]
    double* part;              // ticket | [gridDim.x][n_h][4]
    int W, Tw, T, ns, n_h, hmax, signed_diff;
    int hs[ME_MAX_H];
};

__global__ void __launch_bounds__(ME_WG) k_pred_error(PredErrK k) {
    __shared__ float s_cd[ME_MAX_H][ME_WG];                  // cost_diff of (horizon, window of this workgroup)
    __shared__ uint8_t s_valid[ME_MAX_H][ME_WG];
    __shared__ double s_wave[ME_WG / WAVE][4];
    __shared__ double s_part[ME_MAX_H][4];
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int W = k.W, T = k.T, ns = k.ns;
    const int w = blockIdx.x * ME_WG + tid;
    const bool active = w < W;

    // ---- pass over the window's own column: costs (env_helpers.py:153), rewards (:154), the done rule; all horizons in one walk ----
    {
        int t = 0;
        long long i = 0;
        if (active) { i = w / k.Tw; t = w - (int)i * k.Tw; }
        float costs = 0.0f, rewards = 0.0f;
        bool dead = false;
        int hp = 0;
        for (int s = 0; s < k.hmax; ++s) {
            if (active) {
                costs -= k.rew[(size_t)s * W + w];                                   // cost = -reward (env_helpers.py:601), added in step order
                if (t + s < T) rewards += k.Rs[i * T + t + s];
                dead = dead || (k.done[(size_t)s * W + w] != 0);                     // a done at any step < h = s + 1: the state behind it is a reset state
            }
            if (hp < k.n_h && k.hs[hp] == s + 1) {
                const int h = s + 1;
                const bool v = active && (t + h <= T) && !dead;                      // Os[:, :-h] / Os[:, h:] (:143-144)
                const float cd = v ? (k.signed_diff ? costs + rewards : fabsf(costs + rewards)) : 0.0f;   // :160
                s_cd[hp][tid] = cd; s_valid[hp][tid] = v ? 1 : 0;
                if (active) { k.cost_diff[(size_t)hp * W + w] = cd; k.valid[(size_t)hp * W + w] = v ? 1 : 0; }
                ++hp;
            }
        }
    }
    __syncthreads();

    // ---- per horizon: the ns columns of this wave's 64 windows as one flat range, then the workgroup's four sums ----
    const int wb = blockIdx.x * ME_WG + wave * WAVE;                                  // first window of this wave
    const int nv = max(0, min(WAVE, W - wb));
    for (int hp = 0; hp < k.n_h; ++hp) {
        const int h = k.hs[hp];
        const float* __restrict__ pred = (h < k.hmax) ? k.obs + (size_t)h * W * ns : k.last_obs;
        float* __restrict__ out = k.state_diff + (size_t)hp * W * ns;
        double a_state = 0.0, a_last = 0.0;
        for (int e = lane; e < nv * ns; e += WAVE) {
            const int wl = e / ns, j = e - wl * ns;
            const int ww = wb + wl;
            float d = 0.0f;
            if (s_valid[hp][wave * WAVE + wl]) {
                int t;
                const long long row = window_row(ww, k.Tw, T, t) + h;                 // Os[i, t + h]; t + h <= T: inside the trajectory
                const float real = k.Os[row * ns + j], p = pred[(size_t)ww * ns + j];
                d = k.signed_diff ? p - real : fabsf(real - p);                       // :159 (signed: o - real_final_states, :233)
                a_state += (double)d;
                if (j == ns - 1) a_last += (double)d;
            }
            out[(size_t)ww * ns + j] = d;
        }
        double q[4] = {s_valid[hp][tid] ? 1.0 : 0.0, a_state, a_last, (double)s_cd[hp][tid]};
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1)
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] += __shfl_xor(q[r], o, WAVE);
        if (lane == 0)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_wave[wave][r] = q[r];
        __syncthreads();
        if (tid < 4) {
            double a = 0.0;
            for (int v = 0; v < ME_WG / WAVE; ++v) a += s_wave[v][tid];
            s_part[hp][tid] = a;
        }
        __syncthreads();
    }

    // ---- the workgroups' partials, added IN WORKGROUP ORDER by whichever workgroup arrives last (k_gae's scheme, process.hip) ----
    unsigned int* ticket = (unsigned int*)k.part;
    double* gpart = k.part + 1;
    const int nq = k.n_h * 4;
    if (tid == 0) {
        for (int r = 0; r < nq; ++r) gpart[(size_t)blockIdx.x * nq + r] = s_part[r >> 2][r & 3];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == gridDim.x - 1) ? 1u : 0u;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (!s_last) return;
    if (tid < nq) {
        double a = 0.0;
        for (unsigned int j = 0; j < gridDim.x; ++j) a += __hip_atomic_load(gpart + (size_t)j * nq + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        k.sums[tid] = a;
    }
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int flat_grid(const metrpo_ctx* c, long long n) {
    const long long blocks = (n + ME_WG - 1) / ME_WG;
    return (int)std::max<long long>(1, std::min<long long>(blocks, (long long)c->n_sm * 8));
}

}  // namespace

int launch_window_starts(metrpo_ctx* c, const float* Os, int n, int T, int Tw, float* init_obs, hipStream_t st) {
    const int W = n * Tw;
    hipLaunchKernelGGL(k_window_starts, dim3(flat_grid(c, (long long)W * c->pd.ns)), dim3(ME_WG), 0, st, Os, init_obs, W, Tw, T, c->pd.ns);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int run_model_error(metrpo_ctx* c, const metrpo_model_error_args* a, hipStream_t st) {
    const int ns = c->pd.ns, na = c->pd.na;
    const int Tw = a->t0_only ? 1 : a->T;
    const int W = a->n * Tw, n_h = a->n_h, hmax = a->hs[n_h - 1];
    const bool dbg = a->d_dbg_obs != nullptr;
    const int nblk = (W + ME_WG - 1) / ME_WG;

    // ---- workspace: partials | trajectory of the rollout (none when the caller brought one) ----
    const size_t sz_part = up256(sizeof(double) * ((size_t)nblk * n_h * 4 + 1));
    { bool grew = false;
      const int rc = ws_grow(c, c->d_merr_part, std::max<size_t>(sz_part, 8192), &grew); if (rc) return rc;
      if (grew) HIP_TRY(c, hipMemsetAsync(c->d_merr_part.p, 0, c->d_merr_part.bytes, st)); }   // the ticket (first word) starts at zero; every launch leaves it there
    const float* t_obs = a->d_dbg_obs; const float* t_rew = a->d_dbg_rew; const uint8_t* t_done = a->d_dbg_done; const float* t_last = a->d_dbg_last_obs;
    if (!dbg) {
        const size_t HW = (size_t)hmax * W;
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
        const size_t o_obs = take(sizeof(float) * (HW + W) * ns);      // [hmax + 1][W][ns]: the step loop writes row s + 1; row hmax is its last_obs
        const size_t o_act = take(sizeof(float) * HW * na);
        const size_t o_mean = take(sizeof(float) * HW * na);
        const size_t o_rew = take(sizeof(float) * HW);
        const size_t o_tpath = take(sizeof(int32_t) * HW);
        const size_t o_done = take(HW);
        const size_t o_init = take(sizeof(float) * (size_t)W * ns);
        const size_t o_ts = take(sizeof(int32_t) * (size_t)W);
        const size_t o_model = take(sizeof(int32_t) * (size_t)W);
        { const int rc = ws_grow(c, c->d_merr, off); if (rc) return rc; }
        char* ws = (char*)c->d_merr.p;
        float* obs = (float*)(ws + o_obs); float* rew = (float*)(ws + o_rew); uint8_t* done = (uint8_t*)(ws + o_done);
        float* last = obs + HW * ns;
        int32_t* d_model = (int32_t*)(ws + o_model);
        const int one_head = a->model >= 0;
        // ONE_MODEL is head 0 in every kernel family, as in the reference (env_helpers.py:631-632); head `model` is EPS_RAND with every env's cur_model_idx = model
        const int sam = one_head ? METRPO_SAM_EPS_RAND : METRPO_SAM_MODEL_MEAN;
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)d_model, one_head ? a->model : 0, (size_t)W, st));
        if (!a->known_actions) {
            float* init = (float*)(ws + o_init);
            int32_t* d_ts = (int32_t*)(ws + o_ts);
            { const int rc = launch_window_starts(c, a->d_Os, a->n, a->T, Tw, init, st); if (rc) return rc; }
            HIP_TRY(c, hipMemsetAsync(d_ts, 0, sizeof(int32_t) * (size_t)W, st));
            metrpo_rollout_args r = {};
            r.B = W; r.T = hmax;
            r.H = hmax + 1;                      // the path-length limit never fires: a done in the trajectory is the env's own (Ant)
            r.sam_mode = sam; r.determ = 1; r.eval_all_heads = one_head ? 0 : 1;
            r.d_pool = init; r.n_pool = W;       // a finished env (Ant) resets onto some window start; k_pred_error drops it from there on
            r.d_obs = obs; r.d_act = (float*)(ws + o_act); r.d_rew = rew; r.d_mean = (float*)(ws + o_mean); r.d_done = done;
            r.d_tpath = (int32_t*)(ws + o_tpath); r.d_last_obs = last;
            r.d_init_obs = init; r.d_init_ts = d_ts; r.d_init_model = d_model;
            const int prec = c->dyn_precision;       // the diagnostic judges the f32 models whatever metrpo_set_dyn_precision says
            c->dyn_precision = METRPO_DYN_F32;
            const int rc = metrpo_rollout(c, &r, (void*)st);
            c->dyn_precision = prec;
            if (rc) return rc;
        } else {
            // get_error_distribution(known_actions=True) (env_helpers.py:216-222): the recorded actions of every step gathered once, then the body of
            // metrpo_rollout_actions (rollout_actions.hip) from the window starts in row 0 of obs
            { const int rc = launch_window_starts(c, a->d_Os, a->n, a->T, Tw, obs, st); if (rc) return rc; }
            float* act = (float*)(ws + o_act);
            hipLaunchKernelGGL(k_window_actions, dim3(flat_grid(c, (long long)HW * na)), dim3(ME_WG), 0, st, a->d_As, act, W, Tw, a->T, na, hmax);
            HIP_TRY(c, hipGetLastError());
            metrpo_rollout_actions_args ra = {};
            ra.B = W; ra.T = hmax; ra.sam_mode = sam; ra.uniform_model = one_head ? a->model : -1;
            ra.d_init_obs = obs; ra.d_actions = act; ra.d_model = d_model;
            ra.d_obs = obs; ra.d_rew = rew; ra.d_done = done;
            const int rc = run_rollout_actions(c, &ra, st);
            if (rc) return rc;
        }
        t_obs = obs; t_rew = rew; t_done = done; t_last = last;
    }

    PredErrK k = {};
    k.obs = t_obs; k.rew = t_rew; k.done = t_done; k.last_obs = t_last; k.Os = a->d_Os; k.Rs = a->d_Rs;
    k.state_diff = a->d_state_diff; k.cost_diff = a->d_cost_diff; k.valid = a->d_valid; k.sums = a->d_sums; k.part = c->d_merr_part.p;
    k.W = W; k.Tw = Tw; k.T = a->T; k.ns = ns; k.n_h = n_h; k.hmax = hmax; k.signed_diff = a->signed_diff ? 1 : 0;
    for (int i = 0; i < n_h; ++i) k.hs[i] = a->hs[i];
    hipLaunchKernelGGL(k_pred_error, dim3(nblk), dim3(ME_WG), 0, st, k);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}
