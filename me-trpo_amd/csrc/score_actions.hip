// metrpo_score_actions (include/metrpo.h): the discounted return every head of the ensemble predicts for each of B candidate action sequences -- per
// (head k, candidate b) the loop of build_policy_graph's cost sum, model_based_rl.py:122-141 (head fixed for the whole trajectory, the done mask updated
// AFTER the step's cost, :134-137), under SUPPLIED actions (clipped as VecSimpleEnv.step does, env_helpers.py:599) instead of the policy's.
//
// Fused kernel (k_score_actions): the ONE-head body of k_rollout_actions (rollout_actions.hip) without its stores -- dyn_tile_step.h's tile_rollout
// with a sink that sums instead of storing.
//   * one wave owns one (16-candidate tile, head) pair for all T steps, on the shared head of dyn_head_mfma.h: weight fragments register-resident
//     (swimmer 92, Ant 132 registers), biases and the tile's state in the wave's LDS, every activation in registers, no barrier.  The statements of a
//     step -- normalise, three layers, de-normalise, env_cost / env_done_scan (env_model.h) on the LDS rows -- are that kernel's own, so s' and r carry its bits.
//   * PACKING: one wave per workgroup on a (tiles, K) grid.  The (tile, head) pairs share nothing but read-only inputs, so a workgroup of several waves
//     would buy no exchange and no reuse; it would only tie the waves' placement together (a workgroup starts when ALL its waves fit one CU, and its LDS
//     and registers are held until the slowest tile of it ends).  One-wave workgroups let the dispatcher fill whatever SIMD has the registers free, which
//     is what matters below 1024 waves (B = 512, K = 5: 160 waves on 1024 SIMDs).  blockIdx.x is the tile: neighbouring workgroups read the same head's
//     weights (22 .. 26 KB, out of the cache) and neighbouring action blocks.
//   * the ONLY global load of the step loop is the tile's action block of the NEXT step, issued at the top of a step and read behind that step's matrix
//     instructions into the other of two LDS action buffers (k_rollout_actions).  There is NO global store inside the loop: every lane carries its env's
//     float64 sum, float64 discount (repeated multiplication), alive flag and step count; quad 0 writes d_ret / d_len once behind the loop.
//   * the tile's start rows are gathered per row (candidate b starts from d_init_obs[b / (B / S)]; a tile may straddle two start states).
//   * edge tile (B % 16 != 0): rows >= B are zero state and zero action in LDS, never read from or written to memory.
//
// Generic path (every other shape, and force_generic): per head k the step loop of run_rollout_actions (eps_rand, uniform_model = k) into a ctx
// workspace, chunked over candidates so that the workspace stays within 2^26 floats (score_chunk, metrpo_internal.h), then k_sact_reduce, one thread per candidate,
// applies the same float64 sum to the workspace's rew / done.
//
// Terminal value (metrpo_set_terminal_value; sact_sum.h: TermVal): while one is set, ret gains gamma^T alive_T V(s_T) in front of the single rounding.  Fused: tile_rollout
// leaves s_T in the wave's ST rows behind the loop and the sink's finish evaluates V there once per lane -- nothing is added inside the loop; the value is a
// template parameter of the kernel.  Generic: k_sact_reduce applies the same statement to row T of the chunk's stored trajectory.
//
// d_ret_mean / d_ret_std: k_sact_aggregate, a second small launch over d_ret, one thread per candidate adding in head order; no workgroup waits on another.
#include "dyn_tile_step.h"
#include "sact_sum.h"                 // SactSum: one step of the return
#include <algorithm>
#include <cmath>

struct SactK {
    int B, T, per;            // per = B / S: candidates per start state
    int stop;                 // 1: a candidate stops counting behind its first done
    double gamma;
    const float* init_obs; const float* actions;
    float* ret; int32_t* len;
    TermVal tv;               // the context's terminal value; unset: all NULL
};

// tile_rollout's sink that stores nothing inside the step loop: every lane carries its env's sum, quad 0 writes d_ret / d_len once behind the loop.
// TV: with a terminal value -- a template parameter, so that the kernel without one is the kernel it was (the runtime test's operands cost it 8 .. 14
// scalar registers held across the loop, and 0.3 .. 0.7 % of its time: profiles/r26_terminal_value.txt)
// TV_MLP: the two-layer tanh value, a further value of the same parameter (its two hidden rows take the registers the loop's fragments have released)
template <int TV>
struct SactSink {
    const SactK& r;
    SactSum acc;
    __device__ __forceinline__ void start(const float*, int, int, int) const {}
    __device__ __forceinline__ void step(int, const float*, float cost, bool dn, int, int, int) { acc.step(-cost, dn, r.gamma, r.stop); }
    // ST: the tile's rows behind the loop, s_T.  The terminal value is evaluated here, once per lane, in front of the single rounding
    template <int NS>
    __device__ __forceinline__ void finish(int k, int b0, int lane, const float* ST) {
        const int b = b0 + (lane & 15);
        if ((lane >> 4) == 0 && b < r.B) {                       // rounded to fp32 once, here
            if (TV) acc.terminal(r.tv.template value_of<TV>(ST + (lane & 15) * NS, 1, NS, b, r.per));
            const size_t kb = (size_t)k * r.B + b;
            r.ret[kb] = (float)acc.sum;
            if (r.len != nullptr) r.len[kb] = acc.n;
        }
    }
};

template <int ENV, int TV>
__global__ void __launch_bounds__(64) k_score_actions(SactK r, const float* __restrict__ dynp, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b0 = blockIdx.x * 16, k = blockIdx.y;
    const TileRollK tr = {r.B, r.T, r.per, r.init_obs, r.actions, k, 0, nullptr};
    SactSink<TV> sink = {r};
    tile_rollout<ENV, true>(lds, tr, 1, b0, dynp, norm, sink);
    sink.template finish<Cfg<ENV, 64, 32>::NS>(k, b0, threadIdx.x & 63, lds + Cfg<ENV, 64, 32>::W_ST);
}

// -------------------------------------------------------------------------------------------------
// Generic path.  k_sact_starts: row 0 of the chunk's trajectory <- the start state of candidates c0 .. c0 + Bc - 1, and (a chunk narrower than B) the
// chunk's columns of d_actions [T][B][na] -> [T][Bc][na].
__global__ void __launch_bounds__(256) k_sact_starts(const float* __restrict__ init_obs, const float* __restrict__ actions, int B, int T, int per, int c0, int Bc,
                                                     int ns, int na, float* __restrict__ obs0, float* __restrict__ act_c) {
    const size_t n_obs = (size_t)Bc * ns, n_act = act_c != nullptr ? (size_t)T * Bc * na : 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_obs + n_act; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n_obs) {
            const size_t row = i / ns, col = i - row * ns;
            obs0[i] = init_obs[(size_t)((c0 + (int)row) / per) * ns + col];
        } else {
            const size_t j = i - n_obs, t = j / ((size_t)Bc * na), rest = j - t * (size_t)Bc * na;
            act_c[j] = actions[(t * B + c0) * na + rest];
        }
    }
}
// k_sact_reduce: one thread per candidate of the chunk over the step loop's rew / done [T][Bc]; SactSum is the fused kernel's.  ret / len point at [k][c0].
// tv set: sT holds the chunk's states behind step T, [Bc][ns]; c0 is the chunk's first candidate (the bias row is (c0 + i) / per).
// MLP: the value is the two-layer net (a template parameter: the instantiation without it is the kernel it was).
template <bool MLP>
__global__ void __launch_bounds__(256) k_sact_reduce(const float* __restrict__ rew, const uint8_t* __restrict__ done, int Bc, int T, int stop, double gamma,
                                                     float* __restrict__ ret, int32_t* __restrict__ len, TermVal tv, const float* __restrict__ sT, int ns, int c0, int per) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Bc) return;
    SactSum acc;
    for (int t = 0; t < T; ++t) acc.step(rew[(size_t)t * Bc + i], done[(size_t)t * Bc + i] != 0, gamma, stop);
    if constexpr (MLP) acc.terminal(tv.mlp_value(sT + (size_t)i * ns, 1, ns, c0 + i, per));
    else if (tv.set()) acc.terminal(tv.value(sT + (size_t)i * ns, 1, ns, c0 + i, per));
    ret[i] = (float)acc.sum;
    if (len != nullptr) len[i] = acc.n;
}

// d_ret_mean / d_ret_std from the stored fp32 returns [K][B]: the mean in head order divided by K, the population std two-pass by fmaf in head order --
// rew_std's arithmetic in disagreement.hip.  K = 1: d = r - r / 1 = 0 exactly.
__global__ void __launch_bounds__(256) k_sact_aggregate(const float* __restrict__ ret, int B, int K, float* __restrict__ mean, float* __restrict__ sd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float fK = (float)K;
    float rs = 0.0f;
    for (int k = 0; k < K; ++k) rs += ret[(size_t)k * B + b];
    const float rm = rs / fK;
    if (mean != nullptr) mean[b] = rm;
    if (sd != nullptr) {
        float rv = 0.0f;
        for (int k = 0; k < K; ++k) { const float d = ret[(size_t)k * B + b] - rm; rv = fmaf(d, d, rv); }
        sd[b] = sqrtf(rv / fK);
    }
}

// the three launches above for score_policy_actions.hip as well (metrpo_internal.h); none of them reports an error of its own
void launch_sact_starts(const float* init_obs, const float* actions, int B, int T, int per, int c0, int Bc, int ns, int na, float* obs0, float* act_c, hipStream_t st) {
    const size_t work = (size_t)Bc * ns + (act_c ? (size_t)T * Bc * na : 0);
    hipLaunchKernelGGL(k_sact_starts, dim3((unsigned)std::min<size_t>((work + 255) / 256, 4096)), dim3(256), 0, st, init_obs, actions, B, T, per, c0, Bc, ns, na, obs0, act_c);
}
void launch_sact_reduce(const float* rew, const uint8_t* done, int Bc, int T, int stop, double gamma, float* ret, int32_t* len, const TermVal& tv, bool mlp, const float* sT, int ns,
                        int c0, int per, hipStream_t st) {
    hipLaunchKernelGGL(mlp ? k_sact_reduce<true> : k_sact_reduce<false>, dim3((Bc + 255) / 256), dim3(256), 0, st, rew, done, Bc, T, stop, gamma, ret, len, tv, sT, ns, c0, per);
}
void launch_sact_aggregate(const float* ret, int B, int K, float* mean, float* sd, hipStream_t st) {
    hipLaunchKernelGGL(k_sact_aggregate, dim3((B + 255) / 256), dim3(256), 0, st, ret, B, K, mean, sd);
}

// metrpo_set_terminal_value_mlp: the context's image of the net (sact_sum.h: tvm_*) from the caller's packed parameters
//   W0 [ns][h1] | b0 [h1] | W1 [h1][h2] | b1 [h2] | W2 [h2] | b2, the hidden widths padded with zeros to TVM, and the biases behind it.  One thread per float of the image.
__global__ void __launch_bounds__(256) k_tv_mlp_image(const float* __restrict__ par, int ns, int h1, int h2, const float* __restrict__ bias, int n_bias, float* __restrict__ img) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_img = tvm_floats(ns);
    if (i >= n_img + n_bias) return;
    if (i >= n_img) { img[i] = bias[i - n_img]; return; }
    const float* W0 = par; const float* b0 = W0 + ns * h1; const float* W1 = b0 + h1; const float* b1 = W1 + h1 * h2; const float* W2 = b1 + h2; const float* b2 = W2 + h2;
    float v = 0.0f;
    if (i < tvm_b0(ns)) { const int d = i / TVM, u = i % TVM; if (u < h1) v = W0[d * h1 + u]; }
    else if (i < tvm_w1(ns)) { const int u = i - tvm_b0(ns); if (u < h1) v = b0[u]; }
    else if (i < tvm_b1(ns)) { const int j = i - tvm_w1(ns), w = j / TVM, u = j % TVM; if (u < h1 && w < h2) v = W1[u * h2 + w]; }      // out-major: row w holds unit w's inputs
    else if (i < tvm_w2(ns)) { const int w = i - tvm_b1(ns); if (w < h2) v = b1[w]; }
    else { const int w = i - tvm_w2(ns); if (w < h2) v = W2[w]; else if (w == TVM) v = b2[0]; }
    img[i] = v;
}
// ... context state like metrpo_set_terminal_value's: the one growth path (an outgrown buffer is retired, not freed), one stream-ordered launch, no synchronisation
int run_set_terminal_value_mlp(metrpo_ctx* c, const float* d_params, int h1, int h2, const float* d_bias, int n_bias, hipStream_t st) {
    const int ns = c->pd.ns;
    const size_t total = (size_t)tvm_floats(ns) + (size_t)n_bias;
    { const int rc = ws_grow(c, c->d_tv, sizeof(float) * total); if (rc) { c->tv_n_bias = 0; return rc; } }
    c->tv_n_bias = 0;                                            // a failed launch leaves none set
    hipLaunchKernelGGL(k_tv_mlp_image, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_params, ns, h1, h2, d_bias, n_bias, c->d_tv.p);
    HIP_TRY(c, hipGetLastError());
    c->tv_n_bias = n_bias; c->tv_kind = TV_MLP;
    return METRPO_OK;
}

// -------------------------------------------------------------------------------------------------
typedef void (*sact_kernel_t)(SactK, const float*, const float*);
struct SactEntry { int env; sact_kernel_t kern[3]; int w_sz; };      // kern[the terminal value's kind]
#define SENTRY(ENVID) {ENVID, {k_score_actions<ENVID, TV_NONE>, k_score_actions<ENVID, TV_QUAD>, k_score_actions<ENVID, TV_MLP>}, act_wave_floats<ENVID>()}
static const SactEntry kSact[] = {FUSED_HEAD_ENVS(SENTRY)};

static int launch_sact_fused(metrpo_ctx* c, const SactEntry& en, bool padded, const metrpo_score_actions_args* a, hipStream_t st) {
    SactK r = {};
    r.B = a->B; r.T = a->T; r.per = a->B / a->S; r.stop = a->stop_at_done ? 1 : 0; r.gamma = a->gamma;
    r.init_obs = a->d_init_obs; r.actions = a->d_actions; r.ret = a->d_ret; r.len = a->d_len; r.tv = ctx_term_val(c);
    const float* dyn;
    { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
    const size_t sh = sizeof(float) * (size_t)en.w_sz;
    hipLaunchKernelGGL(en.kern[ctx_tv_kind(c)], dim3((a->B + 15) / 16, c->pd.K), dim3(64), sh, st, r, dyn, c->d_norm.p);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

static int launch_sact_generic(metrpo_ctx* c, const metrpo_score_actions_args* a, hipStream_t st) {
    const size_t ns = c->pd.ns, na = c->pd.na, B = a->B, T = a->T;
    const int K = c->pd.K, per = a->B / a->S;
    // ---- a chunk's workspace (floats): obs [T + 1][Bc][ns] | rew [T][Bc] | done [T][Bc] bytes | (Bc < B) actions [T][Bc][na]; within 2^26 floats ----
    const size_t per_cand = (T + 1) * ns + T + (T + 3) / 4 + T * na;
    const size_t Bc = score_chunk(B, per_cand);
    const size_t o_obs = 0, o_rew = o_obs + (T + 1) * Bc * ns, o_done = o_rew + T * Bc, o_act = o_done + (T * Bc + 3) / 4;
    const size_t total = o_act + (Bc < B ? T * Bc * na : 0);
    { const int rc = ws_grow(c, c->d_sact, sizeof(float) * total); if (rc) return rc; }
    float* ws = (float*)c->d_sact.p;
    const int keep_ract = c->last_ract_kernel;                   // run_rollout_actions reports itself there; this entry point leaves it untouched
    int rc = METRPO_OK;
    for (size_t c0 = 0; c0 < B && rc == METRPO_OK; c0 += Bc) {
        const int n = (int)std::min(Bc, B - c0);
        float* act_c = Bc < B ? ws + o_act : nullptr;
        launch_sact_starts(a->d_init_obs, a->d_actions, a->B, a->T, per, (int)c0, n, (int)ns, (int)na, ws + o_obs, act_c, st);
        if (hipGetLastError() != hipSuccess) { rc = set_err(c, METRPO_EHIP, "score_actions: launch failed"); break; }
        metrpo_rollout_actions_args ra = {};
        ra.B = n; ra.T = a->T; ra.sam_mode = METRPO_SAM_EPS_RAND; ra.force_step_loop = 1;
        ra.d_init_obs = ws + o_obs; ra.d_actions = act_c ? act_c : a->d_actions;
        ra.d_obs = ws + o_obs; ra.d_rew = ws + o_rew; ra.d_done = (uint8_t*)(ws + o_done);
        for (int k = 0; k < K && rc == METRPO_OK; ++k) {
            ra.uniform_model = k;
            rc = run_rollout_actions(c, &ra, st);
            if (rc) break;
            launch_sact_reduce(ra.d_rew, ra.d_done, n, a->T, a->stop_at_done ? 1 : 0, a->gamma, a->d_ret + (size_t)k * B + c0,
                               a->d_len ? a->d_len + (size_t)k * B + c0 : nullptr, ctx_term_val(c), ctx_tv_kind(c) == TV_MLP, ra.d_obs + T * n * ns, (int)ns, (int)c0, per, st);      // row T of the chunk's trajectory
            if (hipGetLastError() != hipSuccess) rc = set_err(c, METRPO_EHIP, "score_actions: launch failed");
        }
    }
    c->last_ract_kernel = keep_ract;
    return rc;
}

int run_score_actions(metrpo_ctx* c, const metrpo_score_actions_args* a, hipStream_t st) {
    bool padded = false;
    const SactEntry* en = a->force_generic ? nullptr : fused_head_entry(kSact, c, 65535, &padded);      // the heads are gridDim.y: no workgroup holds a wave per head
    const int rc = en != nullptr ? launch_sact_fused(c, *en, padded, a, st) : launch_sact_generic(c, a, st);
    if (rc) return rc;
    if (a->d_ret_mean != nullptr || a->d_ret_std != nullptr) {
        launch_sact_aggregate(a->d_ret, a->B, c->pd.K, a->d_ret_mean, a->d_ret_std, st);
        HIP_TRY(c, hipGetLastError());
    }
    c->last_sact_kernel = en != nullptr ? 1 : 0;
    return METRPO_OK;
}
