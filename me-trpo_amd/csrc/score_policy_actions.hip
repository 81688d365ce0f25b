// metrpo_score_policy_actions (include/metrpo.h): the discounted return every head of the ensemble predicts for each of B candidate NOISE sequences
// around the policy -- metrpo_score_actions (score_actions.hip) with the action of every step formed inside the loop, a_t = pi(s_t) (+ noise_t), from
// the head's OWN state.  Per (head k, candidate b) the loop of build_policy_graph's cost sum, model_based_rl.py:122-141 (head fixed for the whole
// trajectory, the done mask updated AFTER the step's cost, :134-137) with get_actions' mean net and, optionally, its noise arithmetic.
//
// Fused kernel (k_score_policy_actions): k_score_actions' mapping with the policy chain of pol_head_mfma.h in front of the dynamics head's step.
//   * one wave owns one (16-candidate tile, head) pair for all T steps, one-wave workgroups on a (tiles, K) grid (score_actions.hip: PACKING); the head's
//     weight fragments AND the policy's (swimmer 30, Ant 40 registers more) are register-resident, all six bias rows and the tile's state live in the
//     wave's LDS (pol_wave_floats<>), every activation in registers, no barrier.
//   * a step: policy mean from ST (two tanh layers on the dependent chain), a = mean (+ noise, fmaf with sigma: sigma = 1 gives mean + noise exactly),
//     the clipped action into the tile's ACT rows IN PLACE of the noise it was formed from (every lane overwrites only what it read), then
//     DynWaveHead::step, env_cost / env_done_scan (env_model.h) on the LDS rows and SactSum -- the statements of tile_rollout's one-head body (dyn_tile_step.h), so fed
//     the same clipped action the step carries k_score_actions' bits (d_act_out replayed through metrpo_score_actions reproduces ret).
//   * the ONLY global load of the step loop is the tile's noise block of the NEXT step, issued at the top of a step and committed UNCLIPPED behind
//     that step's matrix instructions into the other of two LDS buffers (NoiseTile: ActTile's prefetch, its own commit).  d_noise NULL: a variant with
//     no global load in the loop at all.  There is no global store inside the loop unless d_act_out is asked for: a compile-time variant of its own.
//   * start rows, edge tiles (rows >= B: zero state, zero noise, never read from or written to memory) and padded ensembles as in score_actions.hip.
//
//   * terminal value (sact_sum.h: TermVal): behind the loop ST holds s_T; V is evaluated there once per lane in front of the single rounding (a template
//     parameter TV = the value's kind, as in score_actions.hip; nothing inside the loop).  Generic path: k_sact_reduce reads the last step's s_out.
//
// Generic path (every other shape, and force_generic): per chunk of candidates (workspace within 2^26 floats), per head k, per step t the library's
// own policy forward (launch_policy_actions: noise_in_std = 1 hands the noise row in as its eps), k_spol_act where mean + noise has to be formed or
// the action copied out, launch_step (eps_rand, the head fixed) into the other of two state rows; k_sact_reduce applies the float64 sum at the end.
#include "dyn_tile_step.h"
#include "pol_head_mfma.h"
#include "sact_sum.h"
#include <algorithm>
#include <cmath>

struct SpolK {
    int B, T, per;            // per = B / S: candidates per start state
    int stop;                 // 1: a candidate stops counting behind its first done
    int in_std;               // 1: the noise is in units of the policy's std
    double gamma;
    const float* init_obs; const float* noise;
    float* ret; int32_t* len; float* act_out;
    TermVal tv;               // the context's terminal value; unset: all NULL
};

template <int ENV, bool NOISE, bool AOUT, int TV>
__global__ void __launch_bounds__(64) k_score_policy_actions(SpolK r, const float* __restrict__ dynp, const float* __restrict__ theta, const float* __restrict__ norm) {
    using C = Cfg<ENV, 64, 32>;
    constexpr int NS = C::NS, NA = C::NA, NST = cdiv(16 * NS, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, e = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16, k = blockIdx.y, b = b0 + e;
    const int nrows = min(16, r.B - b0);                      // rows of this tile inside the batch
    float* W = lds;
    float* ST = W + C::W_ST;  float* NX = W + C::W_NX;

    DynWaveHead<C> head;
    head.load(dynp + (size_t)k * C::PD, norm, W + C::W_BD0, W + C::W_BD1, W + C::W_BD2, lane);
    PolWaveHead<C> pol;
    pol.load(theta, W + C::W_BP0, W + C::W_BP1, W + C::W_BP2, lane);
    // sigma of this lane's action dims; 1 when the noise is added as it is.  expf, as the fused rollout kernels form it (rollout_mfma.hip); the generic
    // path's k_policy_actions uses __expf (rollout_generic.hip): the two paths agree to rounding in sigma, not bits
    float sig[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) sig[rr] = (NOISE && r.in_std && 4 * q + rr < NA) ? expf(fmaxf(theta[C::pLS + 4 * q + rr], LOG_MIN_STD)) : 1.0f;
    // ---------------- the tile's start rows (gathered per row: a tile may straddle two start states) and the noise of step 0 -----------
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = lane + 64 * j;
        const int row = i / NS, col = i - row * NS;
        if (i < 16 * NS) ST[i] = (row < nrows) ? r.init_obs[(size_t)((b0 + row) / r.per) * NS + col] : 0.0f;
    }
    NoiseTile<C> nz;
    if (NOISE) {
        nz.init(r.noise, r.B, r.T, b0, nrows, lane, W, C::W_ACT, al4(C::W_TOTAL));
        nz.prefetch(0);
        nz.commit(0);
    }
    wave_lds_sync();
    loop_invariant_loads_done();

    SactSum acc;
    for (int t = 0; t < r.T; ++t) {
        float* ACT = NOISE ? nz.cur(t) : W + C::W_ACT;       // the step's noise rows, overwritten by the clipped action
        if (NOISE) nz.prefetch(t + 1);                         // committed behind the matrix instructions
        const f32x4 mu = pol.mean(ST, e);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int d = 4 * q + rr;
            if (d < NA) {
                float a = mu[rr];
                if (NOISE) a = fmaf(ACT[e * NA + d], sig[rr], a);
                if (AOUT && b < r.B) r.act_out[(((size_t)k * r.T + t) * r.B + b) * NA + d] = a;
                ACT[e * NA + d] = fminf(fmaxf(a, -1.0f), 1.0f);            // np.clip(actions, *bounds), env_helpers.py:599
            }
        }
        wave_lds_sync();
        f32x4 nx[C::OUT_CB];
        head.step(nx, ST, NS, ACT, e);
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) NX[e * NS + dim] = nx[cb][rr];
            }
        if (NOISE) nz.commit(t + 1);                           // the loop's only wait for a load
        wave_lds_sync();
        const float cost = env_cost(ENV, NS, NA, EnvVec{NX + e * NS, 1}, EnvVec{ACT + e * NA, 1});
        const bool dn = env_done_scan(ENV, NS, EnvVec{NX + e * NS, 1});
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NS) ST[i] = NX[i];
        }
        wave_lds_sync();
        acc.step(-cost, dn, r.gamma, r.stop);
    }
    if (q == 0 && b < r.B) {                                   // rounded to fp32 once, here
        if (TV) acc.terminal(r.tv.template value_of<TV>(ST + e * NS, 1, NS, b, r.per));               // ST holds s_T behind the loop
        const size_t kb = (size_t)k * r.B + b;
        r.ret[kb] = (float)acc.sum;
        if (r.len != nullptr) r.len[kb] = acc.n;
    }
}

// -------------------------------------------------------------------------------------------------
// Generic path.  k_spol_act: the action of a chunk's step from the policy launch's output -- act <- act + noise where the noise is added as it is
// (the launch left the mean there), and a copy into the chunk's rows of d_act_out.
__global__ void __launch_bounds__(256) k_spol_act(float* __restrict__ act, const float* __restrict__ noise, float* __restrict__ act_out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = act[i];
    if (noise != nullptr) { a = a + noise[i]; act[i] = a; }
    if (act_out != nullptr) act_out[i] = a;
}
// the K head vectors of a chunk, [K][n]: row k is launch_step's model_idx with every env on head k
__global__ void __launch_bounds__(256) k_spol_heads(int32_t* __restrict__ model, int n, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * K) model[i] = i / n;
}

// -------------------------------------------------------------------------------------------------
typedef void (*spol_kernel_t)(SpolK, const float*, const float*, const float*);
struct SpolEntry { int env; spol_kernel_t kern[3][2][2]; int w_sz; };      // kern[the terminal value's kind][noise][act_out]
#define PKERNS(ENVID, TV) {{k_score_policy_actions<ENVID, false, false, TV>, k_score_policy_actions<ENVID, false, true, TV>},   \
                           {k_score_policy_actions<ENVID, true, false, TV>, k_score_policy_actions<ENVID, true, true, TV>}}
#define PENTRY(ENVID) {ENVID, {PKERNS(ENVID, TV_NONE), PKERNS(ENVID, TV_QUAD), PKERNS(ENVID, TV_MLP)}, pol_wave_floats<ENVID>()}
static const SpolEntry kSpol[] = {FUSED_HEAD_ENVS(PENTRY)};

static int launch_spol_fused(metrpo_ctx* c, const SpolEntry& en, bool padded, const metrpo_score_policy_actions_args* a, hipStream_t st) {
    SpolK r = {};
    r.B = a->B; r.T = a->T; r.per = a->B / a->S; r.stop = a->stop_at_done ? 1 : 0; r.in_std = a->noise_in_std ? 1 : 0; r.gamma = a->gamma;
    r.init_obs = a->d_init_obs; r.noise = a->d_noise; r.ret = a->d_ret; r.len = a->d_len; r.act_out = a->d_act_out; r.tv = ctx_term_val(c);
    const float* dyn;
    { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
    const spol_kernel_t kern = en.kern[ctx_tv_kind(c)][a->d_noise != nullptr ? 1 : 0][a->d_act_out != nullptr ? 1 : 0];
    const size_t sh = sizeof(float) * (size_t)en.w_sz;
    { const int rc = allow_dynamic_lds(c, (const void*)kern, sh); if (rc) return rc; }
    hipLaunchKernelGGL(kern, dim3((a->B + 15) / 16, c->pd.K), dim3(64), sh, st, r, dyn, c->d_theta.p, c->d_norm.p);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

static int launch_spol_generic(metrpo_ctx* c, const metrpo_score_policy_actions_args* a, hipStream_t st) {
    const size_t ns = c->pd.ns, na = c->pd.na, B = a->B, T = a->T;
    const int K = c->pd.K, per = a->B / a->S;
    // ---- a chunk's workspace (floats): start [Bc][ns] | two state rows [2][Bc][ns] | act [Bc][na] | mean [Bc][na] | rew [T][Bc] | done [T][Bc] bytes | heads [K][Bc] int32.
    // A chunk of n < Bc candidates (the last one) uses the front of every area with n as its row stride: rew / done are [T][n], as k_sact_reduce reads them.
    // `mean` is never read: launch_policy_actions writes both of its outputs.  spol_chunk_cap (metrpo_debug_score_policy_chunk) lowers Bc for tests. ----
    const size_t per_cand = 3 * ns + 2 * na + T + (T + 3) / 4 + K;
    size_t Bc = score_chunk(B, per_cand);
    if (c->spol_chunk_cap > 0) Bc = std::min<size_t>(Bc, (size_t)c->spol_chunk_cap);
    const size_t o_s0 = 0, o_st = o_s0 + Bc * ns, o_act = o_st + 2 * Bc * ns, o_mean = o_act + Bc * na, o_rew = o_mean + Bc * na, o_done = o_rew + T * Bc,
                 o_head = o_done + (T * Bc + 3) / 4, total = o_head + (size_t)K * Bc;
    { const int rc = ws_grow(c, c->d_spol, sizeof(float) * total); if (rc) return rc; }
    float* ws = (float*)c->d_spol.p;
    const bool add = a->d_noise != nullptr && !a->noise_in_std;
    for (size_t c0 = 0; c0 < B; c0 += Bc) {
        const int n = (int)std::min(Bc, B - c0);
        launch_sact_starts(a->d_init_obs, nullptr, a->B, a->T, per, (int)c0, n, (int)ns, (int)na, ws + o_s0, nullptr, st);
        if (hipGetLastError() != hipSuccess) return set_err(c, METRPO_EHIP, "score_policy_actions: launch failed");
        hipLaunchKernelGGL(k_spol_heads, dim3((n * K + 255) / 256), dim3(256), 0, st, (int32_t*)(ws + o_head), n, K);
        if (hipGetLastError() != hipSuccess) return set_err(c, METRPO_EHIP, "score_policy_actions: launch failed");
        for (int k = 0; k < K; ++k) {
            for (size_t t = 0; t < T; ++t) {
                const float* s_in = t == 0 ? ws + o_s0 : ws + o_st + (t & 1) * Bc * ns;
                float* s_out = ws + o_st + ((t + 1) & 1) * Bc * ns;
                const float* nz = a->d_noise ? a->d_noise + (t * B + c0) * na : nullptr;
                float* ao = a->d_act_out ? a->d_act_out + (((size_t)k * T + t) * B + c0) * na : nullptr;
                int rc = launch_policy_actions(c, s_in, add ? nullptr : nz, n, ws + o_act, ws + o_mean, st);
                if (rc) return rc;
                if (add || ao != nullptr) {
                    hipLaunchKernelGGL(k_spol_act, dim3((n * (int)na + 255) / 256), dim3(256), 0, st, ws + o_act, add ? nz : nullptr, ao, n * (int)na);
                    if (hipGetLastError() != hipSuccess) return set_err(c, METRPO_EHIP, "score_policy_actions: launch failed");
                }
                rc = launch_step(c, s_in, ws + o_act, n, METRPO_SAM_EPS_RAND, (const int32_t*)(ws + o_head) + (size_t)k * n, nullptr, s_out, ws + o_rew + t * n,
                                 (uint8_t*)(ws + o_done) + t * n, nullptr, st);
                if (rc) return rc;
            }
            launch_sact_reduce(ws + o_rew, (const uint8_t*)(ws + o_done), n, a->T, a->stop_at_done ? 1 : 0, a->gamma, a->d_ret + (size_t)k * B + c0,
                               a->d_len ? a->d_len + (size_t)k * B + c0 : nullptr, ctx_term_val(c), ctx_tv_kind(c) == TV_MLP, ws + o_st + (T & 1) * Bc * ns, (int)ns, (int)c0, per, st);      // the last step's s_out
            if (hipGetLastError() != hipSuccess) return set_err(c, METRPO_EHIP, "score_policy_actions: launch failed");
        }
    }
    return METRPO_OK;
}

// Test hook, exported besides the header's ABI like metrpo_set_coop_split (no option key: existing tests pin the table at 25): at most `cap` candidates per
// chunk of the generic path; 0: the library's rule alone.  Chunking changes no bit of any output.
extern "C" int32_t metrpo_debug_score_policy_chunk(metrpo_ctx* c, int32_t cap) {
    if (!c) return METRPO_ENULL;
    if (cap < 0) return set_err(c, METRPO_EINVAL, "debug_score_policy_chunk: cap must not be negative");
    c->spol_chunk_cap = cap;
    return METRPO_OK;
}

int run_score_policy_actions(metrpo_ctx* c, const metrpo_score_policy_actions_args* a, hipStream_t st) {
    bool padded = false;
    const SpolEntry* en = a->force_generic ? nullptr : fused_head_entry(kSpol, c, 65535, &padded);      // the heads are gridDim.y; the class holds the 2 x 32 tanh policy
    const int rc = en != nullptr ? launch_spol_fused(c, *en, padded, a, st) : launch_spol_generic(c, a, st);
    if (rc) return rc;
    if (a->d_ret_mean != nullptr || a->d_ret_std != nullptr) {
        launch_sact_aggregate(a->d_ret, a->B, c->pd.K, a->d_ret_mean, a->d_ret_std, st);
        HIP_TRY(c, hipGetLastError());
    }
    c->last_spol_kernel = en != nullptr ? 1 : 0;
    return METRPO_OK;
}
