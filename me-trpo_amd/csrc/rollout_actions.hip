// metrpo_rollout_actions (include/metrpo.h): the ensemble rolled forward under SUPPLIED actions -- the loop of get_error_distribution(known_actions=True),
// env_helpers.py:216-222, over VecSimpleEnv.step's arithmetic, :597-603.  T chained metrpo_step calls in meaning: no policy, no reset, no path-length
// limit, no draw; stepping continues behind a done.
//
// Fused kernel (k_rollout_actions): rollout_mfma.hip's dynamics step without the policy, the action read from memory instead.  Its body is
// dyn_tile_step.h's tile_rollout (shared with k_score_actions) with the sink below, which stores the trajectory; what follows describes that body.
//   * one workgroup = one tile of 16 envs, walked through all T steps, on the shared head of dyn_head_mfma.h (layout and arithmetic are described there).
//   * the head's weight fragments are register-resident for the whole loop (swimmer 92, Ant 132 registers), biases, normalisers' source map and the
//     tile's state live in LDS; the state is [env][ns], the layout of one row of d_obs, so a row is one linear coalesced store.
//   * cost and is_done are env_model.h's env_cost / env_done_scan on the LDS rows (the functions metrpo_step's kernel calls).
//   * the ONLY global load of the step loop is the tile's action block of the NEXT step (16 * na contiguous floats of d_actions, <= 2 per lane), issued
//     at the top of a step and read behind that step's matrix instructions into the other of two LDS action buffers -- IN FRONT of the step's stores.
//     The vector-memory counter is in order, so the wait for a load is also a wait for every older store (rollout_coop_kernel.h, DRAWS): placed
//     there, the only stores it can meet are those of the step before, a whole step of matrix work old; the step's own stores have a step to drain.
//   * ALL heads (model_mean; eps_rand with a per-env head vector): wave k of the workgroup owns head k (K <= 8 waves), the K next states meet in LDS with
//     ONE barrier per step (double-buffered), every wave then selects or averages redundantly -- in head order k = 0 .. K-1, divided by K, as metrpo_step.
//   * ONE head (one_model; eps_rand with uniform_model): ONE WAVE PER TILE, not one head split over four waves.  A split needs the layer's activations
//     back in LDS and a barrier between layers (the cooperative kernel's scheme), which is what this kernel is asked to avoid; one wave keeps every
//     activation in registers and has no barrier at all.  Its cost: the three layers' dependent MFMA chains are not shortened, and at fewer than 1024
//     tiles (B < 16 384) some SIMDs stay idle.  profiles/r13_rollout_actions.txt has the figure.
//   * edge tile (B % 16 != 0): rows >= B are zero state and zero action in LDS, never read from or written to memory.
//
// Step loop (everything the fused kernel does not hold): launch_step on row t of d_actions, writing row t + 1 of d_obs.  No gather, no action copy.
#include "dyn_tile_step.h"

struct RactK {
    int B, T;
    int mean;                 // ALL: 1 = average the heads (model_mean), 0 = select model[b] (eps_rand)
    int head;                 // ONE: the head
    const float* init_obs; const float* actions; const int32_t* model;
    float* obs; float* rew; uint8_t* done;
};

// tile_rollout's sink that stores the trajectory: a row of d_obs is the tile's LDS state as one linear coalesced store
template <int NS>
struct RactSink {
    static constexpr int NST = cdiv(16 * NS, 64);
    const RactK& r;
    __device__ __forceinline__ void rows(float* __restrict__ orow, const float* ST, int nrows, int lane) const {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < nrows * NS) orow[i] = ST[i];
        }
    }
    // row 0 of d_obs = d_init_obs, bit for bit
    __device__ __forceinline__ void start(const float* ST, int b0, int nrows, int lane) const { rows(r.obs + (size_t)b0 * NS, ST, nrows, lane); }
    // row t + 1 of d_obs, reward = -cost and done of step t; the env goes on either way
    __device__ __forceinline__ void step(int t, const float* ST, float cost, bool dn, int b0, int nrows, int lane) const {
        rows(r.obs + ((size_t)(t + 1) * r.B + b0) * NS, ST, nrows, lane);
        const int b = b0 + (lane & 15);
        if ((lane >> 4) == 0 && b < r.B) { const size_t tb = (size_t)t * r.B + b; r.rew[tb] = -cost; r.done[tb] = dn ? 1 : 0; }
    }
};

template <int ENV, bool ONE>
__global__ void __launch_bounds__(ONE ? 64 : 512) k_rollout_actions(RactK r, int K, const float* __restrict__ dynp, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TileRollK tr = {r.B, r.T, 1, r.init_obs, r.actions, r.head, r.mean, r.model};
    RactSink<Cfg<ENV, 64, 32>::NS> sink = {r};
    tile_rollout<ENV, ONE>(lds, tr, K, blockIdx.x * 16, dynp, norm, sink);
}

// -------------------------------------------------------------------------------------------------
typedef void (*ract_kernel_t)(RactK, int, const float*, const float*);
struct RactEntry { int env; ract_kernel_t all, one; int w_sz, nsp; };
#define RENTRY(ENVID) {ENVID, k_rollout_actions<ENVID, false>, k_rollout_actions<ENVID, true>, act_wave_floats<ENVID>(), Cfg<ENVID, 64, 32>::NSP}
static const RactEntry kRact[] = {FUSED_HEAD_ENVS(RENTRY)};

// ---- what the host sides of the fused head kernels share (metrpo_internal.h) ----
bool fused_head_class(const metrpo_ctx* c, int k_cap, bool* padded) {
    const ProblemDesc& pd = c->pd;
    if (pd.K > k_cap) return false;
    if (mfma_shape_config(c) >= 0 && pd.dyn.dims[1] == 64 && pd.dyn.dims[2] == 64) *padded = false;
    else if (c->coop_pad_cfg >= 0) *padded = true;
    else return false;
    return true;
}
int fused_head_dyn(metrpo_ctx* c, bool padded, hipStream_t st, const float** dyn) {
    *dyn = c->d_dyn.p;
    if (padded) { const int rc = launch_pad_dyn(c, st); if (rc) return rc; *dyn = c->d_dyn_pad.p; }
    return METRPO_OK;
}
int allow_dynamic_lds(metrpo_ctx* c, const void* kernel, size_t bytes) {
    if (bytes > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return METRPO_OK;
}

static int launch_rollout_actions_fused(metrpo_ctx* c, const RactEntry& en, bool padded, const metrpo_rollout_actions_args* a, hipStream_t st) {
    const int K = c->pd.K;
    RactK r = {};
    r.B = a->B; r.T = a->T;
    r.init_obs = a->d_init_obs; r.actions = a->d_actions; r.obs = a->d_obs; r.rew = a->d_rew; r.done = a->d_done;
    bool one = false;
    if (a->sam_mode == METRPO_SAM_ONE_MODEL) { one = true; r.head = 0; }                                  // head 0 by definition (env_helpers.py:631-632)
    else if (a->sam_mode == METRPO_SAM_EPS_RAND && a->uniform_model >= 0) { one = true; r.head = a->uniform_model; }
    else if (a->sam_mode == METRPO_SAM_EPS_RAND) { r.mean = 0; r.model = a->d_model; }
    else r.mean = 1;
    const float* dyn;
    { const int rc = fused_head_dyn(c, padded, st, &dyn); if (rc) return rc; }
    const int grid = (a->B + 15) / 16;
    const ract_kernel_t kern = one ? en.one : en.all;
    const int nw = one ? 1 : K;
    const size_t sh = sizeof(float) * ((size_t)nw * en.w_sz + (one ? 0 : head_exchange_floats(K, en.nsp)));
    { const int rc = allow_dynamic_lds(c, (const void*)kern, sh); if (rc) return rc; }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(nw * 64), sh, st, r, K, dyn, c->d_norm.p);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int run_rollout_actions(metrpo_ctx* c, const metrpo_rollout_actions_args* a, hipStream_t st) {
    const int ns = c->pd.ns, na = c->pd.na, B = a->B, T = a->T;
    const int sam = a->sam_mode;
    bool padded = false;
    const RactEntry* en = nullptr;
    if (!a->force_step_loop && (sam == METRPO_SAM_MODEL_MEAN || sam == METRPO_SAM_EPS_RAND || sam == METRPO_SAM_ONE_MODEL)) en = fused_head_entry(kRact, c, 8, &padded);      // a wave per head
    if (en != nullptr) {
        const int rc = launch_rollout_actions_fused(c, *en, padded, a, st);
        if (rc == METRPO_OK) c->last_ract_kernel = 1;
        return rc;
    }
    // ---- step loop: metrpo_step's kernel on row t of d_actions, row t of d_obs -> row t + 1 ----
    const int32_t* model = a->d_model;
    if (sam == METRPO_SAM_EPS_RAND && a->uniform_model >= 0) {
        { const int rc = ws_grow(c, c->d_ract_model, sizeof(int32_t) * (size_t)B); if (rc) return rc; }
        HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->d_ract_model.p, a->uniform_model, (size_t)B, st));
        model = c->d_ract_model.p;
    }
    if (a->d_init_obs != a->d_obs) HIP_TRY(c, hipMemcpyAsync(a->d_obs, a->d_init_obs, sizeof(float) * (size_t)B * ns, hipMemcpyDeviceToDevice, st));
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)t * B;
        const int32_t* idx = (sam == METRPO_SAM_STEP_RAND) ? a->d_model_idx + row : model;
        const float* noise = (sam == METRPO_SAM_MODEL_MEAN_STD) ? a->d_sel_noise + row * ns : nullptr;
        const int rc = launch_step(c, a->d_obs + row * ns, a->d_actions + row * na, B, sam, idx, noise, a->d_obs + (row + B) * ns, a->d_rew + row, a->d_done + row,
                                   nullptr, st);
        if (rc) return rc;
    }
    c->last_ract_kernel = 0;
    return METRPO_OK;
}
