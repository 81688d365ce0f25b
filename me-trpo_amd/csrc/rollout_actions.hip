// metrpo_rollout_actions (include/metrpo.h): the ensemble rolled forward under SUPPLIED actions -- the loop of get_error_distribution(known_actions=True),
// env_helpers.py:216-222, over VecSimpleEnv.step's arithmetic, :597-603.  T chained metrpo_step calls in meaning: no policy, no reset, no path-length
// limit, no draw; stepping continues behind a done.
//
// Fused kernel (k_rollout_actions): rollout_mfma.hip's dynamics step without the policy, the action read from memory instead.
//   * one workgroup = one tile of 16 envs, walked through all T steps, on the shared head of dyn_head_mfma.h (layout and arithmetic are described there).
//   * the head's weight fragments are register-resident for the whole loop (swimmer 92, Ant 132 registers), biases, normalisers' source map and the
//     tile's state live in LDS; the state is [env][ns], the layout of one row of d_obs, so a row is one linear coalesced store.
//   * cost and is_done are device_common.h's env_cost / env_is_done on the LDS rows (the functions metrpo_step's kernel calls).
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
#include "dyn_head_mfma.h"

struct RactK {
    int B, T;
    int mean;                 // ALL: 1 = average the heads (model_mean), 0 = select model[b] (eps_rand)
    int head;                 // ONE: the head
    const float* init_obs; const float* actions; const int32_t* model;
    float* obs; float* rew; uint8_t* done;
};

template <int ENV> constexpr int ract_wave_floats() { return Cfg<ENV, 64, 32>::W_BP0 + al4(16 * Cfg<ENV, 64, 32>::NA); }

template <int ENV, bool ONE>
__global__ void __launch_bounds__(ONE ? 64 : 512) k_rollout_actions(RactK r, int K, const float* __restrict__ dynp, const float* __restrict__ norm) {
    using C = Cfg<ENV, 64, 32>;
    constexpr int NS = C::NS, NA = C::NA, NSP = C::NSP;
    constexpr int W_ACT2 = C::W_BP0, W_SZ = ract_wave_floats<ENV>();   // per-wave LDS (floats): ST | NX | ACT | dynamics biases | second ACT
    constexpr int NLD = cdiv(16 * NA, 64), NST = cdiv(16 * NS, 64);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16, b = b0 + e;
    const bool active = b < r.B;
    const int nrows = min(16, r.B - b0);                      // rows of this tile inside the batch
    const int NW = ONE ? 1 : K;
    float* W = lds + wave * W_SZ;
    float* ST = W + C::W_ST;  float* NX = W + C::W_NX;
    // (clipped actions of even steps at W_ACT, of odd steps at W_ACT2)
    float* NXT = lds + NW * W_SZ;                             // ALL: [2][K][16][NSP] exchange buffer

    // ---------------- one-time: weight fragments -> registers, biases -> LDS ----------------------
    const float* __restrict__ pk = dynp + (size_t)(ONE ? r.head : wave) * C::PD;
    DynHeadFrags<C> head;
    head.load(pk, e, q);
    for (int i = lane; i < C::BD; i += 64) { W[C::W_BD0 + i] = pk[C::db0 + i]; W[C::W_BD1 + i] = pk[C::db1 + i]; }
    for (int i = lane; i < NSP; i += 64) W[C::W_BD2 + i] = (i < NS) ? pk[C::db2 + i] : 0.0f;
    DynInNorm<C> in;
    DynOutNorm<C> out;
    in.load(norm, q);
    out.load(norm, q);

    // ---------------- the tile's initial state and the actions of step 0 ---------------------------
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = lane + 64 * j;
        if (i < 16 * NS) ST[i] = (i < nrows * NS) ? r.init_obs[(size_t)b0 * NS + i] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
        const int i = lane + 64 * j;
        const float a0 = (i < nrows * NA) ? r.actions[(size_t)b0 * NA + i] : 0.0f;
        if (i < 16 * NA) W[C::W_ACT + i] = fminf(fmaxf(a0, -1.0f), 1.0f);            // np.clip(actions, *bounds), env_helpers.py:599 / :216
    }
    int sel = 0;
    if (!ONE && !r.mean && active) sel = min(max(r.model[b], 0), K - 1);
    wave_lds_sync();
    if (wave == 0) {                                                              // row 0 of d_obs = d_init_obs, bit for bit
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < nrows * NS) r.obs[(size_t)b0 * NS + i] = ST[i];
        }
    }
    // every global load above is complete before the step loop (rollout_coop_kernel.h: else the wait for the loop-invariant loads lands inside it)
    __builtin_amdgcn_s_waitcnt(0x0F70);

    for (int t = 0; t < r.T; ++t) {
        // ---- the action block of step t + 1 (the last step reads its own row again: no branch, nothing out of bounds), issued now and read
        //      behind the matrix instructions, IN FRONT of this step's stores ----
        //      Every lane loads (index clamped into the tile's block): a straight-line load the compiler waits for at its use, not in a masked branch.
        float* ACT = W + ((t & 1) ? W_ACT2 : C::W_ACT);
        float* ACTN = W + ((t & 1) ? C::W_ACT : W_ACT2);
        float a_nx[NLD];
        {
            const float* __restrict__ an = r.actions + ((size_t)min(t + 1, r.T - 1) * r.B + b0) * NA;
#pragma unroll
            for (int j = 0; j < NLD; ++j) a_nx[j] = an[min(lane + 64 * j, nrows * NA - 1)];
        }
        // ---- the head: normalise, drop columns, 3 layers (training.py:218-269) ----------------------
        f32x4 h0[C::DH_CB], h1[C::DH_CB], oa[C::OUT_CB], ob[C::OUT_CB];
        float xin[C::NIN_KS];
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) xin[s] = in.get(ST, NS, ACT, e, s);
        head.layer0(h0, W + C::W_BD0, xin, ReluBits());
        head.layer1(h1, W + C::W_BD1, h0, ReluBits());
        head.layer2(oa, ob, W + C::W_BD2, h1);
        f32x4 nx[C::OUT_CB];
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb) {
            f32x4 o = oa[cb] + ob[cb];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                const float sv = (dim < NS) ? ST[e * NS + dim] : 0.0f;
                o[rr] = out.apply(cb, rr, o[rr], sv);
            }
            nx[cb] = o;
        }
        if (!ONE) {
            // ---- get_next_observation (env_helpers.py:617-634): the K heads meet in LDS, every wave selects redundantly ----
            const int par = t & 1;
            float* nxt_w = NXT + ((size_t)(par * K + wave) * 16 + e) * NSP;
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb) *(f32x4*)&nxt_w[16 * cb + 4 * q] = nx[cb];
            __syncthreads();                                                     // all K heads of step t are in NXT[par]
            const float* nxt_all = NXT + (size_t)par * K * 16 * NSP;
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb) {
                const int off = e * NSP + 16 * cb + 4 * q;
                if (!r.mean) {
                    nx[cb] = *(const f32x4*)&nxt_all[(size_t)sel * 16 * NSP + off];
                } else {
                    f32x4 m = {0.f, 0.f, 0.f, 0.f};
                    for (int k = 0; k < K; ++k) m += *(const f32x4*)&nxt_all[(size_t)k * 16 * NSP + off];    // head order, as metrpo_step
                    nx[cb] = m / (float)K;
                }
            }
        }
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) NX[e * NS + dim] = nx[cb][rr];
            }
        // ---- the prefetched actions become step t + 1's.  The wait for them is the loop's only vmcnt wait; the vector-memory counter is in order, so
        //      it also covers the stores of step t - 1 -- a whole step old by now -- and none of step t's, which follow below ----
        //      (the empty statement takes the loaded values on EVERY path: were they read only inside the masked write below, the load could
        //      still be in flight at the loop's back edge and the compiler would wait for it -- and the stores -- at the top of the next step)
#pragma unroll
        for (int j = 0; j < NLD; ++j) asm volatile("" ::"v"(a_nx[j]));
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NA) ACTN[i] = (i < nrows * NA) ? fminf(fmaxf(a_nx[j], -1.0f), 1.0f) : 0.0f;
        }
        wave_lds_sync();
        // ---- reward = -cost_np_vec(s, a_clipped, s') (:601) and is_done(s', s') (:603); the env goes on either way ----
        const float cost = env_cost(ENV, NS, NA, NX + e * NS, ACT + e * NA, 1, 0);
        const bool dn = env_is_done(ENV, NS, NX + e * NS, 1, 0);
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NS) ST[i] = NX[i];
        }
        wave_lds_sync();
        if (wave == 0) {
            float* __restrict__ orow = r.obs + ((size_t)(t + 1) * r.B + b0) * NS;
#pragma unroll
            for (int j = 0; j < NST; ++j) {
                const int i = lane + 64 * j;
                if (i < nrows * NS) orow[i] = ST[i];
            }
            if (q == 0 && active) { const size_t tb = (size_t)t * r.B + b; r.rew[tb] = -cost; r.done[tb] = dn ? 1 : 0; }
        }
    }
}

// -------------------------------------------------------------------------------------------------
typedef void (*ract_kernel_t)(RactK, int, const float*, const float*);
struct RactEntry { int env; ract_kernel_t all, one; int w_sz, nsp; };
#define RENTRY(ENVID) {ENVID, k_rollout_actions<ENVID, false>, k_rollout_actions<ENVID, true>, ract_wave_floats<ENVID>(), Cfg<ENVID, 64, 32>::NSP}
static const RactEntry kRact[] = {RENTRY(METRPO_ENV_SWIMMER), RENTRY(METRPO_ENV_HALF_CHEETAH), RENTRY(METRPO_ENV_HOPPER), RENTRY(METRPO_ENV_SNAKE), RENTRY(METRPO_ENV_ANT)};

// the fused kernel holds this context's shape: the fused rollout kernels' shape class with two hidden layers of 64 (*padded = false), or narrower ones
// through the zero-padded copy d_dyn_pad that metrpo_create made for them (*padded = true); K <= 8 (a wave per head)
static const RactEntry* ract_entry(const metrpo_ctx* c, bool* padded) {
    const ProblemDesc& pd = c->pd;
    if (pd.K > 8) return nullptr;
    if (mfma_shape_config(c) >= 0 && pd.dyn.dims[1] == 64 && pd.dyn.dims[2] == 64) *padded = false;
    else if (c->coop_pad_cfg >= 0) *padded = true;
    else return nullptr;
    for (const RactEntry& en : kRact)
        if (en.env == pd.env) return &en;
    return nullptr;
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
    const float* dyn = c->d_dyn.p;
    if (padded) { const int rc = launch_pad_dyn(c, st); if (rc) return rc; dyn = c->d_dyn_pad.p; }
    const int grid = (a->B + 15) / 16;
    const ract_kernel_t kern = one ? en.one : en.all;
    const int nw = one ? 1 : K;
    const size_t sh = sizeof(float) * ((size_t)nw * en.w_sz + (one ? 0 : 2 * (size_t)K * 16 * en.nsp));
    if (sh > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(nw * 64), sh, st, r, K, dyn, c->d_norm.p);
    HIP_TRY(c, hipGetLastError());
    return METRPO_OK;
}

int run_rollout_actions(metrpo_ctx* c, const metrpo_rollout_actions_args* a, hipStream_t st) {
    const int ns = c->pd.ns, na = c->pd.na, B = a->B, T = a->T;
    const int sam = a->sam_mode;
    bool padded = false;
    const RactEntry* en = nullptr;
    if (!a->force_step_loop && (sam == METRPO_SAM_MODEL_MEAN || sam == METRPO_SAM_EPS_RAND || sam == METRPO_SAM_ONE_MODEL)) en = ract_entry(c, &padded);
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
