// One step of one dynamics head on a tile of 16 rows under SUPPLIED actions, and what the fused kernels around it share: the one statement of what
// rollout_actions.hip (k_rollout_actions), score_actions.hip (k_score_actions) and disagreement.hip (k_disagreement) run on dyn_head_mfma.h.
//   DynWaveHead     a wave's head: weight fragments and both normalisers in registers, its three bias rows in LDS; step() = s' of the tile in D layout
//   ActTile         the tile's action block, double-buffered in LDS: the next step's rows are loaded at the top of a step and committed behind it
//   HeadExchange    the K heads' next states meeting in LDS (a wave per head), and their mean in head order
//   tile_rollout    T chained steps of one tile with a sink for the results: the body of k_rollout_actions (either form) and of k_score_actions
// No LDS is declared here: every pointer into it is the caller's.  Lane l = (e = l & 15, q = l >> 4) as in dyn_head_mfma.h.
#pragma once
#include "dyn_head_mfma.h"

// per-wave LDS (floats) of tile_rollout: ST | NX | ACT | dynamics biases | second ACT (Cfg<>'s W_* offsets; the policy's bias rows are not needed)
template <int ENV> constexpr int act_wave_floats() { return Cfg<ENV, 64, 32>::W_BP0 + al4(16 * Cfg<ENV, 64, 32>::NA); }
// the K-head exchange area (floats): [2][K][16][NSP]
constexpr size_t head_exchange_floats(int K, int nsp) { return 2 * (size_t)K * 16 * nsp; }

// every global load issued so far is complete: placed in front of a step or tile loop (rollout_coop_kernel.h: else the wait for the loop-invariant
// loads -- fragments, biases, normalisers -- lands inside the loop)
__device__ __forceinline__ void loop_invariant_loads_done() { __builtin_amdgcn_s_waitcnt(0x0F70); }

template <class C>
struct DynWaveHead {
    DynHeadFrags<C> frags;
    DynInNorm<C> in;
    DynOutNorm<C> out;
    const float *bd0, *bd1, *bd2;                // the wave's own LDS rows: [BD] [BD] [NSP]
    int q;

    // pk: the head's parameters (Cfg<>'s layout), norm: d_norm; bias rows -> LDS (padded dims of the output bias zero)
    __device__ __forceinline__ void load(const float* __restrict__ pk, const float* __restrict__ norm, float* bd0_, float* bd1_, float* bd2_, int lane) {
        q = lane >> 4;
        frags.load(pk, lane & 15, q);
        for (int i = lane; i < C::BD; i += 64) { bd0_[i] = pk[C::db0 + i]; bd1_[i] = pk[C::db1 + i]; }
        for (int i = lane; i < C::NSP; i += 64) bd2_[i] = (i < C::NS) ? pk[C::db2 + i] : 0.0f;
        in.load(norm, q);
        out.load(norm, q);
        bd0 = bd0_; bd1 = bd1_; bd2 = bd2_;
    }
    // nx = the de-normalised next state of env e from LDS state rows (st_stride floats apart) and clipped action rows: normalise, drop columns, 3 layers
    // (training.py:218-269), diff_mean + diff_std * out + s (:257).  Register [cb][r] is state dim 16 cb + 4 q + r, zero on the padded dims.
    __device__ __forceinline__ void step(f32x4 (&nx)[C::OUT_CB], const float* ST, int st_stride, const float* ACT, int e) const {
        f32x4 h0[C::DH_CB], h1[C::DH_CB], oa[C::OUT_CB], ob[C::OUT_CB];
        float xin[C::NIN_KS];
#pragma unroll
        for (int s = 0; s < C::NIN_KS; ++s) xin[s] = in.get(ST, st_stride, ACT, e, s);
        frags.layer0(h0, bd0, xin, ReluBits());
        frags.layer1(h1, bd1, h0, ReluBits());
        frags.layer2(oa, ob, bd2, h1);
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb) {
            f32x4 o = oa[cb] + ob[cb];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                const float sv = (dim < C::NS) ? ST[e * st_stride + dim] : 0.0f;
                o[rr] = out.apply(cb, rr, o[rr], sv);
            }
            nx[cb] = o;
        }
    }
};

// The action block of a tile ([16][NA] of d_actions [T][B][na] at rows b0 ..), clipped (np.clip(actions, *bounds), env_helpers.py:599 / :216), in two
// LDS buffers: step t reads cur(t), the block of step t + 1 goes into the other one.  Rows at and beyond nrows (B % 16 != 0) are zero actions and are
// never read from memory.  The loop's only global load: <= 2 floats per lane.
template <class C>
struct ActTile {
    static constexpr int NA = C::NA, NLD = cdiv(16 * NA, 64);
    const float* actions;
    // the wave's LDS; the two buffers are at W + off0, W + off1.  Offsets, not two pointers: W depends on the wave and so lives in a vector register,
    // and a select between two such pointers keeps both alive over the step (k_rollout_actions<swimmer, false>: 172 registers instead of 166, which
    // is 2 waves per SIMD instead of 3); a select between two constants is scalar.
    float* W;
    int off0, off1;
    int B, T, b0, nact, lane;                    // nact = nrows * NA: floats of the block inside the batch
    float a_nx[NLD];

    __device__ __forceinline__ void init(const float* actions_, int B_, int T_, int b0_, int nrows, int lane_, float* W_, int off0_, int off1_) {
        actions = actions_; B = B_; T = T_; b0 = b0_; nact = nrows * NA; lane = lane_; W = W_; off0 = off0_; off1 = off1_;
    }
    __device__ __forceinline__ float* cur(int t) const { return W + ((t & 1) ? off1 : off0); }
    // issue the loads of step t's block (behind the last step: the last step's own block again -- no branch, nothing out of bounds).  Every lane
    // loads, the index clamped into the tile's block: a straight-line load the compiler waits for at its use, not in a masked branch.
    __device__ __forceinline__ void prefetch(int t) {
        const float* __restrict__ an = actions + ((size_t)min(t, T - 1) * B + b0) * NA;
#pragma unroll
        for (int j = 0; j < NLD; ++j) a_nx[j] = an[min(lane + 64 * j, nact - 1)];
    }
    // the loaded block becomes cur(t).  Inside a step loop this is the loop's only vmcnt wait, and the caller places it behind the step's matrix
    // instructions and IN FRONT of the step's stores: the vector-memory counter is in order, so the wait also covers every older store -- those of
    // the step before, a whole step of matrix work old -- and none of this step's.
    // The empty statement takes the loaded values on EVERY path: were they read only inside the masked write below, the load could still be in
    // flight at the loop's back edge and the compiler would wait for it -- and the stores -- at the top of the next step.
    __device__ __forceinline__ void commit(int t) {
        float* dst = cur(t);
#pragma unroll
        for (int j = 0; j < NLD; ++j) asm volatile("" ::"v"(a_nx[j]));
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NA) dst[i] = (i < nact) ? fminf(fmaxf(a_nx[j], -1.0f), 1.0f) : 0.0f;
        }
    }
};

// get_next_observation's meeting of the heads (env_helpers.py:617-634): wave k writes its head's nx into NXT[par][k] (par: the double buffer), ONE
// barrier of the caller's, then every wave reads what it needs.  off = e * NSP + 16 cb + 4 q addresses lane (e, q)'s registers of block cb.
template <class C>
struct HeadExchange {
    static constexpr int NSP = C::NSP;
    float* NXT;                                  // [2][K][16][NSP]
    int K;

    __device__ __forceinline__ void put(int par, int wave, int e, int q, const f32x4 (&nx)[C::OUT_CB]) const {
        float* nxt_w = NXT + ((size_t)(par * K + wave) * 16 + e) * NSP;
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb) *(f32x4*)&nxt_w[16 * cb + 4 * q] = nx[cb];
    }
    __device__ __forceinline__ const float* heads(int par) const { return NXT + (size_t)par * K * 16 * NSP; }
    static __device__ __forceinline__ f32x4 head(const float* all, int k, int off) { return *(const f32x4*)&all[(size_t)k * 16 * NSP + off]; }
    // the mean over the heads: summed in head order k = 0 .. K-1, divided by K, as metrpo_step
    static __device__ __forceinline__ f32x4 mean(const float* all, int K, int off) {
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < K; ++k) m += head(all, k, off);
        return m / (float)K;
    }
};

// What tile_rollout needs to know of a launch.  ONE head: `head`; ALL heads (a wave per head, K <= 8): mean = 1 averages them, 0 selects model[b].
struct TileRollK {
    int B, T, per;                               // candidate b starts from init_obs[b / per]
    const float* init_obs; const float* actions;
    int head, mean; const int32_t* model;
};

// One tile of 16 envs (rows b0 .. of the batch) walked through all T steps under the supplied actions: VecSimpleEnv.step's arithmetic (env_helpers.py:597-603)
// chained, no policy, no reset, no draw; stepping continues behind a done.  lds: NW waves' act_wave_floats, then (ALL) head_exchange_floats.
//   ONE: one wave, one head, every activation in registers, no barrier.  ALL: wave k owns head k, one barrier per step, every wave selects or averages
//   redundantly and keeps the tile's state in its own LDS.
// Sink (called by wave 0 only): start(ST, b0, nrows, lane) with the start rows in LDS; step(t, ST, cost, done, b0, nrows, lane) behind step t with
//   s' in ST [env][NS] -- the layout of one row of d_obs -- and this lane's env's cost_np_vec(s, a_clipped, s') (:601) and is_done(s', s') (:603).
template <int ENV, bool ONE, class Sink>
__device__ __forceinline__ void tile_rollout(float* lds, const TileRollK& r, int K, int b0, const float* __restrict__ dynp, const float* __restrict__ norm, Sink& sink) {
    using C = Cfg<ENV, 64, 32>;
    constexpr int NS = C::NS, NA = C::NA, NSP = C::NSP, NST = cdiv(16 * NS, 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = ONE ? 0 : tid >> 6;
    const int e = lane & 15, q = lane >> 4;
    const int b = b0 + e;
    const int nrows = min(16, r.B - b0);                      // rows of this tile inside the batch
    float* W = lds + wave * act_wave_floats<ENV>();
    float* ST = W + C::W_ST;  float* NX = W + C::W_NX;
    const HeadExchange<C> xch = {lds + (ONE ? 1 : K) * act_wave_floats<ENV>(), K};

    DynWaveHead<C> head;
    head.load(dynp + (size_t)(ONE ? r.head : wave) * C::PD, norm, W + C::W_BD0, W + C::W_BD1, W + C::W_BD2, lane);
    // ---------------- the tile's start rows (gathered per row: a tile may straddle two start states) and the actions of step 0 -----------
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = lane + 64 * j;
        const int row = i / NS, col = i - row * NS;
        if (i < 16 * NS) ST[i] = (row < nrows) ? r.init_obs[(size_t)((b0 + row) / r.per) * NS + col] : 0.0f;
    }
    ActTile<C> act;
    act.init(r.actions, r.B, r.T, b0, nrows, lane, W, C::W_ACT, C::W_BP0);
    act.prefetch(0);
    act.commit(0);
    int sel = 0;
    if (!ONE && !r.mean && b < r.B) sel = min(max(r.model[b], 0), K - 1);
    wave_lds_sync();
    if (wave == 0) sink.start(ST, b0, nrows, lane);
    loop_invariant_loads_done();

    for (int t = 0; t < r.T; ++t) {
        const float* ACT = act.cur(t);
        act.prefetch(t + 1);                                                     // committed behind the matrix instructions, in front of the sink's stores
        f32x4 nx[C::OUT_CB];
        head.step(nx, ST, NS, ACT, e);
        if (!ONE) {                                                              // every wave selects or averages redundantly
            xch.put(t & 1, wave, e, q, nx);
            __syncthreads();                                                     // all K heads of step t are in NXT[t & 1]
            const float* all = xch.heads(t & 1);
#pragma unroll
            for (int cb = 0; cb < C::OUT_CB; ++cb) {
                const int off = e * NSP + 16 * cb + 4 * q;
                nx[cb] = r.mean ? xch.mean(all, K, off) : xch.head(all, sel, off);
            }
        }
#pragma unroll
        for (int cb = 0; cb < C::OUT_CB; ++cb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int dim = 16 * cb + 4 * q + rr;
                if (dim < NS) NX[e * NS + dim] = nx[cb][rr];
            }
        act.commit(t + 1);                                                       // the loop's only vmcnt wait
        wave_lds_sync();
        const float cost = env_cost(ENV, NS, NA, EnvVec{NX + e * NS, 1}, EnvVec{ACT + e * NA, 1});
        const bool dn = env_done_scan(ENV, NS, EnvVec{NX + e * NS, 1});
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int i = lane + 64 * j;
            if (i < 16 * NS) ST[i] = NX[i];
        }
        wave_lds_sync();
        if (wave == 0) sink.step(t, ST, cost, dn, b0, nrows, lane);
    }
}
