#pragma once
// Cooperative-heads MFMA rollout (second generation of rollout_mfma.hip; same arithmetic, same reference
// sites: samplers/vectorized_sampler.py:45-116, env_helpers.py:597-635, training.py:218-269).
//
// Why: with one head per wave (rollout_mfma.hip) a K=5 workgroup has 5 waves on 4 SIMDs, one SIMD carries two
// heads (2 x 92 MFMAs per step) and, at ~230 VGPRs, only ONE such workgroup fits a CU -- the 313 tiles of the
// headline shape (B = 5000) then run in two sequential rounds on 256 CUs (measured: B=4096 0.64 ms, B=5000 1.23 ms).
// Here a workgroup is exactly 4 waves (one per SIMD) for a 16-env tile and EVERY head is split across them:
//     wave w owns hidden col-block w (16 of the 64 units) of layers 0 and 1 of all K heads, and the K-slice w of
//     layer 2 (its own 16 hidden units), i.e. K x (3 + 16 + 4) = 115 MFMAs per step instead of 92 / 184,
// balanced over the 4 SIMDs, and two workgroups fit a CU (8 waves, 2 per SIMD).  Costs: the layer-0 activations and the layer-2
// partial sums cross waves through LDS -> three barriers per step (action, layer-0 activations, layer-2 partials).
// Round 2: the policy (32 MFMAs, 16 tanh per lane) runs on wave 0 only; waves 1-3 meanwhile run the state-only k-steps of layer 0
// (their own col-block and wave 0's) and wave 1 the next step's Philox draws; launches with up to 1.55 tiles per CU run ONE workgroup
// per CU with the tile-steps dealt out evenly and tiles migrating between workgroups (see the kernel and launch_rollout_coop);
// this file is compiled with -amdgpu-mfma-vgpr-form (Makefile) so that MFMA results stay in the vector half of the register file.
// Head-split form (k_rollout_coop_split): launches with one workgroup per CU of the envs with one output col-block at K = 2 ... 5 run 8 waves on
// the tile, two per SIMD, each SIMD's pair sharing a col-block and splitting the heads -- the same units in the same order, bit for bit (metrpo_set_coop_split(ctx, 0): 4 waves).
// Both forms are ONE body, rollout_coop_body.h: every phase of the tile-step is written once, and a role block at its top holds what the forms disagree on.
#include "dyn_head_mfma.h"

// Developer instrumentation (tools/build_variant.sh timing -DCOOP_TIMING=0xFFF): per-phase shader-clock sums of the four waves of
// workgroup 0, read back with metrpo_debug_coop_phases (tools/coop_phases.py).  Not part of the shipped library.
#if defined(COOP_TIMING) && defined(COOP_MAIN_TU)
// s_memtime (the SHADER_CYCLES hardware register reads 0 on gfx950); all four waves of workgroup 0.  Every mark also drains the wave's
// LDS queue (s_memtime returns through lgkmcnt), so phases that overlap LDS latency with later work look longer than they are.
__device__ unsigned long long g_coop_phase[8][16];                       // [wave][phase]; rows 4-7: the second head group of the head-split form
#define PH_NOW() __builtin_readcyclecounter()
#define PH_DECL unsigned long long ph_t = PH_NOW(); unsigned long long ph_acc[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PH_MARK(i) { if ((COOP_TIMING >> (i)) & 1) { const unsigned long long n_ = PH_NOW(); ph_acc[i] += n_ - ph_t; ph_t = n_; } }   // -DCOOP_TIMING=<bit mask of live marks>
#define PH_DUMP { if (lane == 0 && blockIdx.x == 0) for (int i_ = 0; i_ < 14; ++i_) g_coop_phase[wave][i_] = ph_acc[i_]; }
extern "C" int32_t metrpo_debug_coop_phases(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_coop_phase), sizeof(unsigned long long) * 128) == hipSuccess ? 0 : -1; }
#else
#define PH_DECL
#define PH_MARK(i)
#define PH_DUMP
#endif

#ifndef COOP_SKIP
#define COOP_SKIP 0        // developer experiments (tools/build_variant.sh): bit mask of step parts to leave out; results are then meaningless
#endif
template <int ENV, int K, int NWV = 4>                                  // NWV: waves of the workgroup (8: the head-split form below)
struct Coop {
    using C = Cfg<ENV, 64, 32>;
    static constexpr int NS = C::NS, NA = C::NA, NSP = C::NSP;
    static constexpr int P0KS = 4 * C::OUT_CB;                        // policy layer-0 k-steps (cb_in, rr): input dim 16 cb_in + 4 q + rr, the D layout of the state
    static constexpr int NPF = P0KS * 2 + 16 + 8;                     // policy weight fragments: wp0[P0KS][2], wp1[8][2], wp2[8]
    // LDS map (floats)
    static constexpr int WV = ((16 * NSP + 16 * NS + 16 * NA + 3) / 4) * 4;   // per wave: ST (rows padded to NSP: one unpredicated 16-byte access per lane) | NX | ACT
    static constexpr int O_BD0 = NWV * WV, O_BD1 = O_BD0 + K * 64, O_BD2 = O_BD1 + K * 64, O_BP0 = O_BD2 + K * NSP,
                         O_BP1 = O_BP0 + 32, O_BP2 = O_BP1 + 32, O_PW = O_BP2 + 16, O_H0 = O_PW + NPF * 64,
                         O_PART = O_H0 + K * 1024, O_RNG = O_PART + K * 4 * 16 * NSP, O_WX = O_RNG + 2 * 16 * 20,
                         O_AK = O_WX + 3 * ((K + 2) / 3) * C::NIN_KS * 64, TOTAL = O_AK + 2 * 16 * NA;   // O_AK: unclipped action | mean of the step          // O_WX: col-block-0 layer-0 fragments of the helper waves (two-tile kernel)
};

// ONE: instantiation for launches with at most one tile per CU -- the whole register file (512 lanes-wide registers per SIMD) belongs to
// one workgroup, so the half-cheetah / Ant weight fragments (150 VGPRs) stop spilling to scratch.
// DRAWS: instantiation for launches that SUPPLY draws (eps / model_idx / sel_noise / reset_idx / reset_model: the parity tests).  The
// production instantiation (Philox draws) has no global load in the step loop outside the rare reset branch, hence no s_waitcnt
// vmcnt in it: a vmcnt wait also waits for the step's stores, whose acknowledge latency then lands on the critical path.
//
// Head-split form (G = 0 / 1) of the one-workgroup-per-CU kernel: 8 waves, two per SIMD, on ONE tile (envs with one output col-block, K = 2 ... 5).
// Why: at one wave per SIMD a tile-step is a latency chain (three barriers, the LDS round trips of H0 / PART / ACT, the ReLU and tanh
// stretches, selection, the policy) that leaves the matrix pipe idle half of the time, and a launch with about one tile per CU cannot
// fill the gaps with a second, co-resident tile.  Here the second wave of every SIMD comes from the SAME tile: wave 4 g + w sits on SIMD w
// and owns hidden col-block w of the heads of group g only --
//     group 0 (waves 0-3): heads 0 .. K/2 - 1          (the lighter one: 2 of 5 heads)
//     group 1 (waves 4-7): heads K/2 .. K - 1
// Every (head, col-block) unit keeps the instruction order, the H0 / PART slots (indexed by col-block) and the four-term partial sum of
// the 4-wave form, so the results are that form's bit for bit; only the wave that executes a unit changes.  The group is a template
// argument of the body (a wave-uniform branch in k_rollout_coop_split picks it), so the weight fragments stay register arrays sized by the group.
// Singleton jobs stay with the waves of the lighter group: wave 0 the policy and the obs / action / mean stores (no layer 0),
// wave 1 the next step's Philox block, wave 2 the reward / done / tpath stores (group 0 evaluates the reward, group 1 does not).  Layer 0 of col-block 0
// has a natural owner, wave 4: it runs it for its own heads and for the heads of group 0 (wave 0 is busy with the policy) -- the
// help waves 1-3 give in the 4-wave form.  Barriers (B0, B1, B2), the migration hand-over and the launch shape are the same; every
// wave keeps its own copy of the tile state and evaluates the selection for itself.
// Measured (profiles/r16_coop_split.txt; swimmer K = 5): tile-step 8910 -> 8405 cycles, kernel 0.428 -> 0.417 ms at B = 5000, 0.350 -> 0.340 ms at B = 4096.  The
// B1 -> B2 phase (layers 1 and 2) went from ~4250 to ~3650 cycles and is now the matrix pipe's own time (the pair of a SIMD shares it: 100 instructions x 32
// cycles), layer 0 from ~900 to ~680; the ~2400 cycles every wave waits for wave 0's policy chain before B0 are unchanged -- no wave of the same tile has work
// that does not need the action.  224 / 242 registers (Philox / supplied draws), no vector spill; K = 4 spills up to 48 and is still 2.7 % faster than 4 waves.
//
// One body for both forms, rollout_coop_body.h, included as text into each entry: G = -1, the four waves own all K heads (k_rollout_coop); G = 0 / 1,
// a head group of the 8-wave form (coop_split_group, ONE).  What the forms disagree on is the role block at the top of the body.
template <int ENV, int K, bool ONE, bool DRAWS>
__global__ void __launch_bounds__(256, ONE ? 1 : 2) k_rollout_coop(RolloutK r, const float* __restrict__ dynp,
                                                      const float* __restrict__ theta, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int G = -1;
    const int w = (int)threadIdx.x >> 6;
#define COOP_SPLIT_FORM 0
#include "rollout_coop_body.h"
#undef COOP_SPLIT_FORM
}
template <int ENV, int K, bool DRAWS, int G>
__device__ __forceinline__ void coop_split_group(const RolloutK& r, const float* __restrict__ dynp, const float* __restrict__ theta,
                                                 const float* __restrict__ norm, float* lds, const int w) {
    constexpr bool ONE = true;
#define COOP_SPLIT_FORM 1
#include "rollout_coop_body.h"
#undef COOP_SPLIT_FORM
}
template <int ENV, int K, bool DRAWS>
__global__ void __launch_bounds__(512, 1) k_rollout_coop_split(RolloutK r, const float* __restrict__ dynp,
                                                                const float* __restrict__ theta, const float* __restrict__ norm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));          // wave-uniform: scalar branch, both groups keep the barrier count
    if (wave < 4) coop_split_group<ENV, K, DRAWS, 0>(r, dynp, theta, norm, lds, wave);
    else coop_split_group<ENV, K, DRAWS, 1>(r, dynp, theta, norm, lds, wave - 4);
}

// -------------------------------------------------------------------------------------------------
typedef void (*coop_kernel_t)(RolloutK, const float*, const float*, const float*);
template <int ENV> static constexpr bool coop_two_per_cu_spills() { return EnvDim<ENV>::NS > 16; }   // see the launch rule in rollout_coop.hip
// kern[one workgroup per CU][draws supplied]; kern[0][*] == nullptr: the shape only has the one-workgroup-per-CU instantiation (K > 5)
struct CoopEntry { int env, K; coop_kernel_t kern[2][2]; int lds_floats; bool always_one; double pair, rem_slope; };
#define CENTRY(ENVID, KK) {ENVID, KK, {{k_rollout_coop<ENVID, KK, false, false>, k_rollout_coop<ENVID, KK, false, true>}, \
                                       {k_rollout_coop<ENVID, KK, true, false>, k_rollout_coop<ENVID, KK, true, true>}}, Coop<ENVID, KK>::TOTAL, coop_two_per_cu_spills<ENVID>(), \
                                       (ENVID == METRPO_ENV_SWIMMER) ? 1.50 : (ENVID == METRPO_ENV_SNAKE) ? 1.58 : 1.65, (ENVID == METRPO_ENV_SWIMMER) ? 0.0 : 1.0}
// K = 6 ... 10 heads (round 6): K x 23 weight fragments per wave need the WHOLE register file of a SIMD (512 registers: one workgroup per CU) -- only that instantiation
// exists; each K is a translation unit of its own (rollout_coop_k<K>.hip: these kernels compile for ~30 s apiece)
// (the LDS map grows with K x padded state width: Ant holds 8 heads in a CU's 160 KB, half-cheetah 9, the 16-dim envs 10 -- larger K: no kernel, nullptr)
template <int ENV, int K, bool DRAWS> constexpr coop_kernel_t coop_one_kernel() {
    if constexpr (Coop<ENV, K>::TOTAL * sizeof(float) <= 160 * 1024) return k_rollout_coop<ENV, K, true, DRAWS>; else return nullptr;
}
#define CENTRY_ONE(ENVID, KK) {ENVID, KK, {{nullptr, nullptr}, {coop_one_kernel<ENVID, KK, false>(), coop_one_kernel<ENVID, KK, true>()}}, Coop<ENVID, KK>::TOTAL, true, 0.0, 0.0}
#define COOP_WIDE_TABLE(NAME, KK) extern const CoopEntry NAME[5]; const CoopEntry NAME[5] = { CENTRY_ONE(METRPO_ENV_SWIMMER, KK), CENTRY_ONE(METRPO_ENV_HALF_CHEETAH, KK), \
    CENTRY_ONE(METRPO_ENV_HOPPER, KK), CENTRY_ONE(METRPO_ENV_SNAKE, KK), CENTRY_ONE(METRPO_ENV_ANT, KK) };

// kern[draws supplied] of the head-split form, or nullptr outside its scope (launch_rollout_coop)
struct CoopSplitEntry { int env, K; coop_kernel_t kern[2]; int lds_floats; };
#define CSPLIT(ENVID, KK) {ENVID, KK, {k_rollout_coop_split<ENVID, KK, false>, k_rollout_coop_split<ENVID, KK, true>}, Coop<ENVID, KK, 8>::TOTAL}
#define CSPLIT_ENV(ENVID) CSPLIT(ENVID, 5), CSPLIT(ENVID, 4), CSPLIT(ENVID, 3), CSPLIT(ENVID, 2)
