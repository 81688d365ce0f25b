// Internal definitions shared by the HIP translation units of libmetrpo.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>
#include "metrpo.h"
#include "xchg_device.h"

#define MAXL (METRPO_MAX_LAYERS + 1)   // weight layers per MLP (hidden + output)
#define WAVE 64

// One MLP as offsets into a flat float vector: [W0 (n_in x n_out row-major), b0, W1, b1, ...].
struct NetDesc {
    int n_layers;            // weight layers
    int dims[MAXL + 1];      // dims[0] = inputs ... dims[n_layers] = outputs
    int act[MAXL];           // metrpo_act applied after layer l (last: identity)
    int w_off[MAXL];         // offsets in the DEVICE-RESIDENT layout.  Dynamics: every W/b array and every model starts on a
    int b_off[MAXL];         // 16-byte boundary (pads are zero) so the GEMM/MFMA kernels can use float4 loads for all heads;
    int n_params;            // policy: identical to the API layout.  n_params = floats of one network (policy: WITHOUT log_std)
    int api_w_off[MAXL];     // offsets in the dense caller-visible layout of include/metrpo.h
    int api_b_off[MAXL];
    int api_n_params;
    int max_width;           // max over dims
};

// Normaliser block layout in ctx->d_norm: in_mean[ns+na] | in_std[ns+na] | diff_mean[ns] | diff_std[ns]
struct ProblemDesc {
    int env, ns, na, K, n_drop, nin;   // nin = ns + na - n_drop
    NetDesc dyn, pol;
    int P;                             // policy params incl. log_std
};

#define METRPO_MAX_PAR_ROUNDS 8
// ---- variant / tuning switches of a context (metrpo_set_option / metrpo_get_option, include/metrpo.h) ----------------------------------------------
// One table per context, read by the launch paths through ctx_opt(); metrpo_create fills the defaults ONCE from the environment (METRPO_<KEY>), nothing
// else in the library reads the environment for kernel selection.  A key is the upper-case name below (the ABI also takes lower case and a METRPO_ prefix).
#define METRPO_OPT_LIST(X) X(NO_FUSED_OUT) X(NO_L0_ROWS) X(NO_MERGED_ROUNDS) X(NO_RESIDENT) X(NO_RESIDENT_VALIDATION) X(NO_STREAMK) X(PRE_GEMM) X(RESIDENT_PLAN) X(RESIDENT_TEST_SKIP) X(RESIDENT_WS) X(SEQ_ROUNDS) X(STEP_MERGE) X(STREAMK) X(STREAMK_LATE) X(STREAMK_PLACE) X(VAL_PLAN) X(XCHG_TIMEOUT_MS) X(NO_PERSIST) X(QUIET) X(TIME_FVP) X(PERSIST_STATS) X(PERSIST_WIDE) X(PERSIST_NCLOSE) X(NO_POL_FUSED3) X(NO_PRE_SPLIT)
enum MetrpoOpt {
#define X(n) OPT_##n,
    METRPO_OPT_LIST(X)
#undef X
    OPT_COUNT
};

// One device allocation owned by a context: freed (hipFree) when the context is deleted, bytes = its size (0: none).  Not copyable -- a copy
// would be a second owner, and a kernel argument taken by value would be the wrapper rather than the pointer -- and deliberately without
// a conversion to T*: every use names .p.  Grown only by ws_grow below.
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct metrpo_ctx {
    int device = 0;
    metrpo_dims dims = {};
    ProblemDesc pd = {};
    DevBuf<float> d_dyn;     // [K][dyn.n_params]
    DevBuf<float> d_norm;    // 2*(ns+na) + 2*ns
    DevBuf<float> d_theta;   // [P]
    bool have_dyn = false, have_pol = false;
    // --- MFMA fast path: pre-permuted weight images, built by set_* ---
    DevBuf<float> d_pol_img; // (int32 payload) gather map of the policy weight-fragment image, see policy_mfma.hip
    int pol_img_idx = -1;    // table index the map was built for (-1: none)
    // image VALUES of one CG solve (policy_mfma.hip): [weight entries of theta, written by the gradient kernel's block 0 | tangent entries of the
    // current CG vector, written by the fused CG tails through d_pol_vpos (theta index -> image position, -1: none)].  SolveScope::publish_image is
    // raised by run_trpo_update while both writers are on the launch sequence; the cached-activation FVP then copies the image instead of gathering it.
    DevBuf<float> d_pol_imgval; DevBuf<int> d_pol_vpos;
    // --- BPTT (bptt.hip) ---
    DevBuf<void> d_bptt;                      // XS | WT | GM | gout | costs
    DevBuf<void> d_pol_adam; int pol_adam_t = 0;   // Adam moments of the policy parameters + segment table
    int det_cfg = -1;                         // bptt_mfma.hip table index (-1: generic sweeps / generic validation kernel)
    DevBuf<double> d_detpart;                 // per-tile cost partials of the MFMA forward sweep
    int det_gemm = 0;                         // 1: GEMM-path sweeps (det_gemm.hip) for large dynamics nets
    DevBuf<void> d_dg;                        // workspace of the GEMM-path sweeps
    int mfma_cfg = -1;       // index into the instantiation table, -1 = generic path only
    int pol_mfma = -1;       // index into policy_mfma.hip's table, -1 = generic update kernels
    int coop_cfg = -1;       // index into rollout_coop.hip's table, -1 = head-per-wave kernel (rollout_mfma.hip)
    // two hidden layers of at most 64 units each, not both 64 (round 6): the cooperative kernel on a zero-padded copy of the weights in the 64 x 64 layout (padded units: zero weights and
    // bias -> relu(0) = 0 -> they add exact zeros); the copy is rebuilt from d_dyn in front of every rollout launch (one small kernel: no tracking of who wrote d_dyn)
    int coop_pad_cfg = -1; DevBuf<float> d_dyn_pad; NetDesc dyn_pad = {};
    int det_padded = 0;      // the validation-cost / BPTT sweeps of bptt_mfma.hip run on the same padded copy
    int rollout_variant = 0; // test hook: 0 = fastest available, 1 = head-per-wave MFMA kernel
    // --- workspaces for the update path (lazily sized) ---
    DevBuf<float> d_partials;      // [n_blocks][P+2] per-block partial sums
    DevBuf<double> d_cg;           // CG vectors + scalars, see trpo_update.hip
    DevBuf<float> d_vf;            // [P] float copy of the FVP input
    DevBuf<float> d_theta_try;     // [P] line-search candidate
    DevBuf<double> d_valbuf;       // validation-cost accumulators
    DevBuf<double> d_vbuf;         // [N] baseline predictions for the GAE scan
    DevBuf<double> d_gae_part;     // k_gae: arrival ticket + one (sum adv, sum adv^2, count) triple per workgroup, added in workgroup order
    DevBuf<double> d_gram_part;    // per-block Gram partials (process.hip)
    DevBuf<unsigned int> d_ticket; // arrival counter of k_finalize's fused CG tail
    DevBuf<float> d_hcache;        // activation cache of one CG solve (policy_mfma.hip OP_FVPC)
    DevBuf<void> d_sub;            // metrpo_subsample_batch: the gathered sub-batch (obs | old_mean | old_log_std | valid), valid until the next call of that entry point
    DevBuf<void> d_merr; DevBuf<double> d_merr_part;   // model_error.hip: trajectory of the diagnostic's rollout (obs | act | mean | rew | tpath | done | window starts | ts | model) | arrival ticket + per-workgroup sums of k_pred_error
    DevBuf<double> d_ppo_kl;       // run_ppo_kl_update / launch_ppo_kl_loss_grad: one [loss, mean KL] pair per epoch, written by the OP_LOSSKL reduction and read by the OP_PPOKL kernels
    DevBuf<void> d_mig; int mig_epoch = 0;        // rollout_coop.hip: hand-over slots of migrating tiles (flag | ts | model | obs per tile)
    void* nccl_comm = nullptr; int comm_world = 0, comm_rank = 0;   // comm.hip: RCCL communicator attached by metrpo_comm_init (NULL: single rank)
    // comm.hip: one-shot direct all-reduce (xchg_device.h).  xg_region = this rank's receive region (IPC-exported), xg_peer[q] = rank q's
    // region as mapped here; xg_seq counts the exchanges issued so far (identical on every rank: SPMD)
    void* xg_region = nullptr; void* xg_peer[XCHG_MAX_WORLD] = {}; int xg_world = 0, xg_rank = 0, xg_cap = 0; unsigned int xg_seq = 0; unsigned long long xg_timeout = 0;
    int pol_path = 1;        // 1 auto (fused MFMA kernels where the shape has them, GEMM path for large N otherwise), 0 generic forced, 2 GEMM path forced
    DevBuf<void> d_pg; long long pg_fwd_rows = -1; const float* pg_fwd_obs = nullptr;   // policy_gemm.hip workspace + validity of its cached forward pass
    int pol_f3 = 0;          // 1: fused MFMA update kernels for three-hidden-layer policies (policy_fused3.hip) serve this shape
    DevBuf<void> d_f3; long long f3_rows = -1; const float* f3_obs = nullptr; const float* f3_theta = nullptr; int f3_img_ok = 0;   // policy_fused3.hip: activation cache + mean-adjoint of one (theta, batch) and its validity
    DevBuf<void> d_adam;     // Adam moments [2][K][Pd] + loss accumulators (dyn_train.hip)
    long long adam_t = 0;    // Adam step count
    DevBuf<void> d_train;    // training activation workspace
    DevBuf<double> d_train_part;   // k_train_out: per-model arrival tickets + per-workgroup loss sums (added in workgroup order)
    DevBuf<void> d_big;      // workspace of the GEMM step-wise rollout (rollout_gemm.hip)
    DevBuf<void> d_res; unsigned int res_seq = 0;   // rollout_resident.hip: uncached exchange region (abort cell | X packets | P packets) and the step stamps issued so far
    DevBuf<unsigned long long> d_skp_stats; int skp_stats_n = 0;   // option PERSIST_STATS: per-workgroup statistics of the last persistent launch (metrpo_debug_persist_stats) | its workgroup count
    std::vector<int> skp_tab_host;                    // host copy of the table below, as raw 32-bit words (source of its asynchronous upload; SkRec: mlp_streamk.h)
    DevBuf<void> d_skp_tab; long long skp_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1}; int skp_Jx[8] = {}, skp_Jmax = 0, skp_L = 0, skp_NSL = 0; int persist_failed = 0;   // mlp_persist.h: cached chunk-record table of the persistent stream-K rollout (key: the launch's shape) | a persistent launch timed out
    int res_failed = 0;                                   // a resident launch gave up (its grid was not co-resident): this context stays on the step-wise path from then on
    int last_ract_kernel = -1;                            // metrpo_rollout_actions (rollout_actions.hip): -1 none yet, 0 step loop, 1 fused
    DevBuf<int32_t> d_ract_model;                         // ... its step loop's [B] head vector when the caller gave uniform_model instead of d_model
    int last_dis_kernel = -1;                             // metrpo_ensemble_disagreement (disagreement.hip): -1 none yet, 0 generic, 1 fused
    DevBuf<void> d_dis; int dis_per_cu = 0;               // ... its workspace (generic: every head's next state | metrpo_step's s_next, reward, done; either path: the scores when only d_sums is asked for) | workgroups of the fused kernel per CU (0: not asked yet)
    int last_sact_kernel = -1; DevBuf<void> d_sact;       // metrpo_score_actions (score_actions.hip): -1 none yet, 0 generic, 1 fused | the generic path's chunk workspace (obs | rew | done | the chunk's actions)
    int last_sagr_kernel = -1; DevBuf<void> d_sagr;       // metrpo_score_actions_grad (score_actions_grad.hip): -1 none yet, 0 generic, 1 fused | a chunk's states and weights (XS | WT)
    int last_spol_kernel = -1; DevBuf<void> d_spol;       // metrpo_score_policy_actions (score_policy_actions.hip): -1 none yet, 0 generic, 1 fused | the generic path's chunk workspace (start | two state rows | act | mean | rew | done | head vectors)
    int last_spag_kernel = -1; DevBuf<void> d_spag;       // metrpo_score_policy_actions_grad (score_policy_actions_grad.hip): -1 none yet, 0 generic, 1 fused | a chunk's states, weights and per-head actions (XS | WT | AW)
    DevBuf<float> d_tv; int tv_n_bias = 0;                // metrpo_set_terminal_value: w1 [ns] | w2 [ns] | bias [n_bias], read by the four scoring calls above (sact_sum.h: TermVal) | 0: none set
    int tv_kind = 0;                                      // ... which form d_tv holds while tv_n_bias > 0: 1 the quadratic above, 2 metrpo_set_terminal_value_mlp's zero-padded image | bias (sact_sum.h: tvm_*)
    int spol_chunk_cap = 0;                               // ... test hook (metrpo_debug_score_policy_chunk): at most this many candidates per chunk of its generic path; 0: the 2^26-float rule alone
    DevBuf<void> d_svg; int last_svg_path = -1;         // svg.hip: workspace of metrpo_svg_grad / _update (zeroed copy of the rollouts | mean-adjoint | F | Pi | chunk buffers | lambda_0 | gradient) | -1 none yet, 1 generic, 2 GEMM
    int coop_no_split = 0;                                // switch (metrpo_set_coop_split): 1 keeps the 4-wave form of the cooperative kernel where the head-split form would run
    int last_coop_waves = 0;                              // waves per workgroup of the last cooperative launch: 4, or 8 (head-split form); diagnostics (metrpo_debug_coop_waves)
    int last_rollout_kernel = -1;                         // which kernel family the last metrpo_rollout ran on: 0 generic, 1 head-per-wave MFMA, 2 cooperative MFMA, 3 step-wise GEMM, 4 resident
    int dyn_precision = METRPO_DYN_F32;                   // metrpo_set_dyn_precision: operand precision of the dynamics forward inside metrpo_rollout (rollout_bf16.hip)
    DevBuf<uint16_t> d_dyn_bf16;                          // ... its bf16 weight image [K][layer][N][Kp], rebuilt from d_dyn in front of every bf16 rollout call
    int bf16_last_layers = 0, bf16_last_bn[MAXL] = {};    // ... the column tile (64 / 128) of every layer GEMM of its last step, written on the host by launch_bf16_layers (metrpo_debug_last_bf16_layers)
    // metrpo_trpo_update_begin / _end: an update whose line search is still undecided on the host
    // metrpo_trpo_update_begin's outcome lands in pinned host memory straight from its last kernel (k_ls_publish: scal | lk | ls, then a
    // stamp); _end polls the stamp (no copy engine, no event, no blocking wait to wake up from).  Publishing from a side stream behind a device-scope
    // event was measured too: the second queue costs the update 35 us, more than the 15 us gap in front of the next rollout it removes.
    double* h_upd = nullptr; unsigned long long upd_stamp = 0;
    // lbfgs.hip: the L-BFGS state (float64 vectors, S / Y ring, scalars) of the open minimisation, its shape, and the pinned slots its step kernels
    // publish their task word into (one per evaluation in flight, stamped)
    DevBuf<double> d_lb; int lb_n = 0, lb_m = 0, lb_open = 0; double* h_lb = nullptr; unsigned long long lb_stamp = 0;
    int upd_pending = 0, upd_spec = 0, upd_changed_in_end = 0; metrpo_batch upd_batch = {}; metrpo_trpo_params upd_params = {}; metrpo_trpo_diag upd_diag = {};
    hipStream_t side_stream[METRPO_MAX_PAR_ROUNDS - 1] = {}; hipEvent_t ev_fork = nullptr, ev_join[METRPO_MAX_PAR_ROUNDS - 1] = {}; int side_ready = 0;   // rollout_gemm.hip: independent rounds of a small-batch rollout run concurrently
    double* h_pinned = nullptr;    // pinned host scratch for the per-trial read-back
    int n_sm = 256;          // CU count (device property)
    int upd_tiles_per_wave = 1;   // MFMA update kernels: at least this many 16-sample tiles per wave before another block is added (1; the option that set it was retired in round 6: experiments/upd_small.py)
    int n_cu_sched = 0;      // CUs that actually ran this process's waves (probe.hip: census; 0 = not measured yet)
    int exclusive = 1;       // the caller's metrpo_set_exclusive value (1 at metrpo_create); 0: the GPU is shared with other compute processes.  Read through ctx_exclusive(), which also honours option NO_RESIDENT
    std::string opt_val[OPT_COUNT]; bool opt_set[OPT_COUNT] = {};   // METRPO_OPT_LIST: set by metrpo_create from the environment, then only by metrpo_set_option
    hipEvent_t fvp_ev[32] = {}; int fvp_ev_n = 0, fvp_ev_made = 0;   // option TIME_FVP: events around the Fisher-vector-product kernel of launch_fvp_tail (metrpo_debug_fvp_us)
    // the last policy-update launch, written on the host when it is enqueued (metrpo_debug_last_update): family (0 generic, 1 fused 2 x 32, 2 GEMM path, 3 fused 100-50-25),
    // UpdOp as launched (OP_FVPC where the fused kernel took it), index into policy_mfma.hip's table (-1 elsewhere), sample tile of the generic kernels (0 elsewhere),
    // partial rows handed to k_finalize (0 on the GEMM path), splits / kchunk of the GEMM path's gradient GEMMs (0 elsewhere)
    struct UpdLast { int family = -1, op = -1, table = -1, pt = 0, nrows = 0, splits = 0, kchunk = 0; } upd_last;
    // the Fisher-vector products of the last CG solve run_trpo_update enqueued (metrpo_debug_last_solve), written on the host from upd_last after each of them:
    // family / op / table of the last product (-1: the solve made none), their count (step-scale product included), and the SolveScope / fusion the solve ran under
    struct SolveLast { int family = -1, op = -1, table = -1, n_fvp = 0, cache_activations = 0, publish_image = 0, fused_tails = 0, fvp_batch = 0; } solve_last;
    // the last metrpo_rollout on a GEMM-class or resident family, written on the host while it is enqueued (metrpo_debug_last_rollout_launch; rollout_gemm.hip,
    // rollout_resident.hip): pre-step kind (0 2 x 32 MFMA, 1 the same with the previous step's post merged in, 2 Humanoid MFMA3, 3 MFMA3 split, 4 GEMM chain,
    // 5 VALU k_big_pre, 6 MFMA3 with the post merged in; -1: none), k_big_post's lanes per env (0: a persistent or resident launch closes the steps), SkPath::mode,
    // SkArgs::late of the launch that carries the output layer, layer-0 route (0 producer, 1 k_l0_rows, 2 tile GEMM), fused output tile, partials of the output
    // layer that k_big_post adds (0: unsplit), persistent: two-block tiles | closing workgroups, rounds (0 single, 1 parallel streams, 2 merged),
    // resident: slice width | threads | post waves per workgroup | rounds per launch group | rotating deal.  All 0 / -1 on every other family.
    struct RollLast { int pre = -1, post_width = 0, sk_mode = 0, late = 0, l0_route = 0, fuse_tile = 0, out_splits = 0, persist_wide = 0, nclose = 0, rounds = 0,
                      res_ws = 0, res_threads = 0, res_pw = 0, res_rg = 0, res_rot = 0; } roll_last;
    std::string rollout_note;   // why the last metrpo_rollout left the fast dispatch table ("" when it did not): metrpo_rollout_note
    int fallback_logged = 0;  // a rollout shape that fell off the fast dispatch table has been reported once (METRPO_VERBOSE)
    std::vector<std::pair<void*, size_t>> ws_retired; size_t ws_retired_bytes = 0;   // outgrown workspaces and their sizes (ws_grow below): freed by metrpo_destroy, or by one sweep once they pass WS_RETIRED_MAX
    std::string err;
};

// Workspace growth inside a launch entry point (a larger B / N than any call before).  hipFree waits for the whole device -- every stream of the process -- while the
// ABI promises stream-ordered calls (include/metrpo.h, Threading): an outgrown buffer is RETIRED instead of freed.  Kernels already enqueued on any stream may still
// read it, which is exactly what retiring allows.  Retired buffers go at metrpo_destroy; a caller that sweeps ever larger shapes through ONE context pays one
// synchronising sweep whenever the retired bytes pass WS_RETIRED_MAX (or an allocation fails), a loop at fixed shapes never does.  hipMalloc does not wait for
// running work (tests/test_gpu_api.py::test_rollout_at_a_larger_batch_does_not_wait_for_other_streams).
constexpr size_t WS_RETIRED_MAX = (size_t)4 << 30;
static inline void ws_sweep(metrpo_ctx* c) {
    for (const auto& r : c->ws_retired) (void)hipFree(r.first);   // (the first hipFree waits for the device)
    c->ws_retired.clear(); c->ws_retired_bytes = 0;
}
int set_err(metrpo_ctx* c, int code, const std::string& msg);
// The one way a context-owned buffer gets memory: afterwards it holds at least `bytes`.  When it has to grow, the old buffer is retired with its size
// and a new one of exactly `bytes` is allocated (a failure for lack of memory sweeps the retired buffers and tries once more); *grew then reports
// that the contents are new and uninitialised.  On failure the buffer is left empty.
template <class T> static inline int ws_grow(metrpo_ctx* c, DevBuf<T>& b, size_t bytes, bool* grew = nullptr) {
    if (grew) *grew = false;
    if (bytes <= b.bytes) return METRPO_OK;
    if (b.p) {
        c->ws_retired.emplace_back((void*)b.p, b.bytes); c->ws_retired_bytes += b.bytes;
        b.p = nullptr; b.bytes = 0;
        if (c->ws_retired_bytes > WS_RETIRED_MAX) ws_sweep(c);
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory && !c->ws_retired.empty()) { (void)hipGetLastError(); ws_sweep(c); e = hipMalloc(&p, bytes); }
    if (e != hipSuccess) return set_err(c, METRPO_EHIP, "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    b.p = (T*)p; b.bytes = bytes;
    if (grew) *grew = true;
    return METRPO_OK;
}

// value of a switch, NULL when unset -- the same contract as the getenv() calls these replaced
static inline const char* ctx_opt(const metrpo_ctx* c, int id) { return c->opt_set[id] ? c->opt_val[id].c_str() : nullptr; }
// kernels that wait on other workgroups of their own launch may be selected: the caller said the device is its own (metrpo_set_exclusive) AND option NO_RESIDENT is unset
static inline bool ctx_exclusive(const metrpo_ctx* c) { return c->exclusive != 0 && ctx_opt(c, OPT_NO_RESIDENT) == nullptr; }
// the three-hidden-layer fused update kernels (policy_fused3.hip) serve an update launch of this context; vjp: the launch is the VJP mode of the gradient
// kernels (PolK::gm supplied), which they do not have (GEMM path)
static inline bool f3_active(const metrpo_ctx* c, bool vjp) { return c->pol_f3 != 0 && c->pol_path == 1 && !vjp && ctx_opt(c, OPT_NO_POL_FUSED3) == nullptr; }
const char* metrpo_opt_name(int id);
int metrpo_opt_id(const char* key);       // -1: unknown

struct RolloutK {          // device-side copy of metrpo_rollout_args (plain pointers)
    int B, T, H, sam_mode, determ, eval_all, n_pool;
    uint64_t seed, stream_offset;
    const float* pool;
    const float* eps;
    const int32_t* model_idx;
    const float* sel_noise;
    const int32_t* reset_idx;
    const int32_t* reset_model;
    float* obs; float* act; float* rew; float* mean; uint8_t* done; int32_t* tpath; float* last_obs;
    // continuation (metrpo_rollout_args ABI 2)
    int t0; const float* init_obs; const int32_t* init_ts; const int32_t* init_model;
    int32_t* last_ts; int32_t* last_model; const int32_t* stop;
    long long stop_batch; const double* stop_cum;     // in-launch stop rule (metrpo_rollout_args ABI 4): honoured by the persistent stream-K rollout only
    // tile migration of the cooperative kernel (rollout_coop.hip; ctx-owned hand-over slots, NULL elsewhere)
    int32_t* mig_flag; float* mig_obs; int32_t* mig_ts; int32_t* mig_model; int mig_epoch; double* mig_err;
    // merged rounds of the step-wise path (rollout_gemm.hip): vB > 0 -> the B rows of this launch are vR rounds of vB envs, row b = env b % vB of round
    // b / vB, whose steps are the rows t + (b / vB) * H of the trajectory tensors (vB envs per row) and of the draw counters
    int vB, vR;
};
// env index within its round (Philox stream, column of the trajectory row) | first step of the env's round | envs per trajectory row
#define RK_ENV(r, b) ((r).vB ? (b) % (r).vB : (b))
#define RK_TOFF(r, b) ((r).vB ? ((b) / (r).vB) * (r).H : 0)
#define RK_STRIDE(r) ((r).vB ? (r).vB : (r).B)
#define RK_LAST_ROUND(r, b) (!(r).vB || (b) / (r).vB == (r).vR - 1)

static inline RolloutK make_rollout_k(const metrpo_rollout_args* a) {
    RolloutK r;
    r.B = a->B; r.T = a->T; r.H = a->H; r.sam_mode = a->sam_mode; r.determ = a->determ; r.eval_all = a->eval_all_heads;
    r.n_pool = a->n_pool; r.seed = a->seed; r.stream_offset = a->stream_offset; r.pool = a->d_pool; r.eps = a->d_eps;
    r.model_idx = a->d_model_idx; r.sel_noise = a->d_sel_noise; r.reset_idx = a->d_reset_idx;
    r.reset_model = a->d_reset_model; r.obs = a->d_obs; r.act = a->d_act; r.rew = a->d_rew; r.mean = a->d_mean;
    r.done = a->d_done; r.tpath = a->d_tpath; r.last_obs = a->d_last_obs;
    r.t0 = a->t0; r.init_obs = a->d_init_obs; r.init_ts = a->d_init_ts; r.init_model = a->d_init_model;
    r.last_ts = a->d_last_ts; r.last_model = a->d_last_model; r.stop = a->d_stop;
    r.stop_batch = a->stop_batch; r.stop_cum = a->d_stop_cum;
    r.mig_flag = nullptr; r.mig_obs = nullptr; r.mig_ts = nullptr; r.mig_model = nullptr; r.mig_epoch = 0; r.mig_err = nullptr;
    r.vB = 0; r.vR = 0;
    return r;
}

struct PolK {
    const float* obs; const float* act; const float* adv; const float* old_mean; const float* old_ls;
    int ls_stride;
    float clip_lo;           // OP_PPO: the clip bounds 1 - c and 1 + c (ppo.py:112).  The two floats sit where the struct had alignment padding, so every
    const uint8_t* valid; long long N; float inv_n;
    float clip_hi;           // other member keeps its offset and the other instantiations their argument layout
    const float* gm;         // non-NULL: VJP mode of the gradient kernels (bptt.hip): d objective / d mean [N][na] supplied, no loss terms
    const int* img_map;      // policy_mfma.hip: gather map of the LDS weight-fragment image (built once per ctx on the host)
    const double* skip;      // non-NULL: a line-search trial that leaves at once when skip[0] >= 0 (the search already stopped: CgTail::ls)
    float* imgval;           // policy_mfma.hip: non-NULL under SolveScope::publish_image -- gradient kernel: block 0 publishes its image here; OP_FVPC: the image to copy
    float* hcache;           // policy_mfma.hip: hidden activations of (theta, batch): written by the gradient kernel, read by OP_FVPC
    // OP_PPOKL (ppo.py:120-121; last, so that every member above keeps its offset): the reduced GLOBAL mean KL at the theta of this launch, one float64 on
    // the device (read by every wave, a uniform load; the gate mean_kl[0] - kl_delta > 0 is taken in float64), step_size, kl_penalty
    const double* mean_kl; double kl_delta; float kl_beta;
};

// ---- one policy-update launch (policy_update.hip run_update) ------------------------------------------------------------------------------------
// The operation, shared by the four kernel families (generic, fused MFMA, fused 100-50-25, GEMM path).  The values are template arguments of the
// kernels (as int: an unscoped enum converts) and the index into policy_mfma.hip's kern[] table.
enum UpdOp {
    OP_GRAD = 0,      // surrogate loss + gradient (with PolK::gm: the VJP of bptt.hip)
    OP_FVP = 1,       // Fisher-vector product
    OP_LOSSKL = 2,    // loss + KL at a trial theta (line search)
    OP_FVPC = 3,      // policy_mfma.hip only, chosen by its launcher: OP_FVP on the activations the gradient kernel cached
    OP_VPG = 4,       // OP_GRAD with the VPG surrogate's head (algos/vpg.py: ratio 1, loss = -mean(logli * adv))
    OP_PPO = 5,       // OP_GRAD with PPO's clipped head (algos/ppo.py:107-117): loss = -mean(min(lr adv, clip(lr) adv)), a clipped sample carries no gradient;
                      // block 0 also leaves the entropy sum(ls) + na/2 (1 + log 2 pi) of the entry theta in column P+1 of its partial row (ppo_entropy_term)
    OP_PPOKL = 6,     // OP_PPO plus ppo.py:120-121's penalty kl_penalty * max(0, mean_kl - step_size): with the gate open (PolK::mean_kl, ppo_kl_open) every valid sample
                      // adds kl_beta * inv_n * (kl_i - kl_delta) to the loss and kl_beta * inv_n * d kl_i / d (mean, log_std) to its seed; gate closed: OP_PPO's results
};
// What the enclosing solve lets a launch rely on; run_trpo_update / run_vpg_update build one on their stack, every launch outside a solve passes the all-off default.
struct SolveScope {
    bool cache_activations = false;   // the gradient launch keeps its forward pass, the Fisher-vector products of the same (theta, batch) reuse it
    bool publish_image = false;       // policy_mfma.hip: gradient kernel and fused CG tails maintain d_pol_imgval (needs cache_activations)
    bool exchange_in_tail = false;    // sharded run: k_finalize adds the ranks' shares in its own tail (one-shot exchange, xchg_device.h)
};
struct CgTail;
struct AdamTail;
struct UpdCall {
    UpdOp op;
    PolK k;                  // batch; gm / skip set by the caller, img_map / imgval / hcache by policy_mfma_launch
    const float* theta;
    const float* vf;         // OP_FVP: float copy of the tangent vector
    const double* v64;       // OP_FVP: the tangent vector (log_std rows)
    double* out;
    const CgTail* tail;      // step fused into the reduction's tail, or NULL
    const AdamTail* adam;    // k_finalize only: Adam step on the reduced gradient, or NULL
    double ent_coeff;        // OP_PPO: entropy_bonus_coeff (ppo.py:119), applied where the gradient is reduced
    bool ent_in_reduction;   // OP_PPO: k_finalize adds the entropy term (false: a stand-alone k_ppo_step does, behind the ranks' sum)
    SolveScope scope;
};

int policy_mfma_select(const ProblemDesc& pd);
int policy_mfma_image_buffers(metrpo_ctx*);   // gather map, its inverse for the tangent entries and the image-value buffer of ctx->pol_mfma (idempotent)
int policy_mfma_launch(metrpo_ctx*, const UpdCall&, float* partials, int nblocks, hipStream_t);

#define HIP_TRY(c, expr)                                                                      \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return set_err((c), METRPO_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// launch helpers implemented in the individual .hip files
int launch_policy_actions(metrpo_ctx*, const float*, const float*, int, float*, float*, hipStream_t);
int launch_step(metrpo_ctx*, const float*, const float*, int, int, const int32_t*, const float*, float*, float*,
                uint8_t*, float*, hipStream_t);
int launch_rollout_generic(metrpo_ctx*, const metrpo_rollout_args*, hipStream_t);
bool gemm_path_applicable(const metrpo_ctx*);
int sched_cus(metrpo_ctx*, hipStream_t);
bool grid_is_coresident(metrpo_ctx*, const void* kernel, int threads, size_t lds, long long grid, hipStream_t);
int launch_rollout_gemm(metrpo_ctx*, const metrpo_rollout_args*, hipStream_t);
// rollout_bf16.hip: the bf16-operand dynamics layers of metrpo_rollout (METRPO_DYN_BF16).  Image of one head: layer l at off[l], [dims[l + 1]][Kp[l]] bf16
struct Bf16Img { int Kp[MAXL]; size_t off[MAXL]; size_t per_head; };
Bf16Img bf16_img_layout(const ProblemDesc&);
struct Bf16GemmForm { int bn, gx, gy, gz; };               // one layer GEMM's launch: column tile and grid (column tiles, 128-row tiles, heads)
Bf16GemmForm gemm_bf16_form(int n_cu, int M, int N, int heads, int force_bn = 0);
int launch_bf16_dyn_image(metrpo_ctx*, hipStream_t);      // d_dyn -> d_dyn_bf16
size_t bf16_hidden_floats(const ProblemDesc&, int B);      // floats of one hidden-activation buffer ([K][B][width up to 64] bf16)
int launch_bf16_layers(metrpo_ctx*, const float* X, int ldx, void* HA, void* HB, float* OUT, int B, hipStream_t);      // one step's layers: X f32 -> OUT [K][B][ns] f32
int launch_rollout_resident(metrpo_ctx*, const metrpo_rollout_args*, hipStream_t);   // METRPO_EUNSUPPORTED: not a shape / call of the resident kernel
// 'bptt-stochastic' policy noise of one BPTT gradient (bptt.hip): u = clip(mean + eps * exp(log_std)).  Drawn by device_common.h bptt_eps4.
struct BpttNoise {
    const float* eps;               // parity mode: [K][T][B][na] draws; NULL: Philox4x32-10, purpose RNG_BPTT, key = seed
    const float* log_std;           // [na] raw parameter (d_theta + pol.n_params)
    int* n_sat;                     // [B][na] int32 count of |u| == 1 over models and steps (forward sweep), or NULL
    unsigned long long seed;
    int T;
};
// nz == NULL: the deterministic 'bptt' gradient
int launch_bptt_grad(metrpo_ctx*, const float* init, int B, int T, double gamma, double* costs, double* grad, hipStream_t, const BpttNoise* nz = nullptr);
int launch_policy_adam(metrpo_ctx*, const double* grad, double lr, double b1, double b2, double eps, double clip_val, bool reset, hipStream_t);
int ensure_policy_adam(metrpo_ctx*);                 // bptt.hip: allocate the zeroed policy optimizer state + segment table (first Adam step / reset / set)
int ensure_dyn_adam(metrpo_ctx*);                    // dyn_train.hip: allocate the zeroed dynamics optimizer state (first train step / set)
size_t dyn_adam_floats(const metrpo_ctx*);           // floats of ONE moment array in d_adam ([K][Pd] rounded up to 4)
int det_mfma_select(const metrpo_ctx*);
int launch_det_forward(metrpo_ctx*, int idx, const float* s0, int B, int T, double gamma, float* XS, float* WT, double* part, double* costs, hipStream_t,
                       const BpttNoise* nz = nullptr);
int launch_det_backward(metrpo_ctx*, int idx, int B, int T, const float* XS, const float* WT, float* GM, hipStream_t, const BpttNoise* nz = nullptr);
int ensure_detpart(metrpo_ctx*, int B);
int ensure_detpart_n(metrpo_ctx*, size_t n_doubles);
int launch_det_cost_reduce(metrpo_ctx*, int n_part, const double* part, double* costs, hipStream_t, const double* err = nullptr);   // err: time-out cell of the launch that wrote the partials (NaN costs when set)
int launch_validation_resident(metrpo_ctx*, const float* s0, int Bv, int T, double gamma, double* costs, hipStream_t);   // rollout_resident.hip; METRPO_EUNSUPPORTED: not this shape
bool det_gemm_applicable(const metrpo_ctx*);
int launch_dg_forward(metrpo_ctx*, const float* s0, int B, int T, double gamma, float* XS, float* WT, double* costs, hipStream_t,
                      const BpttNoise* nz = nullptr);
int launch_dg_backward(metrpo_ctx*, int B, int T, const float* XS, const float* WT, float* GM, hipStream_t, const BpttNoise* nz = nullptr);
int launch_policy_vjp(metrpo_ctx*, const float* obs, const float* gm, long long N, double* out, hipStream_t);
int launch_dyn_train_step(metrpo_ctx*, const float*, const float*, const metrpo_train_params*, double*, hipStream_t);
int launch_dyn_eval_losses(metrpo_ctx*, const float*, const float*, long long, double, double*, hipStream_t);
int launch_rms_accumulate(metrpo_ctx*, const float*, long long, int, double*, double*, hipStream_t);
int launch_rollout_mfma(metrpo_ctx*, const metrpo_rollout_args*, hipStream_t, int* coop = nullptr);   // returns METRPO_EUNSUPPORTED if no instantiation fits; *coop = 1: the cooperative kernel ran
int mfma_prepare_dynamics(metrpo_ctx*, hipStream_t);
int mfma_prepare_policy(metrpo_ctx*, hipStream_t);
int mfma_select_config(metrpo_ctx*);
int mfma_shape_config(const metrpo_ctx*);
int coop_select_config(metrpo_ctx*);
int launch_rollout_coop(metrpo_ctx*, int idx, const RolloutK&, hipStream_t, bool padded = false);
int launch_pad_dyn(metrpo_ctx*, hipStream_t);      // d_dyn -> d_dyn_pad (zero-padded 64 x 64 layout)
// Host side of the fused head kernels on dyn_tile_step.h (rollout_actions.hip, which has these functions; score_actions.hip; disagreement.hip).
// Do they hold this context?  The fused rollout kernels' shape class with two hidden layers of 64 (*padded = false), or narrower ones through the
// zero-padded copy d_dyn_pad that metrpo_create made for them (*padded = true), and at most k_cap heads: 8 where a workgroup has a wave per head,
// 65535 where the heads are gridDim.y.
bool fused_head_class(const metrpo_ctx*, int k_cap, bool* padded);
int fused_head_dyn(metrpo_ctx*, bool padded, hipStream_t, const float** dyn);   // the ensemble to launch with: d_dyn, or d_dyn_pad behind launch_pad_dyn
int allow_dynamic_lds(metrpo_ctx*, const void* kernel, size_t bytes);           // above 64 KB a kernel needs the attribute before it is launched
// their per-env tables: one ENTRY(env id) per env of the class, rows with a member `env`
#define FUSED_HEAD_ENVS(ENTRY) ENTRY(METRPO_ENV_SWIMMER), ENTRY(METRPO_ENV_HALF_CHEETAH), ENTRY(METRPO_ENV_HOPPER), ENTRY(METRPO_ENV_SNAKE), ENTRY(METRPO_ENV_ANT)
template <class E, size_t N> static inline const E* fused_head_entry(const E (&tab)[N], const metrpo_ctx* c, int k_cap, bool* padded) {
    if (!fused_head_class(c, k_cap, padded)) return nullptr;
    for (const E& en : tab)
        if (en.env == c->pd.env) return &en;
    return nullptr;
}
int launch_validation_cost(metrpo_ctx*, const float*, int, int, double, double*, hipStream_t);
int launch_gae(metrpo_ctx*, const float*, const float*, const uint8_t*, const int32_t*, int, int, const double*,
               double, double, float*, float*, uint8_t*, double*, hipStream_t);
int launch_center(metrpo_ctx*, float*, const uint8_t*, int64_t, const double*, hipStream_t);
int launch_process_begin(metrpo_ctx*, float*, double*, int64_t, hipStream_t);
int launch_sampler_progress(metrpo_ctx*, const uint8_t*, const int32_t*, int, int, int, long long, double*, double*, int32_t*, hipStream_t);
int launch_baseline_solve(metrpo_ctx*, const double* AtA, const double* Aty, double reg, double* coeffs, hipStream_t);
int launch_gram(metrpo_ctx*, const float*, const float*, const int32_t*, const uint8_t*, int64_t, double*, double*,
                hipStream_t);
int launch_loss_grad(metrpo_ctx*, const metrpo_batch*, double*, hipStream_t, const CgTail* tail = nullptr, SolveScope = {});
// 'vpg' policy update (algos/vpg.py): the gradient kernels of every update family in their OP_VPG instantiation
int launch_vpg_loss_grad(metrpo_ctx*, const metrpo_batch*, double* out, hipStream_t);
int run_vpg_update(metrpo_ctx*, const metrpo_batch*, const metrpo_vpg_params*, double* d_loss, hipStream_t);
// 'ppo' policy update (algos/ppo.py): the OP_PPO instantiations, the entropy term in the reduction, n_epochs Adam steps with the old distribution fixed
int launch_ppo_loss_grad(metrpo_ctx*, const metrpo_batch*, const metrpo_ppo_params*, double* out, hipStream_t);
int run_ppo_update(metrpo_ctx*, const metrpo_batch*, const metrpo_ppo_params*, int n_epochs, double* d_losses, hipStream_t);
// ... with use_kl_penalty (ppo.py:120-121): the OP_PPOKL instantiations behind an OP_LOSSKL launch that leaves the mean KL of the same theta on the device
int launch_ppo_kl_loss_grad(metrpo_ctx*, const metrpo_batch*, const metrpo_ppo_params*, const metrpo_ppo_kl_params*, const double* d_mean_kl, double* out, hipStream_t);
int run_ppo_kl_update(metrpo_ctx*, const metrpo_batch*, const metrpo_ppo_params*, const metrpo_ppo_kl_params*, int n_epochs, double* d_losses, double* d_mean_kls, hipStream_t);
// 'l-bfgs' policy update (lbfgs.hip): the reverse-communication L-BFGS-B core and the BPTT-driven minimisation
int lbfgs_begin(metrpo_ctx*, int n, const double* x0, const float* x0_f32, const metrpo_lbfgs_opts*, double* x_eval, hipStream_t);
int lbfgs_iterate(metrpo_ctx*, const double* f, const double* g, double* x_eval, int32_t* task, hipStream_t);
int lbfgs_get_result(metrpo_ctx*, metrpo_lbfgs_result*, hipStream_t);
int run_lbfgs_policy(metrpo_ctx*, const float* init, int B, int T, double gamma, const metrpo_lbfgs_opts*, metrpo_lbfgs_result*, hipStream_t);
int comm_allreduce_f64(metrpo_ctx*, double* buf, long long count, hipStream_t);
// descriptor of the NEXT one-shot exchange (advances the sequence number); world = 0 when no peer-mapped transport is attached
XchgK xchg_next(metrpo_ctx*);
static inline XchgK xchg_none() { XchgK x = {}; return x; }
// scal[S_COMMERR] of the CG workspace (gout[1+P] | x r p z step [5P] | scal[8] | lk[2]): sticky error cell of the exchanges
static inline double* comm_err_cell(metrpo_ctx* c) { return c->d_cg.p + (size_t)(1 + c->pd.P) + 5 * (size_t)c->pd.P + 6; }
// time-out cell of the resident VALIDATION launches (behind scal | lk | ls): cleared in front of every such launch, so an earlier rollout's sticky S_ROLLERR
// cannot poison validation costs and a validation time-out cannot be mistaken for a rollout's
static inline double* val_err_cell(metrpo_ctx* c) { return comm_err_cell(c) + 8; }
// sticky cell of metrpo_subsample_batch (behind the validation cell): raised by the gather kernel when it had to clamp a row index outside [0, N);
// reported and cleared by the next metrpo_trpo_update_fvp / metrpo_comm_check
static inline double* sub_err_cell(metrpo_ctx* c) { return comm_err_cell(c) + 9; }
// A rollout kernel reported a timed-out hand-over (scal[S_ROLLERR]): the trajectories of that launch are invalid.  The cell is cleared so the
// context can go on, and the resident kernel -- the one whose hand-overs need every workgroup of its grid on the chip at once -- is retired.
static inline int rollout_error_seen(metrpo_ctx* c, hipStream_t st) {
    (void)hipMemsetAsync(comm_err_cell(c) + 1, 0, sizeof(double), st);
    const bool was_resident = (c->last_rollout_kernel == 4);
    if (was_resident) c->res_failed = 1;
    if (c->last_rollout_kernel == 6) {
        c->persist_failed = 1;
        return set_err(c, METRPO_EHIP, "rollout: the persistent stream-K kernel's wait for a row block timed out (a workgroup of its grid never ran: is another process using "
                                       "this GPU?); the trajectories of that launch are invalid, later rollouts of this context use the launch-per-step path");
    }
    return set_err(c, METRPO_EHIP, was_resident ? "rollout: the resident kernel's hand-over timed out (a workgroup of its grid never ran: is another process using this GPU?); "
                                                  "the trajectories of that launch are invalid, later rollouts of this context use the step-wise path"
                                                : "rollout: a migrating tile's hand-over timed out (producer workgroup never ran); trajectories are invalid");
}
bool policy_gemm_applicable(const metrpo_ctx*, long long N, bool vjp);   // vjp: as f3_active
// Can the reductions of an update on N samples carry what follows them?  One answer for run_trpo_update, its device-side line search and run_vpg_update:
// the ranks of a sharded run must agree on it, or they issue different numbers of exchanges.  has_callback: the caller brought its own all-reduce
// (metrpo_trpo_params::allreduce).  Asked with no VJP open: an update never is one.
struct UpdFusion {
    bool fused;              // no stand-alone all-reduce (callback, RCCL, chunked exchange) sits between a reduction and its consumer
    bool exchange_in_tail;   // sharded over the one-shot transport, and the reductions add the ranks' shares in their own tail (SolveScope)
    bool finalize_reduces;   // the reduction is k_finalize, not the GEMM path's own kernels: it can carry an accept test or an Adam step
    bool carries_next_step() const { return fused && finalize_reduces; }
};
static inline UpdFusion update_fusion(const metrpo_ctx* c, long long N, bool has_callback) {
    const bool xg = !has_callback && c->xg_world > 1;
    UpdFusion f;
    f.finalize_reduces = !policy_gemm_applicable(c, N, false);
    // in-tail exchange: per-element packets into ONE slot per source (k_finalize does not split); longer vectors take the stand-alone, chunked exchange
    f.exchange_in_tail = xg && f.finalize_reduces && c->pd.P + 1 <= c->xg_cap;
    f.fused = !has_callback && ((c->nccl_comm == nullptr && !xg) || f.exchange_in_tail);
    return f;
}
int policy_f3_select(const ProblemDesc& pd);      // policy_fused3.hip: 1 when the three-hidden-layer kernels cover this policy shape
int policy_f3_launch(metrpo_ctx*, const UpdCall&, float* partials, int nblocks, hipStream_t);
int policy_gemm_run(metrpo_ctx*, const UpdCall&, hipStream_t);
int launch_fvp(metrpo_ctx*, const metrpo_batch*, const double*, double*, hipStream_t);
// FVP + reduction + (in the reduction kernel's last block) the CG vector step described by `tail` (may be NULL)
// vf = float copy of v already on the device (skips the conversion launch); v is still needed for the log_std rows
int launch_fvp_tail(metrpo_ctx*, const metrpo_batch*, const float* vf, const double* v, double* hv, const CgTail* tail, hipStream_t, SolveScope = {});
int launch_loss_kl(metrpo_ctx*, const metrpo_batch*, const float*, double*, hipStream_t, const CgTail* decide = nullptr, SolveScope = {});   // decide: op 4 tail (device-side accept test)
// fvp_batch: the batch the Fisher-vector products see ([rllab] subsample_inputs); NULL or the same batch = the whole batch (the launches of ABI 4's update)
int run_trpo_update(metrpo_ctx*, const metrpo_batch*, const metrpo_trpo_params*, metrpo_trpo_diag*, double*,
                    double*, hipStream_t, int phase = 0, int spec = 0, const metrpo_batch* fvp_batch = nullptr);
// policy_update.hip: gather of the rows d_idx[0 .. m) of `b` into c->d_sub (metrpo_subsample_batch)
// model_error.hip: window gather and the whole diagnostic (metrpo_model_error_windows / metrpo_model_error; arguments checked by the entry points)
int launch_window_starts(metrpo_ctx*, const float* Os, int n, int T, int Tw, float* init_obs, hipStream_t);
int run_model_error(metrpo_ctx*, const metrpo_model_error_args*, hipStream_t);
// rollout_actions.hip: the body of metrpo_rollout_actions (arguments checked by the entry point; B, T > 0).  d_init_obs may BE row 0 of d_obs (model_error.hip)
int run_rollout_actions(metrpo_ctx*, const metrpo_rollout_actions_args*, hipStream_t);
// disagreement.hip: the body of metrpo_ensemble_disagreement (arguments checked by the entry point; 0 < N < 2^31)
int run_disagreement(metrpo_ctx*, const metrpo_disagreement_args*, hipStream_t);
// candidates per chunk of a scoring call whose workspace takes per_cand floats a candidate: the workspace stays within 2^26 floats (svg.hip's rule) unless
// the caller's own chunk (override > 0) says otherwise; never more than B, never less than 1
static inline size_t score_chunk(size_t B, size_t per_cand, size_t override_ = 0) {
    return std::min(B, override_ > 0 ? override_ : std::max<size_t>(1, ((size_t)1 << 26) / per_cand));
}
// threads per block of a generic kernel that keeps floats_per_thread LDS columns: the largest of 64, 32, .. 1 (<= 64 lanes, so a block is one wave and needs
// no barrier) whose columns fit 160 KB; 0: none does
static inline int lds_block_size(size_t floats_per_thread) {
    const size_t LDS_MAX = 160 * 1024;
    int bs = 64;
    while (bs > 1 && floats_per_thread * bs * sizeof(float) > LDS_MAX) bs >>= 1;
    return floats_per_thread * bs * sizeof(float) > LDS_MAX ? 0 : bs;
}
// score_actions.hip: the body of metrpo_score_actions (arguments checked by the entry point; B, T > 0, B % S == 0)
int run_score_actions(metrpo_ctx*, const metrpo_score_actions_args*, hipStream_t);
// ... its generic path's start-row gather (act_c NULL: the start rows only), its reduction over a stored rew / done [T][Bc], and the head statistics of d_ret
void launch_sact_starts(const float* init_obs, const float* actions, int B, int T, int per, int c0, int Bc, int ns, int na, float* obs0, float* act_c, hipStream_t);
struct TermVal;   // sact_sum.h: the context's terminal value; set: sT is the chunk's states behind step T [Bc][ns], c0 the chunk's first candidate, per = B / S
void launch_sact_reduce(const float* rew, const uint8_t* done, int Bc, int T, int stop, double gamma, float* ret, int32_t* len, const TermVal& tv, bool mlp, const float* sT, int ns,
                        int c0, int per, hipStream_t);
// ... the body of metrpo_set_terminal_value_mlp (arguments checked by the entry point): d_tv <- the zero-padded image of d_params | bias, stream-ordered
int run_set_terminal_value_mlp(metrpo_ctx*, const float* d_params, int h1, int h2, const float* d_bias, int n_bias, hipStream_t);
void launch_sact_aggregate(const float* ret, int B, int K, float* mean, float* sd, hipStream_t);
// score_policy_actions.hip: the body of metrpo_score_policy_actions (arguments checked by the entry point; B, T > 0, B % S == 0, policy and dynamics set)
int run_score_policy_actions(metrpo_ctx*, const metrpo_score_policy_actions_args*, hipStream_t);
// score_actions_grad.hip: the body of metrpo_score_actions_grad (arguments checked by the entry point; B, T > 0, B % S == 0, chunk >= 0)
int run_score_actions_grad(metrpo_ctx*, const metrpo_score_actions_grad_args*, hipStream_t);
// ... its head-order mean of d_grad [K][n] (k_sagr_mean), for score_policy_actions_grad.hip as well; reports no error of its own
void launch_sagr_mean(const float* grad, size_t n, int K, float* mean, hipStream_t);
// ... the MLP terminal value's seed of a chunk (k_tv_mlp_seed), for score_policy_actions_grad.hip as well: seed [K][n][ns] = WE * dV/ds at slice T of XS [K][T + 1][n][ns]
void launch_tv_mlp_seed(const TermVal& tv, const float* XS, const float* WE, float* seed, int K, int T, int n, int ns, hipStream_t);
// score_policy_actions_grad.hip: the body of metrpo_score_policy_actions_grad (arguments checked by the entry point; B, T > 0, B % S == 0, chunk >= 0, policy and dynamics set)
int run_score_policy_actions_grad(metrpo_ctx*, const metrpo_score_policy_actions_grad_args*, hipStream_t);
// svg.hip: the body of metrpo_svg_grad / metrpo_svg_update (arguments checked by the entry points); update: the SGD step with `lr` on the ctx theta
int run_svg(metrpo_ctx*, const metrpo_svg_args*, double lr, bool update, hipStream_t);
int launch_subsample(metrpo_ctx*, const metrpo_batch* b, const int32_t* d_idx, long long m, double inv_n_global, metrpo_batch* out, double* d_valid_count, hipStream_t);
