/*
 * metrpo.h -- C ABI of libmetrpo.so: the MI355X (gfx950) implementation of the ME-TRPO
 * policy-optimisation inner loop (imagined rollout -> GAE -> TRPO CG/FVP update).
 *
 * The reference (thanard/me-trpo) is pure Python on TF1.4 + rllab and has NO FFI of its own
 * (SURVEY.md section 2); this header therefore declares the entry points a binding for that path
 * would need, one per reference operation, each citing the reference interface it replaces
 * (file:line under the reference tree).  `[rllab]` marks arithmetic that lives in the reference's
 * third-party dependency rllab (not vendored, no version pinned) and is reached at the cited
 * call site.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - every pointer named `d_*` is DEVICE memory owned by the caller (e.g. torch `data_ptr()`);
 *    the library never frees or retains it past the call, except the `set_*` calls which COPY.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, calls return
 *    without synchronising unless documented.  One ctx per GPU, one host thread per ctx, and the
 *    calls of a ctx on ONE stream at a time (they share ctx-owned workspaces: work of the same ctx
 *    enqueued on two streams is not ordered against itself).
 *  - no launch entry point frees device memory or synchronises the device: a ctx-owned workspace
 *    that has to grow (a B / N larger than any call before) is allocated with hipMalloc and the
 *    outgrown buffer is kept until metrpo_destroy (one synchronising sweep only once 4 GB of
 *    outgrown buffers have piled up in a context that keeps growing its shapes).
 *  - all functions return 0 (METRPO_OK) or a negative metrpo_status; no exception or abort
 *    crosses the ABI; metrpo_last_error() gives the message for the last failure on a ctx.
 *  - arithmetic is float32 on device (TF graph dtype of the reference); CG vectors, reductions
 *    and advantage statistics are float64, as the reference's host-side NumPy is.
 *  - trajectory tensors are TIME-MAJOR: element (t, b) of a [T][B][w] tensor is at
 *    ((t*B)+b)*w.  B = parallel imagined envs (the reference's n_envs), T = steps executed.
 */
#ifndef METRPO_H
#define METRPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define METRPO_ABI_VERSION 4
#define METRPO_MAX_LAYERS 6      /* hidden layers per MLP */

typedef struct metrpo_ctx metrpo_ctx;

typedef enum {
    METRPO_OK = 0,
    METRPO_EINVAL = -1,          /* bad dimension / argument */
    METRPO_ENULL = -2,           /* required pointer is NULL */
    METRPO_EHIP = -3,            /* HIP runtime error, see metrpo_last_error */
    METRPO_EUNSUPPORTED = -4,    /* configuration exceeds this build's limits (e.g. LDS) */
    METRPO_ESTATE = -5,          /* set_dynamics / set_policy not called yet */
    METRPO_UNSET = -100          /* metrpo_get_option: the key is known and has no value (not an error; distinct from METRPO_EINVAL = unknown key) */
} metrpo_status;

/* analytic reward / termination of the env families the reference ships (envs/com_*_env.py) */
typedef enum {
    METRPO_ENV_SWIMMER = 0,      /* envs/com_swimmer_env.py:112-114        */
    METRPO_ENV_HALF_CHEETAH = 1, /* envs/com_half_cheetah_env.py:72-75     */
    METRPO_ENV_ANT = 2,          /* envs/com_ant_env.py:77-83, is_done :88-101 */
    METRPO_ENV_HUMANOID = 3,     /* envs/com_simple_humanoid_env.py:105-109 */
    METRPO_ENV_HOPPER = 4,       /* envs/com_hopper_env.py:94-104          */
    METRPO_ENV_SNAKE = 5         /* envs/com_snake_env.py:81-84            */
} metrpo_env;

/* VecSimpleEnv.get_next_observation sampling modes, env_helpers.py:617-634 */
typedef enum {
    METRPO_SAM_STEP_RAND = 0, METRPO_SAM_EPS_RAND = 1, METRPO_SAM_MODEL_MEAN_STD = 2,
    METRPO_SAM_MODEL_MEAN = 3, METRPO_SAM_MODEL_MED = 4, METRPO_SAM_ONE_MODEL = 5
} metrpo_sam_mode;

typedef enum { METRPO_ACT_IDENTITY = 0, METRPO_ACT_RELU = 1, METRPO_ACT_TANH = 2 } metrpo_act;

/* Static shape of the problem (params/params-<env>.json keys in brackets).
 * Dynamics-model variant: prediction_type "state_change" only (training.py:257).  "second_derivative" (training.py:259-264), the "*_goal"
 * types (:265-268) and use_logit_weights (:234-242) have no field here and no kernel behind it: a host reading such a params file must refuse
 * it by name (me-trpo_amd/engine.py: Engine(prediction_type=..., use_logit_weights=...) raises). */
typedef struct {
    int32_t env;                              /* metrpo_env                                   */
    int32_t ns, na;                           /* state / action dims                          */
    int32_t n_models;                         /* K  [n_models]                                */
    int32_t dyn_n_hidden;                     /* [dynamics_model.hidden_layers]               */
    int32_t dyn_hidden[METRPO_MAX_LAYERS];
    int32_t dyn_act[METRPO_MAX_LAYERS];       /* metrpo_act per hidden layer [.nonlinearity]  */
    int32_t n_drop;                           /* 2: ignore_xy_input, 1: ignore_x_input, 0     */
    int32_t pol_n_hidden;                     /* [policy.hidden_layers], tanh, identity out   */
    int32_t pol_hidden[METRPO_MAX_LAYERS];
} metrpo_dims;

int32_t metrpo_abi_version(void);
const char* metrpo_status_string(int32_t status);

/* ---- context ------------------------------------------------------------------------------ */
int32_t metrpo_create(metrpo_ctx** out, int32_t device, const metrpo_dims* dims);
int32_t metrpo_destroy(metrpo_ctx* ctx);
/* exclusive = 0: other compute processes share this GPU (several ranks per device).  Kernels that wait on other workgroups of their own launch
 * (the resident rollout / validation kernels, the migrating-tile schedule) are then never selected; default 1 (0 when METRPO_NO_RESIDENT is set
 * in the environment).  With exclusive use they are still only launched when the runtime's occupancy answer times the CUs that actually
 * schedule this process's waves (a census: CU masks and partitions count) covers their grid.  No reference counterpart: the reference is
 * single-process and single-session (utils.py:229-232). */
int32_t metrpo_set_exclusive(metrpo_ctx* ctx, int32_t exclusive);
/* Variant / tuning switches of a context (ABI 4).  The reference steers its run with params-*.json and command-line flags (main.py:21-60); this library's
 * kernel-selection switches were process-global METRPO_<KEY> environment variables read inside the launch paths up to ABI 3.  They are now one table per
 * context: metrpo_create() fills the defaults ONCE from the environment (METRPO_<KEY>), afterwards only metrpo_set_option() changes them (value NULL
 * unsets a key; takes effect at the next launch) and metrpo_get_option() reports them (returns the value's length, METRPO_UNSET when unset, METRPO_EINVAL for an unknown
 * key).  Keys: the names metrpo_option_name(i), i = 0, 1, ... returns (NULL beyond the table), e.g. "STREAMK", "NO_STREAMK", "NO_RESIDENT", "SEQ_ROUNDS",
 * "PRE_GEMM"; lower case and a "METRPO_" prefix are accepted.  None of them changes results beyond the summation-order notes in DESIGN.md section 4. */
int32_t metrpo_set_option(metrpo_ctx* ctx, const char* key, const char* value);
int32_t metrpo_get_option(metrpo_ctx* ctx, const char* key, char* buf, int32_t cap);
const char* metrpo_option_name(int32_t index);
const char* metrpo_last_error(const metrpo_ctx* ctx);
/* floats per dynamics model: [W0 (n_in x h0, row-major), b0, W1, b1, ..., Wout, bout]          */
int32_t metrpo_dyn_param_count(const metrpo_ctx* ctx);
/* floats in the flat policy vector, [rllab] get_param_values order: W0,b0,...,Wout,bout,log_std */
int32_t metrpo_policy_param_count(const metrpo_ctx* ctx);

/* Replaces the K `dynamics_model` graph copies + RunningMeanStd read-outs the reference builds at
 * model_based_rl.py:91-97 from training.py:218-269 / running_mean_std.py:22-27.
 * d_params [K][dyn_param_count]; d_in_mean,d_in_std [ns+na]; d_diff_mean,d_diff_std [ns]. COPIES. */
int32_t metrpo_set_dynamics(metrpo_ctx* ctx, const float* d_params, const float* d_in_mean,
                            const float* d_in_std, const float* d_diff_mean, const float* d_diff_std,
                            void* stream);
/* [rllab] policy.set_param_values / get_param_values (used by ConjugateGradientOptimizer and by
 * the snapshot/restore at model_based_rl.py:1127-1129,1291-1293,1400).  d_theta [P]. COPIES. */
int32_t metrpo_set_policy(metrpo_ctx* ctx, const float* d_theta, void* stream);
int32_t metrpo_get_policy(metrpo_ctx* ctx, float* d_theta_out, void* stream);

/* ---- single step API (drop-in granularity of the reference's sampler loop) ---------------- */
/* [rllab] GaussianMLPPolicy.get_actions, called at samplers/vectorized_sampler.py:63.
 * d_obs [B][ns]; d_eps [B][na] N(0,1) draws or NULL (actions = mean, the determ=True path :64-65);
 * outputs d_actions [B][na] (unclipped), d_mean [B][na].  log_std is theta's tail. */
int32_t metrpo_policy_actions(metrpo_ctx* ctx, const float* d_obs, const float* d_eps, int32_t B,
                              float* d_actions, float* d_mean, void* stream);
/* VecSimpleEnv.step minus the horizon/reset bookkeeping: env_helpers.py:599-603 + 609-635.
 * d_s [B][ns]; d_a [B][na] UNCLIPPED (clipped inside, :599); d_model_idx [B] int32 (step_rand:
 * fresh draw, eps_rand: cur_model_idx; ignored otherwise, may be NULL); d_noise [B][ns] for
 * model_mean_std else NULL.  Outputs: d_s_next [B][ns], d_reward [B] (= -cost_np_vec, :601),
 * d_done [B] uint8 (= is_done(s',s'), :603), optional d_next_all [K][B][ns] (all heads, :612). */
int32_t metrpo_step(metrpo_ctx* ctx, const float* d_s, const float* d_a, int32_t B, int32_t sam_mode,
                    const int32_t* d_model_idx, const float* d_noise, float* d_s_next, float* d_reward,
                    uint8_t* d_done, float* d_next_all, void* stream);

/* ---- fused rollout: VectorizedSampler.obtain_samples (samplers/vectorized_sampler.py:45-116)
 *      driving VecSimpleEnv.reset/step (env_helpers.py:585-607) and policy.get_actions ---------- */
typedef struct {
    int32_t B, T, H;             /* envs, steps to execute, max_path_length                      */
    int32_t sam_mode;            /* metrpo_sam_mode                                              */
    int32_t determ;              /* 1: actions = mean (obtain_samples(determ=True), :64-65)      */
    int32_t eval_all_heads;      /* 1: evaluate all K heads every step as the reference does
                                    (env_helpers.py:612); 0: only the selected head where the
                                    mode allows (step_rand/eps_rand/one_model)                   */
    const float* d_pool;         /* [n_pool][ns] initial-state pool standing in for the real
                                    simulator's env.reset() (env_helpers.py:552-555)             */
    int32_t n_pool;
    uint64_t seed;               /* Philox seed for every draw not supplied below                */
    uint64_t stream_offset;      /* added to the Philox counter: rank*B for sharded runs         */
    /* parity mode: explicit draws (any may be NULL -> Philox)                                   */
    const float* d_eps;          /* [T][B][na]  policy noise (np.random.normal in get_actions)   */
    const int32_t* d_model_idx;  /* [T][B]      step_rand index (env_helpers.py:619)             */
    const float* d_sel_noise;    /* [T][B][ns]  model_mean_std noise (:626)                      */
    const int32_t* d_reset_idx;  /* [T+1][B]    pool row used when env b resets AFTER step t-1
                                                (row 0 = the initial reset(), :49/:585-595)      */
    const int32_t* d_reset_model;/* [T+1][B]    cur_model_idx drawn at that reset (:593)         */
    /* outputs, time-major                                                                      */
    float* d_obs;                /* [T][B][ns]  observation BEFORE the step (:91)                */
    float* d_act;                /* [T][B][na]  UNCLIPPED action (:92)                           */
    float* d_rew;                /* [T][B]                                                       */
    float* d_mean;               /* [T][B][na]  agent_infos['mean'] (log_std = theta tail)       */
    uint8_t* d_done;             /* [T][B]      done flag returned by step (incl. ts>=H, :604)   */
    int32_t* d_tpath;            /* [T][B]      0-based step index inside its path               */
    float* d_last_obs;           /* [B][ns]     state after the last step (optional, may be NULL) */
    /* ---- continuation (ABI 2; all zero / NULL = a fresh rollout starting with vec_env.reset()) ----
     * The reference's sampling loop `while n_samples < batch_size` (samplers/vectorized_sampler.py:60) runs an unknown number
     * of steps when the env terminates early (Ant).  A caller issues the steps in chunks: each further chunk resumes from the
     * d_last_* outputs of the previous one, and chunks enqueued after the stop condition was met do nothing.                   */
    int32_t t0;                  /* global index of this call's first step: Philox counters use t0 + t, so a chunked rollout
                                    draws exactly what one long call would; output tensors and the supplied-draw tensors are
                                    indexed by the LOCAL step t (row 0 of d_reset_* is unused when resuming)                */
    const float* d_init_obs;     /* [B][ns]     resume from these states instead of resetting (with d_init_ts/_model)       */
    const int32_t* d_init_ts;    /* [B]         steps already taken in each env's current path                              */
    const int32_t* d_init_model; /* [B]         cur_model_idx of each env (eps_rand, env_helpers.py:583,593)                */
    int32_t* d_last_ts;          /* [B]         outputs matching d_init_* (optional; may alias the d_init_* arrays)         */
    int32_t* d_last_model;
    const int32_t* d_stop;       /* optional device flag: if *d_stop != 0 when the call executes, nothing is computed or
                                    written (see metrpo_sampler_progress)                                                   */
    /* ---- in-launch stop rule (ABI 4; 0 / NULL = off) ----
     * stop_batch > 0: the loop condition of obtain_samples (`while n_samples < batch_size`, vectorized_sampler.py:60,104) may be
     * applied INSIDE the call: a kernel family that runs all T steps in one launch (the persistent stream-K rollout) counts the
     * samples of completed paths per step itself, starting from *d_stop_cum (the total of the steps in front of this call:
     * metrpo_sampler_progress's d_state[0]), and stops stepping behind the first step at which the total reaches stop_batch.
     * Rows beyond that step, d_last_* included, are then UNDEFINED; metrpo_sampler_progress over this call's d_done / d_tpath
     * still finds the stop step (it scans in step order and stops there).  Kernel families that launch per step ignore both fields
     * and run all T steps.                                                                                                       */
    int64_t stop_batch;
    const double* d_stop_cum;
} metrpo_rollout_args;
int32_t metrpo_rollout(metrpo_ctx* ctx, const metrpo_rollout_args* args, void* stream);
/* Which kernel family the last metrpo_rollout of this context ran on (-1 none yet; 0 thread-per-env, 1 head-per-wave fused, 2 cooperative fused, 3 step-wise
 * GEMM, 4 resident, 5 step-wise stream-K, 6 persistent stream-K, 7 step-wise GEMM with bf16 operands: metrpo_set_dyn_precision below), and -- when the shape fell off the fast dispatch table (2 x 64 nets with more heads than the
 * fused kernels hold: K > 10, Ant > 8, half-cheetah > 9, or K > 5 on a shared device; hidden widths that are neither 64 nor multiples of 256; INTEGRATION.md
 * section 9 has the table and the measured cost) -- why ("" otherwise; also printed once per context on stderr unless option QUIET is set).  The reference has one code path for every shape
 * (env_helpers.py:609-635); these two calls are how a caller learns which of this library's it got. */
int32_t metrpo_last_rollout_kernel(const metrpo_ctx* ctx);
const char* metrpo_rollout_note(const metrpo_ctx* ctx);
/* Diagnostics: the sub-form of the last metrpo_rollout on a GEMM-class (3, 5, 6, 7) or resident (4) family, as the host noted it while it enqueued the launches
 * (no device work, no synchronisation).  out[16]:
 *   [0]  family, as metrpo_last_rollout_kernel
 *   [1]  pre-step: 0 2 x 32 MFMA, 1 the same with the previous step's post merged in, 2 Humanoid MFMA3, 3 MFMA3 split (a tile per workgroup), 4 GEMM chain,
 *        5 VALU k_big_pre, 6 MFMA3 with the post merged in; -1 none (resident, fused 2 x 64 families)
 *   [2]  k_big_post's lanes per env, 32 or 64; 0 where a persistent or resident launch closes the steps
 *   [3]  stream-K mode 0 ... 3      [4] late split of the launch that carries the output layer      [5] layer 0: 0 producer, 1 k_l0_rows, 2 tile GEMM
 *   [6]  fused output tile 0, 1, 2  [7] partials of the output layer added in the closing kernel (0: the output layer was unsplit)
 *   [8]  persistent: two-block tiles     [9] persistent: closing workgroups     [10] rounds: 0 single, 1 side by side (streams / one resident grid), 2 merged
 *   [11] resident: slice width   [12] threads per workgroup   [13] post waves per workgroup   [14] rounds per launch group   [15] rotating deal
 * Everything behind [0] is 0 ([1]: -1) on the other families. */
int32_t metrpo_debug_last_rollout_launch(const metrpo_ctx* ctx, int32_t* out);

/* ---- opt-in bf16-operand dynamics forward inside metrpo_rollout (an EXTENSION: the reference computes in f32 throughout) ----
 * The f32 matrix instruction of gfx950 runs at 1/16 of the bf16 one's rate and there is no xf32 form.  The dynamics model is a residual,
 * s' = s + diff_mean + diff_std * net(...) (training.py:257): the state itself stays f32, operand rounding touches only the predicted change.
 * With METRPO_DYN_BF16 every dynamics layer l of every head computes, inside metrpo_rollout,
 *     out[b][j] = act_l( b_l[j] + sum_i bf16(in[b][i]) * bf16(W_l[i][j]) )
 *   - bf16(.) is round-to-nearest-even from f32, applied to the layer's input (the normalised, column-dropped [s, clip(a)] for layer 0, the previous
 *     layer's activations otherwise) and to the weights.  A hidden activation is rounded exactly once: the f32 value act(b + sum) is what gets rounded.
 *   - products are exact in f32; the sum is accumulated in f32 in the matrix instruction's order (v_mfma_f32_32x32x16_bf16, k ascending in steps of 16).
 *   - bias add and activation stay f32, and so does everything outside the matrix products: normalisation, the column drop, de-normalisation plus
 *     residual, head selection (all six sam_modes), reward, is_done, reset, the policy, and every Philox draw -- the same code and the same draws as under F32.
 *   - metrpo_rollout ONLY.  metrpo_step, metrpo_validation_cost, metrpo_bptt_grad*, metrpo_lbfgs_*, metrpo_dyn_train_*, metrpo_dyn_eval_losses,
 *     metrpo_model_error and metrpo_rollout_actions compute in f32 whatever the setting: the models are trained and validated in f32 and early stopping
 *     judges the policy on the f32 models; only the sampling that feeds the TRPO / VPG / PPO update runs on rounded operands.
 *   - supported exactly on the contexts whose f32 rollout runs on a step-wise GEMM family (3, 5, 6 of metrpo_last_rollout_kernel): every hidden layer
 *     >= 16 units, ns <= 64, and not a fused 2 x 64-class shape.  On any other context the setter returns METRPO_EUNSUPPORTED, metrpo_last_error names
 *     the shape, and the precision stays F32: there is no silent f32 under a bf16 label.
 *   - such a rollout reports family 7 and an empty metrpo_rollout_note.  It launches per step: stop_batch / d_stop_cum are ignored (see above); the
 *     continuation fields (t0, d_init_*, d_last_*, d_stop) work as on family 3.  The bf16 weight image is rebuilt from the context's f32 weights at
 *     the start of every such call (no cache), so metrpo_set_dynamics*, metrpo_dyn_train_step and checkpoint loads are always seen.
 * The setter takes effect at the next metrpo_rollout; the default is METRPO_DYN_F32, under which nothing changes.  Unknown value: METRPO_EINVAL. */
typedef enum { METRPO_DYN_F32 = 0, METRPO_DYN_BF16 = 1 } metrpo_dyn_precision;
int32_t metrpo_set_dyn_precision(metrpo_ctx* ctx, int32_t precision);
int32_t metrpo_get_dyn_precision(const metrpo_ctx* ctx);

/* Loop condition of obtain_samples (samplers/vectorized_sampler.py:60,104): n_samples counts the samples of COMPLETED paths
 * only and is tested once per time step.  For the chunk [t0, t0+T) just rolled out (d_done, d_tpath [T][B]) this adds each
 * step's completed-path samples, sum_b done[t][b] * (tpath[t][b] + 1), to d_state[0] in step order; the first step at which
 * the total reaches batch_size is written to d_state[1] (global index, -1 until then) and *d_stop is set to 1.  A chunk
 * processed while *d_stop is already 1 changes nothing.  d_state [2] float64 (caller initialises {0, -1}), d_counts [T]
 * float64 scratch, d_stop int32 (caller zeroes).  The caller keeps steps 0..d_state[1]; paths still open there are dropped
 * by metrpo_gae's valid mask, as the reference drops them. */
int32_t metrpo_sampler_progress(metrpo_ctx* ctx, const uint8_t* d_done, const int32_t* d_tpath, int32_t T, int32_t B,
                                int32_t t0, int64_t batch_size, double* d_counts, double* d_state, int32_t* d_stop,
                                void* stream);

/* build_policy_graph forward (model_based_rl.py:106-151): per model i, deterministic clipped
 * policy, model i for the whole trajectory, cost_i = sum_t gamma^t mean_b cost (Ant: masked by the
 * running dones, :134-137).  d_s0 [Bv][ns] -> d_costs [K] (float64). */
int32_t metrpo_validation_cost(metrpo_ctx* ctx, const float* d_s0, int32_t Bv, int32_t T, double gamma,
                               double* d_costs, void* stream);

/* ---- BaseSampler.process_samples (samplers/base.py:48-104) -------------------------------- */
/* Per env column reverse scan: V = [rllab] LinearFeatureBaseline.predict (zeros if d_coeffs NULL),
 * delta = r + g*V' - V, adv = discount_cumsum(delta, g*lam), ret = discount_cumsum(r, g) (:57-64),
 * restarting at every done; samples of a trailing unfinished path get valid=0 (the reference
 * drops such paths, vectorized_sampler.py:60,104).  d_coeffs [2*ns+4] float64 or NULL.
 * d_stats [3] float64 is ACCUMULATED (caller zeroes): sum(adv), sum(adv^2), count over valid. */
int32_t metrpo_gae(metrpo_ctx* ctx, const float* d_obs, const float* d_rew, const uint8_t* d_done,
                   const int32_t* d_tpath, int32_t T, int32_t B, const double* d_coeffs, double gamma,
                   double lam, float* d_adv, float* d_ret, uint8_t* d_valid, double* d_stats, void* stream);
/* Opening launch of process_samples (samplers/base.py:48-104): d_old_log_std [na] <- max(log_std of the ctx policy, log 1e-6) -- the
 * agent_infos['log_std'] every sample of the batch carries ([rllab] GaussianMLPPolicy.dist_info, min_std = 1e-6; vectorized_sampler.py:72-77) -- and
 * d_acc [n_acc] float64 <- 0 (the accumulators metrpo_gae / metrpo_baseline_gram add into).  Either pointer may be NULL.  One launch, stream-ordered:
 * call it after the rollout was enqueued and before the policy is updated. */
int32_t metrpo_process_begin(metrpo_ctx* ctx, float* d_old_log_std, double* d_acc, int64_t n_acc, void* stream);
/* [rllab] util.center_advantages (base.py:82-83): adv <- (adv-mean)/(std+1e-8) over valid samples,
 * mean/std from d_stats (after the caller all-reduced it across ranks). */
int32_t metrpo_center_advantages(metrpo_ctx* ctx, float* d_adv, const uint8_t* d_valid, int64_t N,
                                 const double* d_stats, void* stream);
/* [rllab] LinearFeatureBaseline.fit normal equations (base.py:164-167): ACCUMULATES
 * d_AtA [F][F] += F^T F and d_Aty [F] += F^T ret over valid samples, F = 2*ns+4 features
 * [o, o^2, t/100, (t/100)^2, (t/100)^3, 1], o = clip(obs,-10,10).  float64. The F x F solve stays
 * with the caller (after its all-reduce). */
int32_t metrpo_baseline_gram(metrpo_ctx* ctx, const float* d_obs, const float* d_ret, const int32_t* d_tpath,
                             const uint8_t* d_valid, int64_t N, double* d_AtA, double* d_Aty, void* stream);
/* The solve of that fit, on the device ([rllab] linear_feature_baseline.py fit: lstsq(F^T F + reg I, F^T ret), reg x 10 while the
 * solution contains a NaN, at most 5 attempts): d_coeffs [F] float64 from d_AtA / d_Aty (summed over the ranks by the caller).
 * Stream-ordered, no host round trip: the coefficients go straight into the next metrpo_gae.  The system is square and nonsingular
 * (symmetric positive definite) for reg > 0, so elimination in the natural order returns lstsq's solution (to float64 conditioning). */
int32_t metrpo_baseline_solve(metrpo_ctx* ctx, const double* d_AtA, const double* d_Aty, double reg_coeff, double* d_coeffs, void* stream);

/* ---- NPO/TRPO update (algos/npo.py:68-111, algos/trpo.py:18-20; [rllab] ConjugateGradientOptimizer) */
typedef struct {
    const float* d_obs;          /* [N][ns]                                                      */
    const float* d_act;          /* [N][na] unclipped actions                                    */
    const float* d_adv;          /* [N]                                                          */
    const float* d_old_mean;     /* [N][na] agent_infos['mean']                                  */
    const float* d_old_log_std;  /* [N][na] (stride na) or [na] broadcast (stride 0)             */
    int32_t old_log_std_stride;
    const uint8_t* d_valid;      /* [N] or NULL (= all valid)                                    */
    int64_t N;                   /* local samples                                                */
    double inv_n_global;         /* 1 / (valid samples over ALL ranks): partial results are
                                    pre-scaled so that a sum all-reduce yields the global mean   */
} metrpo_batch;

/* f_loss + f_grad of the surrogate (npo.py:75): d_out[0] = loss partial, d_out[1..P] = gradient
 * partial (float64, this rank's share).  theta = the ctx policy. */
int32_t metrpo_loss_grad(metrpo_ctx* ctx, const metrpo_batch* batch, double* d_out, void* stream);
/* [rllab] PerlmutterHvp f_Hx_plain: Hessian(mean_kl) . v WITHOUT the reg_coeff*v term (added by the
 * caller after its all-reduce).  d_v [P] float64 in, d_hv [P] float64 out (this rank's share). */
int32_t metrpo_fvp(metrpo_ctx* ctx, const metrpo_batch* batch, const double* d_v, double* d_hv, void* stream);
/* f_loss_constraint at d_theta (float32 [P], or NULL = ctx policy): d_out[0]=loss, d_out[1]=mean_kl
 * partials (float64). */
int32_t metrpo_loss_kl(metrpo_ctx* ctx, const metrpo_batch* batch, const float* d_theta, double* d_out,
                       void* stream);

/* ---- VPG update (algos/vpg.py:88 surr_obj = -mean(logli * adv), :26-33 FirstOrderOptimizer(batch_size=None, max_epochs=1);
 * training.py:337-352).  logli = DiagonalGaussian.log_likelihood_sym of the unclipped stored action under the ctx policy (log_std
 * clamped at log(1e-6) as in the TRPO kernels); no likelihood ratio: d_old_mean / d_old_log_std of the batch may be NULL. */
/* f_loss + gradient of surr_obj: d_out[0] = loss partial, d_out[1..P] = gradient partial (log_std slots included), float64, this
 * rank's share -- the layout of metrpo_loss_grad, for a host-driven all-reduce (metrpo_allreduce_fn, gloo) and metrpo_policy_adam_step. */
int32_t metrpo_vpg_loss_grad(metrpo_ctx* ctx, const metrpo_batch* batch, double* d_out, void* stream);
typedef struct {
    double lr, beta1, beta2, eps;    /* tf.train.AdamOptimizer(learning_rate=1e-3): 1e-3, 0.9, 0.999, 1e-8 (FirstOrderOptimizer, vpg.py:26-33) */
} metrpo_vpg_params;
/* One optimize_policy of VPG (vpg.py:100-118): ONE Adam step on the whole batch's gradient, every policy parameter incl. log_std, no
 * clipping.  The optimizer state is the ctx policy Adam state (metrpo_get_policy_adam / metrpo_set_policy_adam; not reset here,
 * model_based_rl.py:398-405).  Two launches on the stream, no synchronisation: the gradient kernel, then the reduction whose blocks
 * apply the step to the columns they reduced (with the ranks' sum when a one-shot transport is attached; with an RCCL communicator
 * the all-reduce and a stand-alone step follow the reduction).  d_loss (optional, 1 double) = the loss at the entry theta. */
int32_t metrpo_vpg_update(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_vpg_params* params, double* d_loss, void* stream);

/* ---- PPO update (algos/ppo.py:107-119).  With lr_i = exp(logli_theta(a_i | o_i) - logli_old(a_i | o_i)) (ppo.py:107; logli as for VPG, the old
 * distribution is the batch's d_old_mean / d_old_log_std, which must be there: NULL is METRPO_EINVAL):
 *     loss = -mean_i min(lr_i A_i, clip(lr_i, 1 - clip_lr, 1 + clip_lr) A_i) - entropy_bonus_coeff * mean_i H_i        (ppo.py:112-119)
 * H = sum_j log_std_j + na / 2 (1 + log 2 pi) of the clamped log_std (ppo.py:109), means over the valid samples (inv_n_global).  The gradient is
 * tf.minimum's / tf.clip_by_value's: a sample contributes -A_i lr_i grad(logli_i) / N when lr_i A_i <= clip(lr_i) A_i (ties: the unclipped
 * branch) and nothing otherwise; the entropy term adds -entropy_bonus_coeff on every unclamped log_std slot.  use_kl_penalty (ppo.py:120-121):
 * the block below.  The optimiser ppo.py:61-62 names (an AdamOptimizer the file never imports or defines) is stated here: n_epochs full-batch
 * tf.train.AdamOptimizer steps, no clipping, every policy parameter incl. log_std. */
typedef struct {
    double clip_lr, entropy_bonus_coeff;   /* ppo.py:19, :24: 0.3, 0 */
    double lr, beta1, beta2, eps;          /* the Adam epochs of metrpo_ppo_update (1e-3, 0.9, 0.999, 1e-8); not read by metrpo_ppo_loss_grad */
} metrpo_ppo_params;
/* Loss and gradient of ppo.py:119's clipped_surr_pen_loss at the ctx policy: d_out [1 + P] float64 in metrpo_loss_grad's layout.  The surrogate part
 * is this rank's share; the entropy term is per parameter and is added whole by every call -- a host-driven all-reduce over W ranks passes
 * entropy_bonus_coeff / W. */
int32_t metrpo_ppo_loss_grad(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_ppo_params* params, double* d_out, void* stream);
/* One optimize_policy of PPO (ppo.py:157-177, the optimizer.optimize call): n_epochs x (gradient kernel + reduction whose blocks add the entropy term
 * and apply the Adam step to the columns they reduced), the old distribution fixed while theta moves.  No synchronisation and no host read between
 * the epochs.  The optimizer state is the ctx policy Adam state, not reset here (as metrpo_vpg_update).  Sharded: each epoch's reduction carries the
 * one-shot exchange in its tail; with an RCCL communicator (and on the GEMM path) the all-reduce and a stand-alone step follow the reduction.
 * d_losses (optional, n_epochs doubles): d_losses[e] = the loss at the theta entering epoch e. */
int32_t metrpo_ppo_update(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_ppo_params* params, int32_t n_epochs, double* d_losses, void* stream);

/* ---- PPO's KL penalty (use_kl_penalty, ppo.py:120-121).  With beta = kl_penalty, delta = step_size (ppo.py:34: 0.01) and mean_kl = the mean over the valid
 * samples (inv_n_global) of dist.kl_sym(old, new) -- the quantity metrpo_loss_kl returns in d_out[1], with the same log_std clamp:
 *     loss = [the PPO loss above] + beta * max(0, mean_kl - delta)
 * Gate: tf.maximum's gradient (MaximumGrad) sends a tie to the constant 0., so the penalty contributes to the gradient iff mean_kl - delta > 0, strictly.
 * The gate is decided on the float64 REDUCED mean_kl (one device cell every kernel of the launch reads), never on a sample's or a rank's float32 share.
 * Gate open: sample i adds beta * inv_n_global * d kl_i / d theta to the clipped surrogate's seed; with sigma = exp(clamped log_std)
 *     d kl_i / d mean_j = (mean_j - old_mean_j) / sigma_j^2,    d kl_i / d log_std_j = 1 - (sigma_old_j^2 + (old_mean_j - mean_j)^2) / sigma_j^2,
 * the log_std gradient being zero on a clamped slot like every other term; a sample whose surrogate is clipped still carries its KL gradient.  The loss
 * term is accumulated per sample as beta * inv_n_global * (kl_i - delta), which sums to beta * (mean_kl - delta) over all ranks' valid samples.
 * Gate closed: loss and gradient are metrpo_ppo_loss_grad's, bit for bit.
 * mean_kl is GLOBAL: over all ranks' valid samples, summed before the gate is taken.  Rank sums: the surrogate and the KL parts of d_out are this rank's
 * share (no / W rule for the penalty); the entropy term keeps metrpo_ppo_loss_grad's convention; d_out[0] summed over the ranks is the global loss. */
typedef struct { double kl_penalty, step_size; } metrpo_ppo_kl_params;   /* ppo.py:27 initial_kl_penalty = 1 (the caller's current value), :34 step_size = 0.01 */
/* metrpo_ppo_loss_grad with the penalty.  d_mean_kl: device pointer to the global mean KL at the ctx theta (one double; a host-driven all-reduce sums
 * metrpo_loss_kl's d_out[1] over the ranks first), or NULL: computed by the call (the launches of metrpo_loss_kl at the ctx theta in front of the gradient
 * launch, summed over the ranks by an attached communicator).  kl_penalty < 0, a non-finite kl_penalty or step_size and a NULL old distribution are
 * METRPO_EINVAL. */
int32_t metrpo_ppo_kl_loss_grad(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_ppo_params* params, const metrpo_ppo_kl_params* kl,
                                const double* d_mean_kl, double* d_out, void* stream);
/* metrpo_ppo_update with the penalty: per epoch the loss + KL launch and its reduction at the theta entering the epoch (into a ctx-owned float64 pair;
 * sharded with an attached communicator the reduction carries the exchange, as the line-search trials do), the gradient launch that reads that pair and
 * takes the gate itself, and the reduction with entropy term and Adam step.  No synchronisation and no host read between the epochs; on the RCCL / GEMM
 * path metrpo_ppo_update's stand-alone step sequence applies unchanged.  d_losses (optional, n_epochs doubles) as there, penalty included; d_mean_kls
 * (optional, n_epochs doubles): the global mean KL at the theta entering each epoch.  An open TRPO update is METRPO_ESTATE. */
int32_t metrpo_ppo_kl_update(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_ppo_params* params, const metrpo_ppo_kl_params* kl, int32_t n_epochs,
                             double* d_losses, double* d_mean_kls, void* stream);

/* ---- multi-GPU: one process and one ctx per GPU, the env batch B sharded over the ranks.  The only exchanges on
 * the path are sum all-reduces of small float64 vectors.  Attach an RCCL communicator to the ctx and metrpo_trpo_update issues
 * its all-reduces itself (ncclAllReduce on the caller's stream, in-place, float64); the reference has no counterpart (it is a
 * single-process TF session, utils.py:229-232).  Bootstrap: rank 0 calls metrpo_comm_get_unique_id and ships the 128 bytes to
 * the other ranks by any side channel (bench.py: a torch.distributed broadcast); then EVERY rank calls metrpo_comm_init
 * (collective, blocks until all ranks arrive).  librccl is loaded on first use. */
#define METRPO_COMM_ID_BYTES 128
int32_t metrpo_comm_get_unique_id(void* id_out /* METRPO_COMM_ID_BYTES */);
int32_t metrpo_comm_init(metrpo_ctx* ctx, const void* id /* METRPO_COMM_ID_BYTES */, int32_t world, int32_t rank);
int32_t metrpo_comm_destroy(metrpo_ctx* ctx);
/* in-place sum over the ranks of the attached communicator, stream-ordered (advantage statistics, baseline normal equations) */
int32_t metrpo_allreduce_sum_f64(metrpo_ctx* ctx, double* d_buf, int64_t count, void* stream);

/* One-shot direct all-reduce (SURVEY.md 8e "collective choice on xGMI"): the exchanges above are latency-bound, and xGMI connects
 * every pair of GPUs directly, so each rank writes its vector straight into a slot of every peer's receive region (device memory
 * exported with hipIpcGetMemHandle and mapped by the peers) and adds the slots of its own region in rank order -- one fabric
 * traversal, deterministic, bit-identical on every rank, no host in the loop.  Inside metrpo_trpo_update the exchange rides in the
 * tail of the kernel that reduces the per-block partial rows, in front of the CG vector step.  Takes precedence over an RCCL
 * communicator when both are attached.  World size <= 8 (one node); the ranks may also share one GPU (tests).
 *   every rank: metrpo_comm_ipc_export(ctx, blob) -> all-gather the blobs by any side channel (Comm.attach_engine: torch.distributed)
 *   every rank: metrpo_comm_ipc_attach(ctx, blobs[world], world, rank)
 * A rank that never arrives makes the waiting kernels give up after METRPO_XCHG_TIMEOUT_MS (default 20 000) and the next
 * metrpo_trpo_update / metrpo_comm_check returns METRPO_EHIP instead of hanging the GPU. */
#define METRPO_COMM_IPC_BLOB_BYTES 128
int32_t metrpo_comm_ipc_export(metrpo_ctx* ctx, void* blob_out /* METRPO_COMM_IPC_BLOB_BYTES */);
int32_t metrpo_comm_ipc_attach(metrpo_ctx* ctx, const void* blobs /* world x METRPO_COMM_IPC_BLOB_BYTES */, int32_t world, int32_t rank);
int32_t metrpo_comm_ipc_detach(metrpo_ctx* ctx);
/* time limit of a waiting exchange kernel from now on (attach sets METRPO_XCHG_TIMEOUT_MS or 20 000) */
int32_t metrpo_comm_set_timeout_ms(metrpo_ctx* ctx, int64_t ms);
/* 0 = single rank, 1 = RCCL communicator, 2 = one-shot direct all-reduce */
int32_t metrpo_comm_transport(const metrpo_ctx* ctx);
/* synchronises `stream`; METRPO_EHIP if an exchange timed out since the transport was attached, or if a tile hand-over of the
 * cooperative rollout kernel gave up waiting (both are sticky device-side error cells, also checked by metrpo_trpo_update) */
int32_t metrpo_comm_check(metrpo_ctx* ctx, void* stream);

/* all-reduce(sum) hook for sharded runs WITHOUT an attached communicator (e.g. a gloo group in the CPU-side tests; takes
 * precedence over the communicator when both are given): called on the host while enqueuing, must reduce `count`
 * float64 values at device pointer d_buf in place across ranks, ordered after prior work on
 * `stream` and before later work on it.  NULL = single rank. */
typedef int32_t (*metrpo_allreduce_fn)(void* user, double* d_buf, int64_t count, void* stream);

typedef struct {
    double max_kl;               /* step_size (params trpo.step_size, npo.py:22,88)              */
    int32_t cg_iters;            /* 10                                                           */
    double reg_coeff;            /* 1e-5                                                         */
    double backtrack_ratio;      /* 0.8                                                          */
    int32_t max_backtracks;      /* 15                                                           */
    int32_t accept_violation;    /* 0                                                            */
    double residual_tol;         /* 1e-10 ([rllab] krylov.cg)                                    */
    metrpo_allreduce_fn allreduce;
    void* allreduce_user;
    int32_t explicit_final_hvp;  /* 0 (default): d.(H d) of the step scale is taken from the CG recurrence (H d = g - r, the
                                    identity krylov.cg maintains); 1: evaluate f_Hx(descent_direction) once more, as [rllab]
                                    ConjugateGradientOptimizer.optimize literally does.  Same value up to float32 rounding   */
} metrpo_trpo_params;

typedef struct {                 /* host-side diagnostics of one optimize() call                 */
    double loss_before, loss, kl, beta;
    int32_t n_backtrack, accepted, cg_iters_run;
} metrpo_trpo_diag;

/* One [rllab] ConjugateGradientOptimizer.optimize call (reached from algos/npo.py:111): loss_before,
 * flat gradient, cg_iters x FVP in krylov.cg, step scale, backtracking line search; on return the
 * ctx policy holds theta_new (or theta_prev if rejected).  SYNCHRONISES the stream once per
 * line-search trial (the accept test is a host decision in the reference too).
 * Optional parity outputs (may be NULL): d_g_out, d_dir_out [P] float64 (gradient, CG direction). */
int32_t metrpo_trpo_update(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_trpo_params* params,
                           metrpo_trpo_diag* diag, double* d_g_out, double* d_dir_out, void* stream);

/* The same optimize() call (algos/npo.py:111) in two halves, for callers that want to keep enqueuing (the next iteration's
 * obtain_samples, model_based_rl.py:1171-1180) while the line search is being decided.
 *   _begin  gradient, CG solve and the first `spec_trials` (>= 1) trials of the backtracking loop; the loop's break test and the
 *           acceptance rule that follows it are evaluated ON THE DEVICE in the tail of each trial's reduction, an accepted trial's
 *           theta becomes the ctx policy at once, later speculative trials leave without work.  Does NOT synchronise; `batch`
 *           must stay valid until _end.  Launches that follow on `stream` see theta_new if one of these trials was accepted.
 *   _end    waits for _begin's work (not for what was enqueued after it), fills `diag`, and -- only if the search did not stop
 *           within the speculative trials -- runs trials spec_trials, spec_trials+1, ... exactly as metrpo_trpo_update does.
 *           *late_out (may be NULL) = 1 if the policy changed inside _end (accepted at one of those later trials): work enqueued
 *           between the two calls used theta_prev and has to be redone by the caller; 0 otherwise.
 * Results are those of metrpo_trpo_update bit for bit.  With a host all-reduce callback, an RCCL transport or the GEMM update path
 * the accept test cannot run on the device: _begin then performs the whole update synchronously and _end returns its diagnostics. */
int32_t metrpo_trpo_update_begin(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_trpo_params* params, int32_t spec_trials,
                                 double* d_g_out, double* d_dir_out, void* stream);
int32_t metrpo_trpo_update_end(metrpo_ctx* ctx, metrpo_trpo_diag* diag, int32_t* late_out, void* stream);

/* ---- subsampled Fisher-vector products ([rllab] ConjugateGradientOptimizer(subsample_factor < 1).optimize):
 *         n = len(inputs[0]);  inds = np.random.choice(n, int(n * subsample_factor), replace=False)
 *         subsample_inputs = tuple(x[inds] for x in inputs)
 *     loss_before, flat_g and every f_loss_constraint trial use `inputs`; Hx = f_Hx_plain(subsample_inputs) + reg_coeff * x is what krylov.cg and
 *     descent_direction.dot(Hx(descent_direction)) see, the mean KL inside it being the mean over the subsample; one draw per optimize call.
 * All additions to ABI 4: no struct of this header changes, METRPO_ABI_VERSION stays. */
/* The gather x[inds] on the device.  d_idx [m] int32 row indices into `batch` (any order, duplicates allowed); rows are gathered in index order into
 * compact arrays in a ctx-owned workspace and *out is filled to describe them: d_obs [m][ns], d_old_mean [m][na] (NULL if the source's is), d_old_log_std
 * [m][na] for a per-sample source (stride na) -- a broadcast source (stride 0) stays the CALLER's pointer, not expanded --, d_valid [m] (NULL if the
 * source's is), N = m, inv_n_global as given (the sub-batch's: 1 / its valid samples over all ranks; the caller may overwrite the field of *out later).
 * d_act and d_adv of *out are NULL: these are the fields the Fisher-vector-product kernels and the old distribution need; the sub-batch serves
 * metrpo_fvp and the fvp_batch argument below, not the loss entry points.
 * The workspace, and with it *out, stays valid until the next metrpo_subsample_batch on this ctx or metrpo_destroy (it grows by the rule of the
 * Conventions: an outgrown buffer is kept, never freed here, so launches already enqueued on it stay correct).
 * d_valid_count (optional, one device double): the number of valid gathered rows is ADDED to it (caller zeroes; a sharded caller all-reduces it
 * with metrpo_allreduce_sum_f64 / its own transport to obtain the denominator of inv_n_global).
 * An index outside [0, N) is clamped into the batch -- no read outside it -- and raises a sticky device cell: the next metrpo_trpo_update_fvp on this
 * ctx (after it completed) or metrpo_comm_check returns METRPO_EINVAL once.  Stream-ordered, no synchronisation.  N and m below 2^31. */
int32_t metrpo_subsample_batch(metrpo_ctx* ctx, const metrpo_batch* batch, const int32_t* d_idx, int64_t m, double inv_n_global, metrpo_batch* out,
                               double* d_valid_count, void* stream);
/* metrpo_trpo_update / metrpo_trpo_update_begin with a separate batch for Hx: the cg_iters Fisher-vector products, and the explicit final one under
 * explicit_final_hvp, run on fvp_batch (their partials pre-scaled by ITS inv_n_global); gradient, loss_before and the line search run on batch.
 * The activation caches a whole-batch solve keeps between its gradient launch and its products belong to `batch`: with a separate fvp_batch the
 * products run uncached and nothing is cached.  fvp_batch NULL, == batch, or equal to it field by field: exactly the launches
 * and results of metrpo_trpo_update / _begin.  A _begin of this form is closed by metrpo_trpo_update_end like any other (its trials see `batch` only);
 * fvp_batch must stay valid until the launches of _begin have run (a metrpo_subsample_batch workspace does: it changes only in stream order). */
int32_t metrpo_trpo_update_fvp(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_batch* fvp_batch, const metrpo_trpo_params* params,
                               metrpo_trpo_diag* diag, double* d_g_out, double* d_dir_out, void* stream);
int32_t metrpo_trpo_update_fvp_begin(metrpo_ctx* ctx, const metrpo_batch* batch, const metrpo_batch* fvp_batch, const metrpo_trpo_params* params,
                                     int32_t spec_trials, double* d_g_out, double* d_dir_out, void* stream);

/* ---- "next" rows of the scope table: ensemble dynamics training + normaliser statistics ---- */
typedef struct {
    double lr;                   /* dynamics_opt_params.learning_rate["scratch"|"refine"] (model_based_rl.py:905-918)      */
    double beta1, beta2, eps;    /* tf.train.AdamOptimizer defaults 0.9, 0.999, 1e-8 (:162)                                */
    double reg_constant;         /* dynamics_model.regularization.constant (training.py:271-282); SGD(lr) on it (:169-177) */
    int32_t batch_size;          /* dynamics_opt_params.batch_size: rows PER MODEL                                         */
} metrpo_train_params;

/* sess.run(dynamics_adam_init) (model_based_rl.py:912-918): zero the Adam moments and the step count. */
int32_t metrpo_dyn_train_reset(metrpo_ctx* ctx, void* stream);
/* The dynamics optimizer's state (the adam_<scope> slots of model_based_rl.py:154-183, saved by tf.train.Saver() :495):
 * d_m, d_v [K][dyn_param_count] each, in metrpo_get_dynamics' layout; t = Adam steps taken (the next step uses t + 1).
 * Before the first train step a get returns zeros and t = 0; a set allocates the state as that step would.  The copies are
 * asynchronous on `stream` (no device-wide sync); the one exception is a set before the first step, whose one-time
 * allocation and zero fill (hipMalloc + hipMemset, as in that first step) synchronise.  METRPO_EINVAL for a NULL ctx or
 * pointer, or t < 0. */
int32_t metrpo_get_dyn_adam(metrpo_ctx* ctx, float* d_m, float* d_v, int64_t* t_out, void* stream);
int32_t metrpo_set_dyn_adam(metrpo_ctx* ctx, const float* d_m, const float* d_v, int64_t t, void* stream);
/* One sess.run([dynamics_opt_op, dynamics_loss]) (model_based_rl.py:961-971; loss graph :39-71; optimizers :154-183).
 * d_x [batch_size*K][ns+na] = (state, action), d_y [batch_size*K][ns] = next state; the block is consumed as the
 * reference's np.reshape(x_batch, (batch_size, -1)) + utils.get_ith_tensor: model i trains on rows i, K+i, 2K+i, ...
 * The ctx dynamics weights are updated in place.  d_loss_out [K] float64 (optional): per-model loss BEFORE the update. */
int32_t metrpo_dyn_train_step(metrpo_ctx* ctx, const float* d_x, const float* d_y, const metrpo_train_params* params,
                              double* d_loss_out, void* stream);
/* dynamics_losses on np.tile(validation, n_models) (model_based_rl.py:933-945, 977-983): every model on all n rows.
 * d_losses [K] float64 = prediction loss + regulariser per model. */
int32_t metrpo_dyn_eval_losses(metrpo_ctx* ctx, const float* d_x, const float* d_y, int64_t n, double reg_constant,
                               double* d_losses, void* stream);
/* per-model savers (model_based_rl.py:499-509, 927-930, 1002-1004; recover_weights :871-878): read all / write one model. */
int32_t metrpo_get_dynamics(metrpo_ctx* ctx, float* d_params_out, void* stream);
int32_t metrpo_set_dynamics_model(metrpo_ctx* ctx, int32_t model, const float* d_params_model, void* stream);
/* RunningMeanStd read-outs changed (after input_rms.update / output_rms.update, model_based_rl.py:834-835). COPIES. */
int32_t metrpo_set_normalizers(metrpo_ctx* ctx, const float* d_in_mean, const float* d_in_std, const float* d_diff_mean,
                               const float* d_diff_std, void* stream);
/* RunningMeanStd.update (running_mean_std.py:35-42): d_sum[dim] += sum_rows x, d_sumsq[dim] += sum_rows x^2 (float64);
 * count += n, mean and the 0.1-floored std are the caller's (running_mean_std.py:22-27). */
int32_t metrpo_rms_accumulate(metrpo_ctx* ctx, const float* d_x, int64_t n, int32_t dim, double* d_sum, double* d_sumsq,
                              void* stream);

/* ---- "next" row of the scope table: BPTT policy update ('bptt' branch, model_based_rl.py:1181-1187) ---- */
/* Gradient of training_policy_cost = mean_i policy_costs[i] (model_based_rl.py:365) w.r.t. the policy parameters through the
 * unrolled graph of build_policy_graph (:106-151): x <- d_init [B][ns]; T times u = clip(policy_mean(x)), x' = model_i(x, u),
 * cost_i += gamma^t * cost_tf(x, u, x') (Ant: masked by the running `dones`).  `stochastic` is 0 (the 'bptt' branch).
 * d_costs [K] float64 (optional) = policy_costs[i] (same values as metrpo_validation_cost); d_grad [P] float64, log_std slots 0. */
int32_t metrpo_bptt_grad(metrpo_ctx* ctx, const float* d_init, int32_t B, int32_t T, double gamma, double* d_costs,
                         double* d_grad, void* stream);
/* 'bptt-stochastic' branch (model_based_rl.py:1188-1196): metrpo_bptt_grad with u = clip(mean + eps*exp(log_std)) (training.py:115-116,
 * model_based_rl.py:128), eps ~ N(0, 1) independently for every (model i, step t, env b, action d); exp acts on the raw log_std parameter.
 * d_noise [K][T][B][na] float32 (parity mode) or NULL: Philox4x32-10 with key = seed, counter (b, i, t, 4<<16 | d/4), Box-Muller of the
 * block = eps of action dims 4(d/4) .. 4(d/4)+3 (csrc/device_common.h, RNG_BPTT).  Both sweeps see the same eps.
 * d_costs [K] f64 (optional) = the stochastic rollout's policy_costs; d_grad [P] f64 incl. the log_std slots
 * (sum over i, t, b of dcost/du_pre * eps * exp(log_std), float64 in a fixed order);
 * d_n_saturates [B][na] int32 (optional) = sum over models and steps of |u| == 1 (model_based_rl.py:129). */
int32_t metrpo_bptt_grad_stochastic(metrpo_ctx* ctx, const float* d_init, int32_t B, int32_t T, double gamma,
                                    const float* d_noise, uint64_t seed, double* d_costs, double* d_grad,
                                    int32_t* d_n_saturates, void* stream);
/* sess.run(policy_adam_init) (model_based_rl.py:202-204): zero the policy optimizer's moments and step count. */
int32_t metrpo_policy_adam_reset(metrpo_ctx* ctx, void* stream);
/* The policy optimizer's state (adam_<policy scope> of get_policy_optimizer, model_based_rl.py:186-204): d_m, d_v [policy_param_count]
 * each, in metrpo_get_policy's layout (log_std slots included); t as for metrpo_get_dyn_adam.  Same zero-before-first-step,
 * allocation, stream and status rules as metrpo_get_dyn_adam / metrpo_set_dyn_adam; t must also fit an int32. */
int32_t metrpo_get_policy_adam(metrpo_ctx* ctx, float* d_m, float* d_v, int64_t* t_out, void* stream);
int32_t metrpo_set_policy_adam(metrpo_ctx* ctx, const float* d_m, const float* d_v, int64_t t, void* stream);
/* policy_opt_op (get_policy_optimizer, model_based_rl.py:186-195): tf.clip_by_norm(grad, clip_val) per VARIABLE (W_l, b_l;
 * utils.py:262-276; clip_val <= 0: none) then tf.train.AdamOptimizer(lr).apply_gradients on the ctx policy parameters. */
int32_t metrpo_policy_adam_step(metrpo_ctx* ctx, const double* d_grad, double lr, double beta1, double beta2, double eps,
                                double clip_val, void* stream);

/* ---- 'l-bfgs' policy update (model_based_rl.py:391-398, :1197-1202): ScipyOptimizerInterface(training_policy_cost, method='L-BFGS-B')
 * with scipy's defaults, run on the device.  L-BFGS-B 3.0 on an unbounded problem (nbd = 0) as scipy's minimize drives it, by reverse
 * communication: each call consumes f and g at the last requested point and writes the next point to evaluate plus a task code in scipy's
 * (task[0], task[1]) numbering (_lbfgsb_py.py status_messages / task_messages): (3, 0) FG = evaluate d_x_eval next; (4, 401) / (4, 402)
 * CONVERGENCE; (5, 504) / (5, 502) STOP at maxiter / maxfun (checked at each new iterate, as scipy's wrapper does); (8, 0) ABNORMAL (line
 * search failed with no stored pair).  Once the task is not FG the state is frozen and d_x_eval holds the last accepted iterate.
 * State (float64 x, g, d, the start of the search, the S / Y ring of m pairs, the line search's scalars) is ctx-owned device memory; one
 * single-workgroup launch per call, stream-ordered, no synchronisation. */
typedef struct {
    int32_t m, maxls, maxiter, maxfun;   /* scipy: maxcor 10, maxls 20, maxiter 15000, maxfun 15000 */
    double ftol, gtol;                   /* scipy: 2.220446049250313e-09 (factr = ftol / eps = 1e7), 1e-5 */
    int32_t lookahead;                   /* metrpo_lbfgs_policy: evaluations kept in flight ahead of the host's read of a task (1..16; 2) */
    int32_t round_f32;                   /* metrpo_lbfgs_policy: f and g rounded to float32 before the step (TF's float32 loss; 1) */
} metrpo_lbfgs_opts;
typedef struct {
    double fun;                          /* f of the last evaluation (scipy's OptimizeResult.fun) */
    int32_t nit, nfev;                   /* iterations, evaluations (a point equal to the last one evaluated is not evaluated again) */
    int32_t status;                      /* 0 converged, 1 maxiter / maxfun reached, 2 abnormal (scipy's warnflag) */
    int32_t task, task_code;             /* scipy's task[0], task[1] */
    int32_t pad_;
} metrpo_lbfgs_result;
/* Open a minimisation of n variables at d_x0 [n] float64; d_x_eval [n] <- x0 (the first point to evaluate).  m, maxls > 0, n > 0. */
int32_t metrpo_lbfgs_begin(metrpo_ctx* ctx, int32_t n, const double* d_x0, const metrpo_lbfgs_opts* opts, double* d_x_eval, void* stream);
/* One step on f = *d_f and g = d_g [n] at the last requested point: d_x_eval [n] <- the next point, d_task [2] <- the task. */
int32_t metrpo_lbfgs_iterate(metrpo_ctx* ctx, const double* d_f, const double* d_g, double* d_x_eval, int32_t* d_task, void* stream);
/* The state of the open minimisation as a result (fun = f of the last evaluation, nit, nfev, status, task); synchronises `stream`. */
int32_t metrpo_lbfgs_get_result(metrpo_ctx* ctx, metrpo_lbfgs_result* out, void* stream);
/* The 'l-bfgs' branch: x0 = float64(policy theta); each evaluation is metrpo_bptt_grad's cost and gradient at float32(x) on d_init
 * [B][ns], f = mean over the K models (rounded to float32 with round_f32, as is g), then one step whose float32(x) goes straight into
 * the ctx policy.  The host reads only the published task word of each step, `lookahead` evaluations behind the device.  On exit the
 * policy is float32(last accepted iterate); the policy Adam state is untouched.  Synchronises `stream` (a bounded wait that surfaces a
 * device fault); METRPO_ESTATE while a TRPO update is open; n must be the policy's parameter count (log_std slots have gradient 0). */
int32_t metrpo_lbfgs_policy(metrpo_ctx* ctx, const float* d_init, int32_t B, int32_t T, double gamma, const metrpo_lbfgs_opts* opts,
                            metrpo_lbfgs_result* out, void* stream);

/* ---- multi-horizon open-loop prediction error of the dynamics ensemble (env_helpers.py:96-172 evaluate_model_predictions, :175-269
 * get_error_distribution; call sites model_based_rl.py:619-651).  Additions to ABI 4: no struct above changes, METRPO_ABI_VERSION stays.
 * Recorded real trajectories: d_Os [n][T+1][ns] observations, d_As [n][T][na] actions as recorded (unclipped), d_Rs [n][T] rewards, fp32 on the device.
 * A WINDOW is a start (i, t), t in [0, T); the batch has W = n * T of them, window w = i * T + t (t0_only: W = n, t = 0 only).  From every window start
 * ONE deterministic rollout of hmax = hs[n_h - 1] steps is run (the reference rolls each horizon out separately from Os[:, :-h], :143-156; a
 * deterministic rollout does not depend on how long it runs, so the state after h steps is row h of the one trajectory).
 *   model = -1: METRPO_SAM_MODEL_MEAN, the mean over the heads (avg_prediction, model_based_rl.py:626); model = k >= 0: head k alone
 *     (training_models[0], :638) -- run as METRPO_SAM_EPS_RAND with every env's cur_model_idx = k, because METRPO_SAM_ONE_MODEL is head 0 by definition
 *     (env_helpers.py:631-632).
 *   known_actions = 0: the ctx policy's clipped mean action (:149-150), through metrpo_rollout's own dispatch (metrpo_last_rollout_kernel reports the family)
 *     with determ = 1, T = hmax, H = hmax + 1 (so the path-length limit never ends a window), d_init_obs = the window starts, d_init_ts = 0.
 *   known_actions = 1 (:216-222): the recorded actions, clipped; one gather of As[i, min(t + s, T - 1)] for all hmax steps, then the body of
 *     metrpo_rollout_actions below (its dispatch; metrpo_last_rollout_actions_kernel reports the path).  A done (Ant) does not reset here: the window
 *     is dropped from that horizon on all the same.
 * Window (i, t) SERVES horizon h iff t + h <= T (the pairing Os[:, :-h] / Os[:, h:]: T + 1 - h windows per trajectory) and its rollout reported no
 * `done` at any step < h (only Ant can: a finished env is reset from the pool, its state is no prediction any more; the reference's diagnostic never
 * terminates).  Per (horizon index p, window w), zero where the window does not serve:
 *   d_state_diff [n_h][W][ns] = |Os[i, t + h] - pred|   (:159)        d_cost_diff [n_h][W] = |costs + rewards|   (:160)        d_valid [n_h][W] uint8
 *   with costs = -sum of the rollout's rewards and rewards = sum_s Rs[i, t + s], both fp32 sums in step order (:153-154).  signed_diff = 1 drops the
 *   absolute values: pred - Os[i, t + h] and costs + rewards (e_state, e_cost of :232-233).
 *   d_sums [n_h][4] float64, OVERWRITTEN: serving windows, sum_w sum_j state_diff, sum_w state_diff[:, ns - 1], sum_w cost_diff; per workgroup in a fixed
 *   shape, the workgroups' partials added in workgroup order.
 * hs is a HOST array, strictly increasing, 1 <= h <= T, n_h <= METRPO_MODEL_ERROR_MAX_HORIZONS.  Stream-ordered, no synchronisation; the trajectory lives
 * in a ctx-owned workspace.  Neither the policy, the dynamics nor an optimizer state is written.
 * d_dbg_* (all four or none): a caller-made trajectory d_dbg_obs [hmax][W][ns], d_dbg_rew [hmax][W], d_dbg_done [hmax][W], d_dbg_last_obs [W][ns] is
 * compared instead and no rollout runs (tests; timing of the comparison alone). */
#define METRPO_MODEL_ERROR_MAX_HORIZONS 32
typedef struct {
    const float* d_Os; const float* d_As; const float* d_Rs;     /* d_As may be NULL unless known_actions */
    int32_t n, T;
    const int32_t* hs; int32_t n_h;
    int32_t model, known_actions, t0_only, signed_diff;
    float* d_state_diff; float* d_cost_diff; uint8_t* d_valid; double* d_sums;
    const float* d_dbg_obs; const float* d_dbg_rew; const uint8_t* d_dbg_done; const float* d_dbg_last_obs;
} metrpo_model_error_args;
/* The window gather alone: d_init_obs [n * T][ns] <- Os[i, t], i.e. Os[:, :-1] flattened. */
int32_t metrpo_model_error_windows(metrpo_ctx* ctx, const float* d_Os, int32_t n, int32_t T, float* d_init_obs, void* stream);
int32_t metrpo_model_error(metrpo_ctx* ctx, const metrpo_model_error_args* args, void* stream);

/* ---- open-loop rollout of the ensemble under SUPPLIED actions: "what does the model predict for these actions?" -- the loop of
 * get_error_distribution(known_actions=True), env_helpers.py:216-222 (clip the recorded actions once, then per step a = actions[:, t], the model's
 * prediction, its cost), over VecSimpleEnv.step's arithmetic, env_helpers.py:597-603.  Addition to ABI 4: no struct above changes, METRPO_ABI_VERSION stays.
 * The meaning is exactly that of T chained metrpo_step calls: no policy, no reset, no path-length limit and no Philox draw -- a deterministic function
 * of its inputs.  Stepping CONTINUES BEHIND A DONE: d_done[t][b] reports is_done(s_t+1, s_t+1) (:603; only Ant can) and the env is neither stopped nor
 * reset, row t + 2 of d_obs is the model's prediction from row t + 1 whatever d_done says (the reference's diagnostic never terminates, :218-230).
 * Which kernel runs (metrpo_last_rollout_actions_kernel: -1 none yet, 0 step loop, 1 fused):
 *   fused (rollout_actions.hip: all T steps in one launch) -- swimmer, half-cheetah, Ant, hopper, snake at their own dims with two relu hidden layers of 64
 *     and a 2 x 32 policy (the shape class of the fused rollout kernels), narrower hidden layers through the zero-padded copy, K <= 8, sam_mode model_mean,
 *     eps_rand or one_model, force_step_loop = 0;
 *   step loop (metrpo_step's kernel once per step on row t of d_actions, writing row t + 1 of d_obs) -- everything else: humanoid, hidden widths above 64,
 *     other depths / activations / policy shapes, K > 8, step_rand, model_mean_std, model_med.  Bit for bit what T metrpo_step calls give.
 * The two agree to rounding, not bits: the fused kernel normalises by the reciprocal std and sums on the matrix core.
 * Stream-ordered, neither frees nor synchronises; workspace (the step loop's head vector under uniform_model) is ctx-owned.  Needs metrpo_set_dynamics only:
 * theta is never read.  Leaves metrpo_last_rollout_kernel, metrpo_rollout_note, the Philox state, both Adam states, theta and the ensemble untouched.
 * B == 0 or T == 0: METRPO_OK, nothing written. */
typedef struct {
    int32_t B, T;
    int32_t sam_mode;             /* metrpo_sam_mode, all six accepted (see dispatch)                         */
    int32_t uniform_model;        /* >= 0: the caller's promise that every env uses this head (eps_rand only;
                                     d_model then ignored and may be NULL); -1: per-env d_model               */
    int32_t force_step_loop;      /* test / A-B hook: 1 = run the step-wise path whatever the shape           */
    const float*   d_init_obs;    /* [B][ns]                                                                   */
    const float*   d_actions;     /* [T][B][na] UNCLIPPED, clipped inside as metrpo_step does (env_helpers.py:599); never written */
    const int32_t* d_model;       /* [B] eps_rand head per env                                                 */
    const int32_t* d_model_idx;   /* [T][B] step_rand (supplied only)                                          */
    const float*   d_sel_noise;   /* [T][B][ns] model_mean_std (supplied only)                                 */
    float*   d_obs;               /* [T+1][B][ns]: row 0 = d_init_obs, row t+1 = state after step t            */
    float*   d_rew;               /* [T][B]   = -cost_np_vec(s_t, clip(a_t), s_t+1)                            */
    uint8_t* d_done;              /* [T][B]   is_done(s_t+1, s_t+1); stepping CONTINUES behind a done          */
} metrpo_rollout_actions_args;
int32_t metrpo_rollout_actions(metrpo_ctx* ctx, const metrpo_rollout_actions_args* args, void* stream);
int32_t metrpo_last_rollout_actions_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 step loop, 1 fused */

/* ---- 'svg' policy update: value gradients along RECORDED rollouts (svg_utils.py:12-66; wired at model_based_rl.py:381-389, :654-660 and the 'svg'
 * branch of optimize_policy, :1204-1205).  Additions to ABI 4: no struct above changes, no option key is added, METRPO_ABI_VERSION stays.
 * metrpo_svg_grad replaces svg_gradient (svg_utils.py:12-53) and the three gradient callables it is given (:81-121): for each rollout, a list of
 * (s_t, a_t, s_t+1) triplets of which s_t+1 is never read, with lambda = 0 and t = L-1 ... 0
 *   c_s, c_a = d cost_tf(None, a_t, s_t) / d (s_t, a_t)      the "current state cost" of svg_utils.py:123-125: the cost's x_next IS s_t
 *   Pi_t     = d policy_model(s_t) / d s_t   [na x ns]        the raw mean net (training.py:96-117), stochastic = 0, NO clip
 *   F_t      = d dynamics_model([s_t, a_t]) / d [s_t, a_t]    head `model` (the reference: 'model0', model_based_rl.py:382); normalisers, column
 *              [ns x (ns + na)]                               drop and residual included; a_t fed as recorded
 *   q_t      = c_a + gamma lambda F_t[:, ns:]
 *   g_theta  = q_t (d mean / d theta)(s_t) + gamma g_theta    so g_theta_final = sum_t gamma^t q_t J_theta(s_t)
 *   lambda   = c_s + q_t Pi_t + gamma lambda F_t[:, :ns]
 * d_grad = avg_grads['theta'] = the mean over the n rollouts of g_theta, d_state_grad = avg_grads['state'] = the mean of lambda_0 (:44-53).
 * F_t and Pi_t are formed in float32 fmaf chains for all n T samples at once (path 1: one thread per (sample, output row), any widths and
 * activations; path 2: tile GEMMs with the output row as the batch axis -- relu hidden layers of >= 16 units, two weight layers or more, ns <= 64;
 * path 0 takes 2 where it applies), lambda and q are carried in float64 by one wave per rollout in a fixed summation order: repeated calls are
 * bit-identical.  chunk bounds the Jacobian stage's workspace; 0: 65 536 samples (path 1), or as many as keep the transposed chain's two buffers,
 * 2 ns chunk max_width floats, within 2^26 floats (path 2; a multiple of 64, at least 64).
 * Rows at or behind a rollout's length are never read into a result, whatever they hold (NaN included).  Ant: its cost_tf takes a fourth argument
 * (com_ant_env.py:70), the reference's cost_tf(None, a_in, s_in) raises for it: METRPO_EUNSUPPORTED, metrpo_last_error says so.
 * Needs metrpo_set_dynamics and metrpo_set_policy only.  Stream-ordered, neither synchronises nor frees; workspace is ctx-owned.  metrpo_svg_grad
 * leaves theta, both Adam states, the Philox state, the ensemble, metrpo_last_rollout_kernel and metrpo_rollout_note untouched.
 * METRPO_EINVAL: n < 1, T < 1, model outside [0, K), path outside 0 ... 2, chunk < 0, n T ns (ns + na) >= 2^31; METRPO_ENULL: d_obs, d_act or d_grad. */
typedef struct {
    const float*   d_obs;        /* [n][T][ns]  recorded s_t, trajectory-major                                        */
    const float*   d_act;        /* [n][T][na]  recorded a_t                                                          */
    const int32_t* d_len;        /* [n] steps of each rollout, clamped into [1, T] on the device; NULL: all T         */
    int32_t n, T, model, path;   /* model: head (reference: 0).  path: 0 auto, 1 generic, 2 GEMM (tests, A/B)         */
    int32_t chunk;               /* samples per Jacobian chunk; 0: the library's choice                               */
    double  gamma;               /* reference never passes one: 1.0                                                   */
    double* d_grad;              /* [P] avg_grads['theta'] in metrpo_get_policy's layout, log_std slots exactly 0     */
    double* d_state_grad;        /* [ns] avg_grads['state'], optional                                                 */
    float*  d_mean_adj;          /* [n][T][na] gamma^t q_t (rows at or behind len: 0), optional                       */
    float*  d_dyn_jac;           /* [n][T][ns][ns+na] F_t, optional                                                   */
    float*  d_pol_jac;           /* [n][T][na][ns] Pi_t, optional                                                     */
} metrpo_svg_args;
int32_t metrpo_svg_grad(metrpo_ctx* ctx, const metrpo_svg_args* args, void* stream);
/* svg_update (svg_utils.py:56-66): metrpo_svg_grad, then theta_vars += float32(-lr) * float32(avg_grads['theta']) through assign_add on the W and b
 * of the mean network (get_policy_parameters, svg_utils.py:7-10) of the ctx policy; log_std is never touched.  METRPO_ESTATE while a TRPO update is open. */
int32_t metrpo_svg_update(metrpo_ctx* ctx, const metrpo_svg_args* args, double lr, void* stream);
/* which Jacobian path the last metrpo_svg_grad / metrpo_svg_update of this ctx took (no reference counterpart: diagnostics) */
int32_t metrpo_last_svg_path(const metrpo_ctx* ctx);                                           /* -1 none yet, 1 generic, 2 GEMM */

/* ---- disagreement of the ensemble's heads at SUPPLIED (s, a) rows: "where do the K models stop agreeing?" -- the quantity model_mean_std forms inside
 * the step, np.std(next_possible_observations, axis=0) (env_helpers.py:625), returned instead of consumed, for N independent rows in one call (the N = T B
 * rows of an imagined batch; no chain of dependent steps).  Additions to ABI 4: no struct above changes, no option key is added, METRPO_ABI_VERSION stays.
 * Per row n and head k, s'_k is exactly what metrpo_step gives for head k on (d_obs[n], clip(d_actions[n])) (its d_next_all).  From the K next states:
 *   mean[d]  = (s'_0[d] + s'_1[d] + ... + s'_K-1[d]) / K           the f32 sum in head order divided by K, as model_mean forms it (:621-622)
 *   std[d]   = sqrt((sum_k (s'_k[d] - mean[d])^2) / K)             TWO-PASS: deviations from that mean, squares summed in head order by fmaf, divided by K
 *                                                                  (np.std's ddof = 0), then the root; never E[x^2] - mean^2, which loses everything when
 *                                                                  |s'| is large and the heads are close
 *   score    = sqrt(sum_d std[d]^2)  = ||std||_2                   the sum over dims of the population variances (the values under the root above), then the root
 *   maxdev   = max_k sqrt(sum_d (s'_k[d] - mean[d])^2)
 *   rew_std  = the same two-pass population std over r_k = -cost_np_vec(s, clip(a), s'_k), one reward per head (:601 with every head's own next state)
 * K = 1 gives exact zeros in std, score, maxdev and rew_std.
 * d_valid[n] = 0 skips row n: zeros are written to every requested output of that row, the row is left out of d_sums, and whatever d_obs / d_actions hold
 * there (NaN included) enters no result.  Rows at or behind N are neither read nor written.
 * d_sums [G][4] float64, OVERWRITTEN: per group g (rows_per_group > 0: rows g * rows_per_group ... , G = ceil(N / rows_per_group) -- a time-major [T][B]
 * batch flattened with rows_per_group = B gives one group per rollout step; 0: one group of all rows): valid rows, sum score, sum score^2, max score (0 for
 * a group without a valid row).  A second small launch forms them from d_score / d_valid, one fixed-shape workgroup per group adding in a fixed order: a
 * function of the inputs alone, repeated calls are bit-identical; no workgroup waits on another.  d_score may be NULL (a ctx workspace then carries it).
 * Which kernel runs (metrpo_last_disagreement_kernel: -1 none yet, 0 generic, 1 fused):
 *   fused (disagreement.hip: one launch over all rows, a wave per head with its weights in registers, striding over 16-row tiles) -- the shape class of
 *     metrpo_rollout_actions' fused kernel: swimmer, half-cheetah, Ant, hopper, snake at their own dims with two relu hidden layers of 64, narrower
 *     ones through the zero-padded copy, K <= 8, force_generic = 0.  s'_k carries the bits of that kernel's step.
 *   generic (metrpo_step's kernel once with its d_next_all, then a reduction kernel) -- everything else: humanoid, hidden widths above 64, other depths /
 *     activations, K > 8.  d_next_all is bit for bit metrpo_step's.
 * The two agree to rounding, not bits (as the two paths of metrpo_rollout_actions).
 * Stream-ordered, neither frees nor synchronises; workspaces are ctx-owned.  Needs metrpo_set_dynamics only; reads the ensemble and the normalisers and
 * writes nothing else in the context: theta, both Adam states, the Philox state, metrpo_last_rollout_kernel, metrpo_rollout_note and
 * metrpo_last_rollout_actions_kernel are untouched.  N == 0: METRPO_OK, nothing written.  METRPO_ENULL: ctx, args, d_obs, d_actions; METRPO_EINVAL: N < 0,
 * N >= 2^31, rows_per_group < 0; METRPO_ESTATE before metrpo_set_dynamics. */
typedef struct {
    int64_t N;                    /* rows */
    int32_t rows_per_group;       /* > 0: row n belongs to group n / rows_per_group (time-major [T][B] flattened, rows_per_group = B: group = step); 0: one group */
    int32_t force_generic;        /* test / A-B hook, as force_step_loop of metrpo_rollout_actions */
    const float*   d_obs;         /* [N][ns] */
    const float*   d_actions;     /* [N][na] UNCLIPPED, clipped inside as metrpo_step does (env_helpers.py:599); never written */
    const uint8_t* d_valid;       /* optional [N]; 0 = row skipped: zeros written, left out of d_sums */
    float* d_score;               /* [N]      ||std over heads of s'||_2  (sqrt of the sum over dims of the population variance, np.std's ddof = 0, :625) */
    float* d_maxdev;              /* optional [N]      max_k ||s'_k - mean||_2 */
    float* d_std;                 /* optional [N][ns]  np.std(next_possible_observations, axis=0) */
    float* d_mean;                /* optional [N][ns]  the model_mean next state */
    float* d_next_all;            /* optional [K][N][ns], metrpo_step's layout */
    float* d_rew_std;             /* optional [N]      population std over heads of r_k = -cost_np_vec(s, clip(a), s'_k) */
    double* d_sums;               /* optional [G][4] float64, OVERWRITTEN: valid rows, sum score, sum score^2, max score; G = ceil(N / rows_per_group) or 1 */
} metrpo_disagreement_args;
int32_t metrpo_ensemble_disagreement(metrpo_ctx* ctx, const metrpo_disagreement_args* args, void* stream);
int32_t metrpo_last_disagreement_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 generic, 1 fused */

/* ---- the discounted return EVERY head predicts for each of B candidate action sequences: "which of these plans does the ensemble like?" -- the cost sum
 * of build_policy_graph (model_based_rl.py:122-141: model i fixed for the whole trajectory, cost_i = sum_t gamma^t cost) under SUPPLIED actions instead of
 * the policy's, per candidate instead of averaged, negated (reward = -cost, env_helpers.py:601).  Additions to ABI 4: no struct above changes, no option key
 * is added, METRPO_ABI_VERSION stays.
 * For every head k and candidate b, head k rolls ITS OWN trajectory: s_0 = d_init_obs[b / (B / S)], s_t+1 = head k's next state from (s_t, clip(a_t)) --
 * exactly what metrpo_rollout_actions gives with eps_rand, uniform_model = k -- and r_t = -cost_np_vec(s_t, clip(a_t), s_t+1).  Per (k, b):
 *   alive_0   = 1
 *   ret       = sum_t gamma^t alive_t r_t                      carried in float64 in step order, gamma^t by repeated float64 multiplication, rounded
 *                                                              to fp32 ONCE, at the store; a step that is not counted adds nothing
 *   alive_t+1 = alive_t and not is_done(s_t+1, s_t+1)          stop_at_done = 1: the mask of model_based_rl.py:134-137, updated AFTER the step's cost,
 *                                                              so the step that ends an Ant episode still counts; stop_at_done = 0: alive = 1 throughout
 *                                                              (metrpo_rollout_actions' meaning: stepping continues behind a done)
 *   len       = steps counted: index of the first done + 1, else T
 *   ret_mean[b] = (ret_0 + ... + ret_K-1) / K                  from the stored fp32 values, summed in head order
 *   ret_std[b]  = sqrt((sum_k (ret_k - ret_mean)^2) / K)       two-pass, squares summed in head order by fmaf: rew_std of metrpo_ensemble_disagreement
 * K = 1 gives exact zeros in ret_std.
 * Which kernel runs (metrpo_last_score_actions_kernel: -1 none yet, 0 generic, 1 fused):
 *   fused (score_actions.hip: one launch, one wave per (16-candidate tile, head) for all T steps, weights in registers, no store inside the step loop) --
 *     the shape class of metrpo_rollout_actions' fused kernel WITHOUT its K <= 8: swimmer, half-cheetah, Ant, hopper, snake at their own dims with two
 *     relu hidden layers of 64, narrower ones through the zero-padded copy, force_generic = 0.  s' and r carry the bits of that kernel's one-head step.
 *   generic (per head the step loop of metrpo_rollout_actions into a ctx workspace, chunked over candidates to stay within 2^26 floats, then a
 *     reduction kernel) -- everything else: humanoid, hidden widths above 64, other depths / activations.
 * The two agree to rounding, not bits.  d_ret_mean / d_ret_std come from a second small launch over d_ret on either path (fixed order, no workgroup
 * waits on another): repeated calls are bit-identical.
 * Stream-ordered, neither frees nor synchronises; workspaces are ctx-owned.  Needs metrpo_set_dynamics only.  Leaves theta, both Adam states, the Philox
 * state, the ensemble, metrpo_last_rollout_kernel, metrpo_rollout_note, metrpo_last_rollout_actions_kernel and metrpo_last_disagreement_kernel untouched.
 * B == 0 or T == 0: METRPO_OK, nothing written.  METRPO_ENULL: ctx, args, d_init_obs, d_actions, d_ret; METRPO_EINVAL: B < 0, T < 0, S < 1, B % S != 0,
 * gamma not finite; METRPO_ESTATE before metrpo_set_dynamics. */
typedef struct {
    int32_t B, T, S;            /* B candidates, T steps; S start states, B % S == 0: candidate b starts from d_init_obs[b / (B / S)] */
    int32_t stop_at_done;       /* 1: build_policy_graph's mask (model_based_rl.py:134-137); 0: every step counts (metrpo_rollout_actions' meaning) */
    int32_t force_generic;      /* test / A-B hook, as metrpo_ensemble_disagreement's */
    double  gamma;
    const float* d_init_obs;    /* [S][ns] */
    const float* d_actions;     /* [T][B][na] UNCLIPPED, clipped inside (env_helpers.py:599); never written */
    float*   d_ret;             /* [K][B] required */
    int32_t* d_len;             /* optional [K][B] */
    float*   d_ret_mean;        /* optional [B] */
    float*   d_ret_std;         /* optional [B] */
} metrpo_score_actions_args;
int32_t metrpo_score_actions(metrpo_ctx* ctx, const metrpo_score_actions_args* args, void* stream);
int32_t metrpo_last_score_actions_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 generic, 1 fused */

/* ---- the GRADIENT of every head's predicted return with respect to the supplied action sequences: first-order information for planners that refine
 * shooting candidates (metrpo_bptt_grad gives d/d theta under the policy's own actions, not this).  Additions to ABI 4: no struct above changes, no option
 * key is added, METRPO_ABI_VERSION stays.
 * Per (head k, candidate b), R = ret[k][b] EXACTLY as metrpo_score_actions defines it above -- the loop of model_based_rl.py:122-141 with the head fixed,
 * the actions clipped as env_helpers.py:599 does, the done mask updated after the step's cost (:134-137) -- i.e. R = -sum_t w_t c_t with c = cost_tf and
 * w_t = gamma^t alive_t.  SIGN: everything here is the gradient of the RETURN, the ascent direction (the negative of the BPTT sweep's cost gradient).
 *   grad[k][t][b][:] = dR / d a_t          with respect to the UNCLIPPED action
 *   lam0[k][b][:]    = dR / d s_0
 *   grad_mean        = (grad_0 + ... + grad_K-1) / K     from the stored fp32 values, summed in head order
 * Reverse recursion from lambda_T = 0, F the head's Jacobian including both normalisers, the column drop and the residual identity (training.py:218-269):
 *   G        = lambda_t+1 - w_t dc/dx_next
 *   gU       = -w_t dc/du + (action rows of F^T G)
 *   lambda_t = G + (state rows of F^T G)
 * Conventions, all of them the BPTT sweep's (metrpo_bptt_grad): the clip gate passes the gradient iff -1 <= a <= 1 (tf.clip_by_value); relu'(h) = [h > 0];
 * the half-cheetah reward clip passes inside [-10, 10]; hopper's max terms pass on strict inequality; the alive mask is a constant of the differentiation
 * (TF's cast of a comparison); gamma^t is carried in float64 by repeated multiplication and rounded to fp32 when it becomes a weight; a step that is not
 * counted has weight 0.  Steps behind a candidate's last counted step read 0, and so does a clipped action.  ret / len are metrpo_score_actions'.
 * Which kernel runs (metrpo_last_score_actions_grad_kernel: -1 none yet, 0 generic, 1 fused):
 *   fused (score_actions_grad.hip: per chunk two stream-ordered launches -- the forward sweep is metrpo_score_actions' fused kernel with the states and
 *     weights stored, the reverse sweep runs four 16-candidate tiles of one head per workgroup on transposed matrix-instruction chains) -- exactly
 *     metrpo_score_actions' fused shape class: swimmer, half-cheetah, Ant, hopper, snake with two relu hidden layers of 64 or narrower, any K.
 *   generic (one thread per (candidate, head), activations in LDS) -- everything else: humanoid, hidden widths above 64, tanh layers, other depths.
 * The two agree to rounding, not bits.  The workspace (every state and weight of a chunk of candidates) is ctx-owned and stays within 2^26 floats by
 * chunking over candidates; chunk > 0 sets the candidates per pass instead.  Chunking changes no bit of any output.  No atomics: repeated calls are
 * bit-identical.  Stream-ordered, neither frees nor synchronises.  Needs metrpo_set_dynamics only.  Leaves theta, both Adam states, the Philox state, the
 * ensemble, metrpo_last_rollout_kernel, metrpo_last_rollout_actions_kernel, metrpo_last_score_actions_kernel and metrpo_last_disagreement_kernel untouched.
 * B == 0 or T == 0: METRPO_OK, nothing written.  METRPO_ENULL: ctx, args, d_init_obs, d_actions, d_grad; METRPO_EINVAL: B < 0, T < 0, S < 1, B % S != 0,
 * gamma not finite, chunk < 0; METRPO_ESTATE before metrpo_set_dynamics. */
typedef struct {
    int32_t B, T, S;            /* as metrpo_score_actions_args */
    int32_t stop_at_done;
    int32_t force_generic;
    int32_t chunk;              /* candidates per pass of the workspace; 0: the library's rule (the workspace within 2^26 floats) */
    double  gamma;
    const float* d_init_obs;    /* [S][ns] */
    const float* d_actions;     /* [T][B][na] UNCLIPPED; never written */
    float*   d_grad;            /* [K][T][B][na] required */
    float*   d_ret;             /* optional [K][B] */
    int32_t* d_len;             /* optional [K][B] */
    float*   d_grad_mean;       /* optional [T][B][na] */
    float*   d_lam0;            /* optional [K][B][ns] */
} metrpo_score_actions_grad_args;
int32_t metrpo_score_actions_grad(metrpo_ctx* ctx, const metrpo_score_actions_grad_args* args, void* stream);
int32_t metrpo_last_score_actions_grad_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 generic, 1 fused */

/* ---- the discounted return EVERY head predicts for each of B candidate NOISE sequences around the policy: closed-loop candidates for planners that
 * perturb the policy's actions (CEM in noise space), the per-candidate return of the deterministic policy (no noise), and the stochastic policy's return
 * under common random numbers on every head (noise in units of the policy's std).  Additions to ABI 4: no struct above changes, no option key is added,
 * METRPO_ABI_VERSION stays.
 * For every head k and candidate b, head k rolls ITS OWN trajectory from s_0 = d_init_obs[b / (B / S)]; at every step
 *   mean_t = policy_model(s_t)                                 the raw mean net of the context's theta at call time (stream-ordered)
 *   a_t    = mean_t + noise_t                                  noise_in_std = 0
 *          = fmaf(noise_t, exp(max(log_std, LOG_MIN_STD)), mean_t)   noise_in_std = 1: get_actions' arithmetic, noise_t its eps
 *          = mean_t                                            d_noise NULL
 *   u_t    = clip(a_t, -1, 1)                                  env_helpers.py:599
 *   s_t+1  = head k's metrpo_step of (s_t, u_t),  r_t = -cost_np_vec(s_t, u_t, s_t+1)
 * and the done mask is updated AFTER the step's cost (model_based_rl.py:134-137).  ret, len, ret_mean, ret_std, gamma and stop_at_done are defined
 * EXACTLY as for metrpo_score_actions above (float64 sum in step order, gamma^t by repeated multiplication, one rounding to fp32 at the store).
 * act_out[k][t][b][:] = a_t of head k's trajectory, UNCLIPPED: fed back to metrpo_score_actions it reproduces ret[k] (the step arithmetic is shared).
 * Which kernel runs (metrpo_last_score_policy_actions_kernel: -1 none yet, 0 generic, 1 fused):
 *   fused (score_policy_actions.hip: one launch, one wave per (16-candidate tile, head) for all T steps, policy and head weights in registers, no store
 *     inside the step loop unless d_act_out is given) -- metrpo_score_actions' fused shape class (which includes the 2 x 32 tanh policy), force_generic = 0.
 *   generic (per chunk of candidates, head and step: metrpo_policy_actions' launch, a small add kernel where it is needed, metrpo_step's launch with
 *     eps_rand and the head fixed; then metrpo_score_actions' reduction kernel) -- everything else.  It is a fallback and cross-check, not a fast path.
 * The two agree to rounding, not bits.  Repeated calls are bit-identical.  Stream-ordered, neither frees nor synchronises; workspaces are ctx-owned.
 * Needs metrpo_set_dynamics and metrpo_set_policy.  Leaves theta, both Adam states, the Philox state, the ensemble, every other
 * metrpo_last_*_kernel reporter and metrpo_rollout_note untouched.
 * B == 0 or T == 0: METRPO_OK, nothing written.  METRPO_ENULL: ctx, args, d_init_obs, d_ret; METRPO_EINVAL: B < 0, T < 0, S < 1, B % S != 0, gamma not
 * finite; METRPO_ESTATE before metrpo_set_dynamics or metrpo_set_policy, and while an update begun with metrpo_trpo_update_begin is open. */
typedef struct {
    int32_t B, T, S;            /* as metrpo_score_actions_args: candidate b starts from d_init_obs[b / (B / S)] */
    int32_t stop_at_done;
    int32_t noise_in_std;       /* 0: a = mean + noise;  1: a = fmaf(noise, exp(max(log_std, LOG_MIN_STD)), mean), get_actions' arithmetic */
    int32_t force_generic;      /* test / A-B hook */
    double  gamma;
    const float* d_init_obs;    /* [S][ns] */
    const float* d_noise;       /* [T][B][na], or NULL: the deterministic policy (a = mean); never written */
    float*   d_ret;             /* [K][B] required */
    int32_t* d_len;             /* optional [K][B] */
    float*   d_ret_mean;        /* optional [B] */
    float*   d_ret_std;         /* optional [B] */
    float*   d_act_out;         /* optional [K][T][B][na]: the UNCLIPPED action head k's trajectory took at step t */
} metrpo_score_policy_actions_args;
int32_t metrpo_score_policy_actions(metrpo_ctx* ctx, const metrpo_score_policy_actions_args* args, void* stream);
int32_t metrpo_last_score_policy_actions_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 generic, 1 fused */

/* ---- the GRADIENT of every head's closed-loop return with respect to the NOISE sequences around the policy: the fourth corner of the return / gradient
 * family (open loop: metrpo_score_actions / metrpo_score_actions_grad; closed loop: metrpo_score_policy_actions / this), first-order information for
 * planners that refine candidates in noise space.  Additions to ABI 4: no struct above changes, no option key is added, METRPO_ABI_VERSION stays.
 * Per (head k, candidate b), R = ret[k][b] EXACTLY as metrpo_score_policy_actions defines it above; ret, len and act_out carry that call's bits on the
 * same path.  SIGN: the gradient of the RETURN, the ascent direction.
 *   grad[k][t][b][:] = dR / d noise_t      TOTAL: every later step's policy sees the states this noise moved
 *   lam0[k][b][:]    = dR / d s_0          policy path included
 *   grad_mean        = (grad_0 + ... + grad_K-1) / K     from the stored fp32 values, summed in head order
 * Reverse recursion from lambda_T = 0, metrpo_score_actions_grad's with one more term:
 *   G        = lambda_t+1 - w_t dc/dx_next
 *   gU       = -w_t dc/du + (action rows of F^T G)
 *   gm       = gate(a_t) gU                                    dR / d a_t, total
 *   grad_t   = gm                                              noise_in_std = 0
 *            = gm * exp(max(log_std, LOG_MIN_STD))             noise_in_std = 1 (the sigma of the forward sweep)
 *   lambda_t = G + (state rows of F^T G) + J_pi(s_t)^T gm      the policy path
 * Conventions: those of metrpo_score_actions_grad and the BPTT sweep -- the clip gate passes iff -1 <= a_t <= 1 on the head's own UNCLIPPED
 * a_t = mean_t + noise_t sigma (stored by the forward sweep, so the two sweeps cannot disagree by a rounding); relu'(h) = [h > 0]; tanh' = 1 - p^2 of
 * the recomputed activation; the alive mask is a constant; gamma^t in float64, rounded to fp32 where it becomes a weight.  A step behind a candidate's
 * last counted step reads 0, and so does a clipped action.  d_noise NULL: the gradient at noise = 0 (bit for bit that of a zero tensor).
 * Which kernel runs (metrpo_last_score_policy_actions_grad_kernel: -1 none yet, 0 generic, 1 fused):
 *   fused (score_policy_actions_grad.hip: per chunk two stream-ordered launches -- metrpo_score_policy_actions' fused step with states, weights and the
 *     head's unclipped actions stored, then a reverse sweep of four 16-candidate tiles of one head per workgroup with the policy's input adjoint behind
 *     the clip gate) -- exactly metrpo_score_policy_actions' fused shape class.
 *   generic (one thread per (candidate, head), activations in LDS) -- everything else, and force_generic.
 * The two agree to rounding, not bits.  The workspace (XS | WT | AW of a chunk of candidates) is ctx-owned and stays within 2^26 floats by chunking;
 * chunk > 0 sets the candidates per pass instead.  Chunking changes no bit of any output.  No atomics: repeated calls are bit-identical.  Stream-ordered,
 * neither frees nor synchronises.  Leaves theta, both Adam states, the Philox state, the ensemble and every other metrpo_last_* reporter untouched.
 * B == 0 or T == 0: METRPO_OK, nothing written.  METRPO_ENULL: ctx, args, d_init_obs, d_grad; METRPO_EINVAL: B < 0, T < 0, S < 1, B % S != 0, gamma not
 * finite, chunk < 0; METRPO_ESTATE: as metrpo_score_policy_actions. */
typedef struct {
    int32_t B, T, S;            /* as metrpo_score_policy_actions_args */
    int32_t stop_at_done;
    int32_t noise_in_std;
    int32_t force_generic;
    int32_t chunk;              /* candidates per workspace pass; 0: the library's rule (2^26 floats) */
    double  gamma;
    const float* d_init_obs;    /* [S][ns] */
    const float* d_noise;       /* [T][B][na], or NULL: gradient at noise = 0 (the deterministic policy); never written */
    float*   d_grad;            /* [K][T][B][na] required: dR_k / d noise_t */
    float*   d_ret;             /* optional [K][B] */
    int32_t* d_len;             /* optional [K][B] */
    float*   d_grad_mean;       /* optional [T][B][na] */
    float*   d_lam0;            /* optional [K][B][ns]: dR_k / d s_0, policy path included */
    float*   d_act_out;         /* optional [K][T][B][na]: the unclipped actions taken */
} metrpo_score_policy_actions_grad_args;
int32_t metrpo_score_policy_actions_grad(metrpo_ctx* ctx, const metrpo_score_policy_actions_grad_args* args, void* stream);
int32_t metrpo_last_score_policy_actions_grad_kernel(const metrpo_ctx* ctx);   /* -1 none yet, 0 generic, 1 fused */

/* ---- a TERMINAL VALUE for the four corners above: "what is the state behind the horizon worth?"  Without one every corner scores a candidate by
 * sum_{t<T} gamma^t alive_t r_t and stops, so a planner prefers plans that cash in inside the window.  With one set, ret gains gamma^T alive_T V(s_T) and
 * the two gradient calls start their reverse recursion from the matching seed.  Additions to ABI 4: no struct above changes, no option key is added,
 * METRPO_ABI_VERSION stays.
 * V is LinearFeatureBaseline's form once its time features are evaluated at a fixed step (metrpo_baseline_gram's feature row [o, o^2, al, al^2, al^3, 1]
 * with al fixed): a diagonal quadratic in the clipped state plus a bias,
 *   o_d     = clip(s_d, -10, 10)
 *   V(s)    = bias + sum_d (w1[d] o_d + w2[d] o_d^2)      fp32, dims in order: v = bias; v = fmaf(o_d, fmaf(w2[d], o_d, w1[d]), v)
 *   dV/ds_d = fmaf(2 w2[d], o_d, w1[d])  if -10 <= s_d <= 10,  else 0      tf.clip_by_value's convention, as at the action clip
 * V is context state, like theta and the dynamics: d_w1, d_w2 [ns] and d_bias [n_bias] are DEVICE pointers, copied stream-ordered into ctx-owned memory
 * (metrpo_set_policy's stream discipline; neither frees nor synchronises).  n_bias is 1 (one bias for every candidate) or the scoring call's S
 * (candidate b uses bias[b / (B / S)]: the start states of a vectorised controller sit at different path steps, and the baseline's time features
 * move the bias).  metrpo_clear_terminal_value unsets it; metrpo_has_terminal_value: 0, or the n_bias that is set.
 * While a value is set, in all four calls and on both of their paths:
 *   ret      with the sum's fields behind the T-th step (disc = gamma^T, alive after the last step's mask update): if (alive) sum += disc * (double)V(s_T),
 *            in front of the single rounding to fp32.  A candidate that met a done, at the last step included, gets no bootstrap.  len is unchanged;
 *            ret_mean / ret_std come from the stored values, as always.
 *   grad     w_T = alive_T ? (float)gamma^T : 0; the recursion starts from lambda_T = w_T dV/ds_T instead of 0 and is otherwise the one stated above
 *            (closed loop: the seed reaches J_pi through G like any lambda).  w_T is stored by the forward sweep, one more slice of WT.
 *   ret, len and act_out of a gradient call keep carrying the bits of the matching scoring call; chunking changes no bit; repeated calls are
 *   bit-identical; B == 0 or T == 0 still writes nothing.  A scoring call while n_bias is neither 1 nor its S: METRPO_EINVAL, nothing written.
 * With none set every output of the four calls is what it was.  Every other entry point ignores the terminal value.
 * The fused kernels evaluate V once per lane BEHIND the step loop from the state rows the loop leaves in LDS: nothing is added inside the loop.
 * metrpo_set_terminal_value: METRPO_ENULL: ctx or a pointer; METRPO_EINVAL: n_bias < 1. */
int32_t metrpo_set_terminal_value(metrpo_ctx* ctx, const float* d_w1, const float* d_w2, const float* d_bias, int32_t n_bias, void* stream);
int32_t metrpo_clear_terminal_value(metrpo_ctx* ctx);
int32_t metrpo_has_terminal_value(const metrpo_ctx* ctx);   /* 0 / n_bias */

/* ---- the terminal value's SECOND form: a two-layer tanh value net.  The diagonal quadratic above cannot couple state dims ("forward velocity is worth
 * more while the torso is upright"); a small MLP behind a short horizon can.  Further additions to ABI 4: no struct changes, no option key is added.
 *   o_d  = clip(s_d, -10, 10)
 *   p0   = tanh(W0^T o + b0)          h1 units
 *   p1   = tanh(W1^T p0 + b1)         h2 units
 *   V(s) = bias_row + (b2 + sum_j W2[j] p1[j])            bias_row = bias[n_bias > 1 ? b / (B / S) : 0], the rule above
 *   dV/ds_d = (W0 (W1 (W2 * (1 - p1^2)) * (1 - p0^2)))_d  if -10 <= s_d <= 10,  else 0
 * fp32, one device function for every kernel: each sum starts from its bias and adds by fmaf in input order, tanh is the library's tanh_fast; the head
 * b2 + sum_j W2[j] p1[j] is accumulated from b2 in unit order and THEN added to bias_row (so W2 = 0, b2 = 0 gives bias_row exactly, as the quadratic
 * form with w1 = w2 = 0 does).
 * d_params is a DEVICE pointer, weights in-major like theta:  W0 [ns][h1] | b0 [h1] | W1 [h1][h2] | b1 [h2] | W2 [h2] | b2 [1];  1 <= h1, h2 <= 32, the
 * policy's own shape class.  The context keeps a zero-padded 32 x 32 image (exact: tanh_fast(0) = 0 and a zero weight adds an exact zero).
 * The clip acts on the RAW state, so an input normaliser (o - mean) / std folds into W0 and b0 exactly; fold it on the host.  tanh is the only
 * activation built.
 * Context state and stream discipline are metrpo_set_terminal_value's: stream-ordered into ctx-owned memory through the one growth path, neither frees
 * nor synchronises.  Setting either form replaces the other; metrpo_clear_terminal_value clears whichever is set; metrpo_has_terminal_value returns
 * n_bias for either; metrpo_terminal_value_kind says which.  Everything stated above about ret, grad, w_T, the bits shared between the calls, chunking,
 * repeated calls, n_bias against S and the other entry points holds unchanged for this form.  The forward kernels evaluate the net once per lane behind
 * their step loop; the gradient calls form the seed lambda_T = w_T dV/ds_T in one small launch between their two sweeps.
 * METRPO_ENULL: ctx or a pointer; METRPO_EINVAL: h1 or h2 outside [1, 32], n_bias < 1. */
int32_t metrpo_set_terminal_value_mlp(metrpo_ctx* ctx, const float* d_params, int32_t h1, int32_t h2, const float* d_bias, int32_t n_bias, void* stream);
int32_t metrpo_terminal_value_kind(const metrpo_ctx* ctx);   /* 0 none, 1 quadratic, 2 mlp */

#ifdef __cplusplus
}
#endif
#endif /* METRPO_H */
