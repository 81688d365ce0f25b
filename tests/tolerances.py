"""The fp32 tolerance the HIP path guarantees against the float64 oracle / the reference's float64 outputs -- ONE table, the one printed in
DESIGN.md section 5 ("Stated fp32 tolerances").  Every tests/test_gpu_*.py takes its bounds from here; a row may only be loosened here and in
DESIGN.md together, with the reason.  u = 2^-24 = 5.96e-8 is the fp32 unit round-off; "observed" is the worst case over the whole GPU suite
(a run of the suite with METRPO_TOL_REPORT=<file>, see conftest.py; round 4's is summarised in profiles/r04_tolerance_report.txt).

Inputs common to both sides are rounded to fp32 first (the device's storage type), so the bounds cover arithmetic only.  assert_allclose
semantics: |got - ref| <= atol + rtol * |ref| element by element; rel-L2 = ||got - ref||_2 / ||ref||_2.
"""

# --- one step of the model, inputs given (teacher-forced): row 1 -------------------------------------------------------------------------------------
# next state of every ensemble head, the selected next state, the policy mean, hidden widths <= 64.  Sums of <= 64 fp32 products by fmaf in a fixed
# order (error <= sqrt(n) u |w||h| ~ 5e-7 on O(1) pre-activations), tanh with <= 2 ulp, de-normalisation x std + mean.  Observed 6.6e-7 absolute.
# tests/test_gpu_rollout_edges.py holds every 2 x 64 rollout instantiation (47 table entries in every launch form, 2331 cases) to this row at the tile edges:
# worst share observed there mean 0.38, act (ACTION) 0.21, rew (REWARD) 0.050, next state 0.019 (profiles/r20_rollout_edges.txt).
# rtol 1e-5, atol 1e-6.
STEP = dict(rtol=1e-5, atol=1e-6)
# the analytic reward of the same step (env_helpers cost_np_vec): a handful of fp32 operations on the next state; same figure as the state
REWARD = dict(rtol=1e-5, atol=1e-6)
# the sampled action a = mean + exp(log_std) * eps (fp32 expf, one fma): row 1 with the exponential's 2 ulp on an O(1) product
ACTION = dict(rtol=1e-5, atol=2e-6)

# --- one step, wide nets (hidden 128 ... 1024; the MFMA paths): row 2 ------------------------------------------------------------------------------------
# sums 2x ... 16x longer, formed in the MFMA's own order (4 partial chains of k mod 16, chunks of 32): sqrt(n) growth -> 4x row 1's absolute bound,
# 2x its relative one.  Observed 8.6e-7 absolute.  SURVEY 8d has no separate figure (its row 1 figure is for the 2x64 nets).
# tests/test_gpu_wide_rollout_edges.py holds the wide-net rollout kernels in every sub-form the dispatch chooses between (52 forms: tile GEMMs, every
# pre-step, stream-K modes 1 - 3 with and without the late split, persistent, the ten resident entries; 1126 cases) to this row at the edges of their own
# tilings (the 2 x 32 policy's mean and the widths 72 / 96 to row 1, the action to ACTION).  Worst share observed there, per family -- tile GEMMs: mean
# 0.33, act 0.16, rew 0.036, next state 0.014; stream-K: 0.41, 0.17, 0.010, 0.006; persistent: 0.41, 0.18, 0.011, 0.007; resident: 0.36, 0.20, 0.010,
# 0.005 (profiles/r27_wide_rollout_edges.txt).
WIDE = dict(rtol=2e-5, atol=5e-6)

# --- free-running rollouts: rows 3, 4 --------------------------------------------------------------------------------------------------------------
# device and oracle each feed their OWN states back.  t <= 10: SURVEY 8d keeps the single-step figure; the learned dynamics' Jacobian has norm ~1 on the
# fixtures, errors add up linearly: observed 7.5e-8 .. 4.8e-7.
FREE_RUN = dict(rtol=1e-5, atol=1e-6)
# beyond t = 10 (the reference's sampler runs: whole episodes of 100+ steps) SURVEY 8d asks for statistical agreement only; the suite still asserts
# element by element, at 10x the single-step figure (observed 3.2e-7 absolute)
LONG_RUN = dict(rtol=1e-4, atol=1e-5)
# two DEVICE kernel families free-running on the same draws (resident / step-wise / stream-K / generic): different summation orders of the
# same fp32 sums, a few steps: row 2's bound per step x steps <= 10
CROSS_KERNEL = dict(rtol=1e-4, atol=2e-5)

# --- per-model validation cost (discounted sum of T costs, mean over the batch): row 5 -----------------------------------------------------------------
# free-running T <= 15 steps, then a float64 batch mean: the per-step figure times the number of steps.  Observed 1.1e-6 on costs of O(10).
VALIDATION_COST = dict(rtol=2e-5, atol=2e-6)

# --- process_samples: rows 6, 7 -----------------------------------------------------------------------------------------------------------------
# returns: suffix sums of <= 1000 fp32 rewards by a wavefront scan (log-depth tree: error ~ log2(T) u |sum|); observed 1.3e-7
RETURNS = dict(rtol=1e-5, atol=1e-5)
# advantages before centring (GAE over deltas that hold the baseline prediction, an fp32 dot product of 2 ns + 4 features) and after centring
# ((a - mean) / (std + 1e-8), statistics summed in float64).  SURVEY 8d: atol 1e-4 after centring; observed 1.2e-6
ADVANTAGE = dict(rtol=1e-5, atol=5e-5)
ADVANTAGE_CENTRED = dict(rtol=1e-4, atol=1e-4)
# k_gae itself, against the float64 restatement tests/process_ref.py (tests/test_gpu_process_kernels.py): the kernel forms the baseline values, deltas,
# advantages and returns in float64 and rounds ONCE, when it stores adv / ret as fp32.  Its float64 value differs from the sequential float64 scan only
# by the rounding of the composed chunk carry (a few float64 ulps of the largest term, <= 1e-13 of scale at T = 1000), so the stored value is within
# half an fp32 ulp of the reference plus that: 1 ulp = spacing(fp32(|ref|)).  Where |ref| is tiny (cancelling terms) the float64 error of the
# terms dominates: GAE_FLOOR x max |ref| of the case.  A carry factor in fp32, a float t/100, a V read from the wrong step miss it by orders.
# Observed 0.50 of the bound over 37 shapes (T up to 1000, rewards up to 1e3): exactly the store's half ulp (profiles/r07_process_coverage.txt).
GAE_ULP = 1
GAE_FLOOR = 1e-12
# the refitted linear baseline: normal equations from fp32 products summed in float64, solved in float64; the fit's conditioning (kappa ~ 1e3 on the
# fixtures) multiplies the 2e-6 relative error of the moments.  Bound on predictions, relative to max |prediction|.  Observed 6.7e-5.
BASELINE_FIT = 1e-3
NORMAL_EQ = 2e-6            # entries of A^T A / A^T y relative to sqrt(G_ii G_jj): fp32 products, float64 sums

# --- the TRPO update: rows 8 .. 12 ----------------------------------------------------------------------------------------------------------------
LOSS_RTOL = 1e-5            # surrogate loss relative to max(1, |loss|): per-sample fp32, float64 block reduction (rtol 1e-5)
KL_ATOL = 1e-7              # mean KL at theta_old (atol 1e-7); at a trial theta also 1e-4 relative (KL is a difference of O(1) terms)
KL_RTOL = 1e-4
# Both vector rows also hold per variable (W_l, b_l, log_std), dealt out by block size: block_bound() below.  tests/test_gpu_update_kernels.py holds every
# instantiation of the update kernels to these rows at the tile edges (328 cases); worst share of a bound observed there: loss 0.12, KL 0.42,
# gradient 0.31 whole / 0.58 per block, FVP 0.50 whole / 0.52 per block (profiles/r10_update_kernels.txt).
# The solve built from those kernels -- cached products, CG tails, step scale, line search -- is held on the same cases by tests/test_gpu_trpo_solve.py (the
# SOLVE_* rule below; profiles/r12_trpo_solve.txt).
GRAD_REL_L2 = 1e-5          # gradient g (1e-5): per-sample back-propagation in fp32, sums over N in float64.  Observed 1.1e-6
FVP_REL_L2 = 1e-5           # Fisher-vector product (1e-4; held 10x tighter): tangent + back-propagation in fp32, float64 sums over N.  Observed 1.2e-7
CG_COS = 0.9999             # step direction d after 10 CG iterations (cosine >= 0.9999, rel-L2 <= 1e-3: ten FVPs amplify rounding by the
CG_REL_L2 = 3e-4            # Fisher matrix's condition number, ~1e3 on the fixtures).  Observed 7.4e-5; held at 3e-4
STEP_SCALE_RTOL = 1e-3      # beta = sqrt(2 delta / d.Hd): inherits d's figure
THETA_STEP_REL_L2 = 5e-4    # theta_new - theta_old = -ratio * beta * d: d's and beta's figures added.  Observed 8.3e-5
POST_UPDATE_RTOL = 5e-3     # loss / KL evaluated at the (slightly different) accepted theta

# The CG solve at the tile edges (tests/test_gpu_trpo_solve.py; table and float64 side tests/solve_cases.py): d after k = 0 ... 10 iterations, beta and
# step = beta d, whole vector and per variable W_l, b_l, log_std, are held to a bound derived per case from the REFERENCE, not to the ten-iteration
# figures above: the movement of the float64 solve (oracle.metrpo_oracle, started from the device's gradient) when each of its products z_i is
# perturbed by what the FVP_REL_L2 row already admits -- a seeded random direction whose norm per variable block is block_bound(FVP_REL_L2, z_i[blk], z_i)
# -- worst over SOLVE_DRAWS draws, times SOLVE_MARGIN because random directions underestimate the worst direction.  No bound lies below 1e-12 of the
# reference's norm (the float64 side's own rounding).  tests/test_solve_cases.py holds, without the library: every per-block bound is <= 0.1 of its
# block, and a product with one block scaled by 1 + 1e-3, a left-out tile, included invalid samples, a stale CG vector or a missing reg term exceeds one.
SOLVE_DRAWS = 4
SOLVE_MARGIN = 2.0

# --- several ranks against one (sharded sums exchanged in float64): row 13 ------------------------------------------------------------------------------
MULTI_RANK_GRAD = 2e-6      # x max |g|: the same float64 partial sums added in another order, over fp32 per-sample terms
MULTI_RANK_THETA = 2e-3     # x |step|: as THETA_STEP_REL_L2


def wide_or_step(hidden):
    """Row 1 for the 2x64-class nets, row 2 from 128 hidden units on."""
    return STEP if max(hidden) <= 64 else WIDE


def block_bound(row, ref_blk, ref):
    """Bound on ||got_blk - ref_blk||_2 for one variable (W_l, b_l or log_std) of a gradient or Fisher-vector product whose whole vector is held
    to rel-L2 `row` (GRAD_REL_L2 / FVP_REL_L2):  row * max(||ref_blk||_2, sqrt(n_blk / P) * ||ref||_2).
    This is the whole-vector bound dealt out by block size, nothing newly measured: the vector's error budget row * ||ref||_2 split evenly over
    its P entries gives a block of n_blk entries sqrt(n_blk / P) of it, and a block that carries more than its even share of the norm is held
    to `row` of itself.  The whole-vector figure cannot see a narrow block: log_std (na of 1 476 entries at C1) or b_2 wrong by O(1) of itself
    moves it by less than `row`; this bound fails such a block by ||ref_blk|| / bound >= 1 / (row * max(1, sqrt(n_blk / P) ||ref|| / ||ref_blk||))."""
    import numpy as np
    nb, n = float(np.linalg.norm(ref_blk)), float(np.linalg.norm(ref))
    return row * max(nb, (float(np.size(ref_blk)) / float(np.size(ref))) ** 0.5 * n)


# --- widened rows: BPTT policy update and ensemble training -----------------------------------------------------------------------------
BPTT_COST = VALIDATION_COST           # the same discounted cost sums, with the tape kept
# gradient through T <= 30 chained fp32 Jacobians (dynamics o policy): the one-step 1e-5 times T.  tests/test_gpu_bptt.py and test_gpu_bptt_stochastic.py
# hold the whole vector to it (and a cosine); per variable (W_l, b_l, log_std, by block_bound() above) it is held by tests/test_gpu_bptt_edges.py, at
# the tile edges of every sweep and VJP family, on envs drawn clear of every relu / clip / cost / done kink (tests/bptt_cases.py).  The float32 NumPy
# restatement of those cases uses 0.003 of the per-variable bound (tests/test_bptt_cases.py): no block needs an exception.
BPTT_GRAD_REL_L2 = 3e-4
DYN_LOSS = dict(rtol=3e-5, atol=1e-7)     # per-model training loss: mean over batch x ns squared errors in fp32 tiles, float64 across tiles
DYN_EVAL_LOSS = dict(rtol=5e-4, atol=1e-6)   # validation loss after training steps: weights already differ by Adam's sign-like early steps (below)
# Weight and bias gradient of the training step, read out of the Adam moments after a step with lr = 0 (tests/test_gpu_dyn_train_grad.py), per
# (head, layer, W | b) block: contractions over the batch (<= 1000 rows: serial MFMA chains, or split-K partials added in split order) of fp32
# products whose operands carry the forward and back-propagated errors of row 2.  A serial chain's error grows as sqrt(n) u over terms that
# mostly cancel: ~ 1e-6 relative.  GRAD_REL_L2's figure.  The data are drawn so that no relu pre-activation lies within the fp32 error of zero
# (a flipped mask bit moves one sample's term, up to 6e-3 of a block's norm); worst element relative to the block's largest |g|.
# Observed 7.2e-7 rel-L2 and 1.3e-6 worst element (14 shapes, params-file 2 x 1024 and C4 3 x 1024 included).
DYN_GRAD_REL_L2 = 1e-5
DYN_GRAD_MAX = 1e-4

# --- the rollout's own draws (Philox4x32-10 + Box-Muller, csrc/device_common.h) against their float64 restatement ------------------------------------------
# |z_device - z_float64| of one standard normal, z_device recovered as (act - mean) / exp(log_std) from a rollout that drew for itself and z_float64
# from tests/rollout_draws_ref.py (same fp32 uniform; logarithm, square root, sine and cosine in float64).  The words are integers and agree exactly;
# what differs is the device's __logf / __sincosf on radii up to 6.8, plus the recovery's own rounding (act is one fp32 fma of O(1) terms).  Observed over
# the 59 production-mode cases of tests/test_gpu_rollout_draws.py (254 862 normals, all seven kernel families): worst 1.49e-6; floor of the recovery
# alone (parity-mode eps through the same kernels, 8 mixed-mode cases) 2.1e-7.  Bound = 4 x the worst, rounded up to one digit: the margin is for the
# ~1e6 of 2^64 word pairs sampled.  Normals whose restated radius is below 2^-6 are left out of this one check (the logarithm's absolute error is
# divided by r there); 41 of the 254 862 were (at most 9.7e-4 of a case, cap 1e-3), and they turned out closer than the rest: worst 1.8e-8.
# A wrong chunk, a swapped sine / cosine or another word is off by O(1).  profiles/r09_rollout_draws.txt.
PHILOX_NORMAL = 6e-6
