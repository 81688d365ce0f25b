"""Early-stopping state machine of the TRPO inner loop: utils.py:285-296 (stop_critereon),
model_based_rl.py:1339-1371 (is_done), :1403-1419 (update_stats) and the loop control of
optimize_policy (:1171-1180, 1209-1299, 1301): snapshot theta, iterate TRPO, every `log_every`
iterations evaluate the K per-model validation costs (build_policy_graph forward, :106-151),
keep/restore the best policy, stop after `num_iters_threshold` iterations without improvement.
Host control flow in NumPy exactly as the reference; the costs come from the validation kernel."""
import numpy as np
import torch


class StopCriterion(object):
    """Callable with the reference's signature `f(loss_old, loss_new, mode='scalar')` (utils.py:285-296).
    scalar: relative increase of the loss above `threshold`; vector: fraction of models that got worse above
    `percent_models_threshold` (ties are not "worse")."""

    def __init__(self, threshold, offset, percent_models_threshold=0.5):
        self.threshold, self.offset, self.percent_models_threshold = threshold, offset, percent_models_threshold

    def __call__(self, loss_old, loss_new, mode='scalar'):
        if mode == 'vector':
            if not isinstance(loss_new, np.ndarray):
                raise AssertionError("vector mode compares per-model cost arrays")
            worse = np.count_nonzero(np.asarray(loss_new) > np.asarray(loss_old))
            return worse / float(np.size(loss_new)) > self.percent_models_threshold
        if mode != 'scalar' or np.ndim(loss_new) != 0:
            raise AssertionError("scalar mode compares two numbers")
        return (loss_new - loss_old) / (abs(loss_old) + self.offset) > self.threshold


stop_critereon = StopCriterion          # the reference's (mis-spelt) factory name, same argument order


def _per_model(costs):
    """True for the K-vector trackers (handled element-wise), False for scalars and length-1 arrays (replaced whole)."""
    return np.ndim(costs) > 0 and np.size(costs) != 1


def is_done(mode, stop_fn, min_validation_costs, candidates):
    """Stop decision of model_based_rl.py:1339-1371 for one validation round: True = the new policy is worse."""
    if mode == 'no_early':
        return False
    if mode in ('real', 'trpo_mean'):
        return bool(min_validation_costs[mode] < candidates[mode])
    if mode == 'one_model':
        return bool(min_validation_costs['estimated'][0] < candidates['estimated'][0])
    if 'estimated' not in mode:
        raise AssertionError("unknown early-stopping mode %r" % (mode,))
    return any(bool(stop_fn(best, candidates[key], mode='vector'))
               for key, best in min_validation_costs.items() if 'estimated' in key)


def update_stats(min_validation_costs, candidates, whole=False):
    """Bookkeeping of model_based_rl.py:1403-1419: with `whole` every tracker takes the candidate; otherwise each entry keeps
    its minimum (per model for the K-vectors, which are updated in place)."""
    for key in list(min_validation_costs):
        best, new = min_validation_costs[key], candidates[key]
        if _per_model(best):
            take = np.ones(np.shape(best), dtype=bool) if whole else np.asarray(best) > np.asarray(new)
            best[take] = np.asarray(new)[take]
        elif whole or best > new:
            min_validation_costs[key] = new


def optimize_policy(algo, validation_init, T, gamma, mode='estimated', whole=True, log_every=5,
                    num_iters_threshold=25, max_iters=400, stop_fn=None, reset_log_std=True, real_cost_fn=None,
                    logger=None, init_pool=None):
    """TRPO branch of model_based_rl.py:optimize_policy (a VPG object runs the same branch: optimize_policy_vpg); a BPTT object as `algo` runs its
    'bptt' / 'bptt-stochastic' branch instead, and an LBFGS object the 'l-bfgs' branch: that loop with log_every = 1 and max_iters = 1
    (optimize_policy_bptt; `init_pool` is then its source of reset states).  An SVG object runs the 'svg' branch (:1204-1206) through the same
    loop (optimize_policy_svg; `init_pool` is then the recorded rollout_data): one svg_update on the same rollout_data per iteration, training
    cost 0.0, validation every log_every iterations, keep-or-restore.  This DIVERGES from the reference as written, whose loop breaks after
    the first validation round (:1280-1282) and restores the entry checkpoint (:1400), leaving the policy unchanged.  `real_cost_fn()` stands in for
    evaluate_fixed_init_trajectories on the real simulator (out of scope; None -> 0.0)."""
    from .bptt import BPTT
    from .algos import VPG, PPO
    from .lbfgs import LBFGS
    from .svg import SVG
    if isinstance(algo, SVG):
        # 'svg' branch (:1204-1206).  DIVERGENCE from the reference as written: its loop breaks unconditionally after the first validation round
        # (:1280-1282) and log_and_restore (:1400) then restores the checkpoint saved at entry (:1127-1129) -- the run leaves the policy unchanged.
        # Here: the 'bptt' branch's loop, one svg_update on the same rollout_data per iteration, training cost 0.0, validation every log_every
        # iterations, keep-or-restore.  `init_pool` carries rollout_data (collect_data's list of triplet lists) unless algo.rollout_data is set.
        return optimize_policy_svg(algo, validation_init, T, gamma, init_pool, mode=mode, whole=whole, log_every=log_every,
                                   num_iters_threshold=num_iters_threshold, max_iters=max_iters, stop_fn=stop_fn, real_cost_fn=real_cost_fn,
                                   logger=logger)
    if isinstance(algo, LBFGS):
        # run_model_based_rl.py:114-117 (l_bfgs_exception, applied on every launch path): log_every = 1, max_iters = 1 -- one whole
        # minimisation, one validation round, one keep-or-restore decision of the 'bptt' branch's loop (which carries theta only)
        return optimize_policy_bptt(algo, validation_init, T, gamma, init_pool, mode=mode, whole=whole, log_every=1,
                                    num_iters_threshold=num_iters_threshold, max_iters=1, stop_fn=stop_fn, real_cost_fn=real_cost_fn,
                                    logger=logger)
    if isinstance(algo, (VPG, PPO)):      # PPO: the same wiring (Adam state snapshotted and restored with theta, not reset at entry)
        return optimize_policy_vpg(algo, validation_init, T, gamma, mode=mode, whole=whole, log_every=log_every, num_iters_threshold=num_iters_threshold,
                                   max_iters=max_iters, stop_fn=stop_fn, reset_log_std=reset_log_std, real_cost_fn=real_cost_fn, logger=logger)
    if isinstance(algo, BPTT):
        return optimize_policy_bptt(algo, validation_init, T, gamma, init_pool, mode=mode, whole=whole, log_every=log_every,
                                    num_iters_threshold=num_iters_threshold, max_iters=max_iters, stop_fn=stop_fn, real_cost_fn=real_cost_fn,
                                    logger=logger)
    eng = algo.engine
    stop_fn = stop_fn or stop_critereon(0.10, 1e-5, 0.30)
    if reset_log_std:
        algo.policy.reset_log_std()                                        # kwargs['reset_opt'], :1119-1121
    snapshot = eng.get_policy().clone()                                    # saver.save(policy.ckpt), :1127-1129
    # real_cost_fn must return the same value on every rank (evaluate it on rank 0 and broadcast, or on identical simulators)
    real = (lambda: float(real_cost_fn())) if real_cost_fn else (lambda: 0.0)
    est = lambda: eng.validation_cost(validation_init, T, gamma).cpu().numpy()
    min_costs = {'real': real(), 'trpo_mean': np.inf, 'estimated': est()}  # :1153-1163
    best_index, candidates, history = 0, {}, []
    j = 0
    for j in range(1, max_iters + 1):
        algo.start_worker()                                                # :1175
        paths = algo.obtain_samples(j)
        samples_data = algo.process_samples(j, paths)
        algo.optimize_policy(j, samples_data)
        if j % log_every == 0:                                             # :1209
            if mode == 'trpo_mean':                                        # :1221-1229
                determ = algo.obtain_samples(j, determ=True)
                tr = determ.traj
                comp = tr.done.flip(0).cummax(0).values.flip(0).bool()
                # every rank must take the same stop decision (else they issue different numbers of all-reduces): the mean
                # return is formed from the GLOBAL (sum of returns, number of paths) pair
                pair = torch.stack([(tr.rew * comp).sum().double(), tr.done.sum().double()])
                algo.comm.allreduce_sum_(pair)
                pair = pair.cpu()
                candidates['trpo_mean'] = float(-pair[0].item() / max(1.0, pair[1].item()))
            else:
                candidates['trpo_mean'] = 0.0
            candidates['estimated'] = est()                                # :1239-1241
            candidates['real'] = real()
            history.append((j, float(np.mean(candidates['estimated']))))
            if logger:
                logger('iter %d est=%s' % (j, np.array_str(candidates['estimated'], precision=3)))
            if not is_done(mode, stop_fn, min_costs, candidates):          # :1286-1295
                best_index = j
                snapshot = eng.get_policy().clone()
                update_stats(min_costs, candidates, whole)
            if j - best_index >= num_iters_threshold:                      # :1298
                break
    eng.set_policy(snapshot)                                               # log_and_restore, :1301/:1400
    return dict(best_index=best_index, last_index=j, min_validation_costs=min_costs, history=history)


def optimize_policy_vpg(vpg, validation_init, T, gamma, mode='estimated', whole=True, log_every=5, num_iters_threshold=25, max_iters=400,
                        stop_fn=None, reset_log_std=True, real_cost_fn=None, logger=None):
    """'vpg' branch of model_based_rl.py:optimize_policy (:1171-1180 with the rllab VPG): the TRPO branch's loop with three differences of the
    reference's wiring.  The Saver (:495) covers every global variable, so the snapshot (:1127 / :1291) and the restore (:1400) carry theta AND
    VPG's Adam state (m, v, t) together.  policy_adam_init is empty for non-BPTT algorithms (:398-405): the Adam state is not reset at entry and
    carries over between calls.  trpo_mean is computed for algo == 'trpo' only (:1219-1231): its candidate is 0.0 here.
    A PPO object (params 'algo': 'ppo', an extension: the reference's training.py has no such branch) runs this loop unchanged: its n_epochs Adam
    steps per optimize_policy move the same state."""
    eng = vpg.engine
    stop_fn = stop_fn or stop_critereon(0.10, 1e-5, 0.30)
    if reset_log_std:
        vpg.policy.reset_log_std()                                         # kwargs['reset_opt'] (training.py:350-352), :1119-1121

    def save():
        m, v, t = eng.get_policy_adam()
        return eng.get_policy().clone(), m.clone(), v.clone(), t

    def restore(snap):
        theta, m, v, t = snap
        eng.set_policy(theta)
        eng.set_policy_adam(m, v, t)
    snapshot = save()                                                      # saver.save, :1127-1129
    real = (lambda: float(real_cost_fn())) if real_cost_fn else (lambda: 0.0)
    est = lambda: eng.validation_cost(validation_init, T, gamma).cpu().numpy()
    min_costs = {'real': real(), 'trpo_mean': np.inf, 'estimated': est()}  # :1153-1163
    best_index, candidates, history = 0, {}, []
    j = 0
    for j in range(1, max_iters + 1):
        vpg.start_worker()                                                 # :1175
        paths = vpg.obtain_samples(j)
        samples_data = vpg.process_samples(j, paths)
        vpg.optimize_policy(j, samples_data)
        if j % log_every == 0:                                             # :1209
            candidates['trpo_mean'] = 0.0
            candidates['estimated'] = est()                                # :1239-1241
            candidates['real'] = real()
            history.append((j, float(np.mean(candidates['estimated']))))
            if logger:
                logger('iter %d est=%s' % (j, np.array_str(candidates['estimated'], precision=3)))
            if not is_done(mode, stop_fn, min_costs, candidates):          # :1286-1295
                best_index = j
                snapshot = save()
                update_stats(min_costs, candidates, whole)
            if j - best_index >= num_iters_threshold:                      # :1298
                break
    restore(snapshot)                                                      # log_and_restore, :1301/:1400
    return dict(best_index=best_index, last_index=j, min_validation_costs=min_costs, history=history)


def optimize_policy_svg(svg, validation_init, T, gamma, rollout_data=None, **loop_kwargs):
    """'svg' branch of model_based_rl.py:optimize_policy (:1204-1206) on the 'bptt' branch's loop (optimize_policy_bptt: snapshot, iterate, validate
    every log_every iterations, keep or restore theta).  Every iteration is one svg_update on the SAME rollout_data -- the reference feeds the one
    rollout_data of the outer iteration to every policy iteration -- and its training cost is 0.0 (:1206).  The reference's own loop breaks after the
    first validation round and restores the entry checkpoint (:1280-1282, :1400); that is not copied (see me-trpo_amd/svg.py)."""
    if rollout_data is not None:
        svg.rollout_data = rollout_data
    if svg.rollout_data is None:
        raise ValueError("the svg branch differentiates along recorded rollouts: pass rollout_data (collect_data's list of triplet lists, "
                         "svg.rollout_triplets) as init_pool, or set SVG.rollout_data")
    return optimize_policy_bptt(svg, validation_init, T, gamma, svg.rollout_data, **loop_kwargs)


def optimize_policy_bptt(bptt, validation_init, T, gamma, init_pool, mode='estimated', whole=True, log_every=5, num_iters_threshold=25,
                         max_iters=400, stop_fn=None, real_cost_fn=None, logger=None):
    """'bptt' / 'bptt-stochastic' branches of model_based_rl.py:optimize_policy (:1181-1196, 1209-1215, 1286-1298): every iteration
    `batch_size` reset states from `init_pool` (an InitStatePool or an env with reset()) and one BPTT step (stochastic as `bptt` is set:
    every 'bptt-stochastic' step sees the noise); every `log_every` iterations the K validation costs, deterministic as in the reference
    (which sets stochastic back to 0 first, :1211-1215); the stop rule and the snapshot / restore of the TRPO branch.  No reset_opt: the
    reference builds it for trpo / vpg only.  `mode` 'trpo_mean' has no TRPO sampler here and compares 0.0, as for the other branches."""
    if getattr(bptt, 'needs_init_pool', True) and (init_pool is None or not (hasattr(init_pool, 'sample') or hasattr(init_pool, 'reset'))):
        raise ValueError("the bptt branches draw their batch from init_pool: an InitStatePool or an env with reset() (from_params: "
                         "Setup.bptt_optimize_policy_kwargs carries it)")
    eng = bptt.engine
    stop_fn = stop_fn or stop_critereon(0.10, 1e-5, 0.30)
    snapshot = eng.get_policy().clone()
    real = (lambda: float(real_cost_fn())) if real_cost_fn else (lambda: 0.0)
    est = lambda: eng.validation_cost(validation_init, T, gamma).cpu().numpy()
    min_costs = {'real': real(), 'trpo_mean': np.inf, 'estimated': est()}
    best_index, candidates, history, training_costs = 0, {}, [], []
    j = 0
    for j in range(1, max_iters + 1):
        training_costs.append(float(bptt.optimize_policy_iteration(init_pool)))        # :1183-1196, np.squeeze(training_cost)
        if j % log_every == 0:                                             # :1209
            candidates['trpo_mean'] = 0.0
            candidates['estimated'] = est()
            candidates['real'] = real()
            history.append((j, float(np.mean(candidates['estimated']))))
            if logger:
                logger('iter %d training_cost=%.6g est=%s' % (j, training_costs[-1], np.array_str(candidates['estimated'], precision=3)))
            if not is_done(mode, stop_fn, min_costs, candidates):          # :1286-1295
                best_index = j
                snapshot = eng.get_policy().clone()
                update_stats(min_costs, candidates, whole)
            if j - best_index >= num_iters_threshold:                      # :1298
                break
    eng.set_policy(snapshot)
    return dict(best_index=best_index, last_index=j, min_validation_costs=min_costs, history=history, training_costs=training_costs)
