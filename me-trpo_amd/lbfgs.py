"""The 'l-bfgs' branch of the reference's optimize_policy, on the device:

    model_based_rl.py:391-398     train_step = tf.contrib.opt.ScipyOptimizerInterface(training_policy_cost, var_list=<'training_policy'
                                  variables>, method='L-BFGS-B')   -- no options: scipy's defaults (maxcor 10, ftol 2.22e-9, gtol 1e-5,
                                  maxiter 15000, maxfun 15000, maxls 20)
    :1197-1202                    x_batch from env.reset(); train_step.minimize(sess, feed_dict={policy_training_init: x_batch});
                                  training_cost = sess.run(training_policy_cost, ...) at the final point
    run_model_based_rl.py:114-117 l_bfgs_exception: log_every = 1, max_iters = 1 (early_stop.optimize_policy applies it to an LBFGS object)

Every L-BFGS-B step runs in one kernel (csrc/lbfgs.hip) behind the BPTT cost and gradient (metrpo_bptt_grad); f and g reach it as TF
hands them to scipy (float32 values cast to float64) and each trial x reaches the policy as float32(x).  The host reads only the task word
of each step.  scipy is never imported."""
import numpy as np


_STATUS = {0: "START", 1: "NEW_X", 2: "RESTART", 3: "FG", 4: "CONVERGENCE", 5: "STOP", 6: "WARNING", 7: "ERROR", 8: "ABNORMAL"}
_TASK = {0: "", 401: "NORM OF PROJECTED GRADIENT <= PGTOL", 402: "RELATIVE REDUCTION OF F <= FACTR*EPSMCH",
         502: "TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT", 504: "TOTAL NO. OF ITERATIONS REACHED LIMIT"}


def task_message(task):
    """The message scipy's L-BFGS-B wrapper builds for a task (task[0], task[1])."""
    return _STATUS[task[0]] + ": " + _TASK.get(task[1], "")


class LbfgsResult(dict):
    __getattr__ = dict.__getitem__


class LBFGS(object):
    """ScipyOptimizerInterface(training_policy_cost, method='L-BFGS-B') over the engine's policy.  The keyword defaults are scipy's
    L-BFGS-B defaults; `lookahead` evaluations are kept in flight ahead of the host's read of a step's task (the result does not depend
    on it).  log_std is in var_list but its gradient is 0 (stochastic = 0), so it never moves."""

    def __init__(self, engine, T, gamma=1.0, batch_size=100, maxcor=10, ftol=2.220446049250313e-09, gtol=1e-5, maxiter=15000, maxfun=15000,
                 maxls=20, lookahead=2):
        self.engine, self.T, self.gamma, self.batch_size = engine, int(T), float(gamma), int(batch_size)
        self.maxcor, self.ftol, self.gtol = int(maxcor), float(ftol), float(gtol)
        self.maxiter, self.maxfun, self.maxls, self.lookahead = int(maxiter), int(maxfun), int(maxls), int(lookahead)
        self.result = None

    def opts(self):
        return self.engine.lbfgs_opts(m=self.maxcor, maxls=self.maxls, maxiter=self.maxiter, maxfun=self.maxfun, ftol=self.ftol,
                                      gtol=self.gtol, lookahead=self.lookahead, round_f32=True)

    def minimize(self, x_batch):
        """train_step.minimize: one whole L-BFGS-B run from the current policy on the cost of x_batch; the policy ends at float32 of the last
        accepted iterate.  -> result with fun, nit, nfev, status (0 converged / 1 limit / 2 abnormal), task and scipy's message."""
        r = self.engine.lbfgs_policy(x_batch, self.T, self.gamma, self.opts())
        r['message'] = task_message(r['task'])
        self.result = LbfgsResult(r)
        return self.result

    def optimize_policy_iteration(self, env_or_pool):
        """:1197-1202: fresh initial states, one minimize, then the training cost at the final point (a 0-d device tensor, float32 as TF's)."""
        if hasattr(env_or_pool, 'sample'):
            x_batch = env_or_pool.sample(self.batch_size)
        else:
            x_batch = np.array([env_or_pool.reset() for _ in range(self.batch_size)])
        self.minimize(x_batch)
        return self.engine.validation_cost(x_batch, self.T, self.gamma).mean().float()
