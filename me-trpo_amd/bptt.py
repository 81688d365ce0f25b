"""BPTT policy optimisation -- the 'bptt' branch of the reference's optimize_policy:

    model_based_rl.py:1181-1187   x_batch = np.array([env.reset() for i in range(batch_size)])
                                  _, training_cost = sess.run([policy_opt_op, training_policy_cost], {policy_training_init: x_batch})
    :106-151, :365                training_policy_cost = mean_i sum_t gamma^t cost_tf(x_t, clip(policy(x_t)), model_i(x_t, u_t))
    :186-195, utils.py:262-276    policy_opt_op = Adam(learning_rate) on the per-variable clip_by_norm'ed gradient

and the 'bptt-stochastic' branch (:1188-1196): the same update with policy noise in the unrolled graph, u = clip(mean + eps * exp(log_std))
(training.py:115-116), which also trains log_std.  The reference runs set_stochastic[1] and policy_opt_op in one session.run without a control
dependency, so whether its step sees the noise is unspecified; here every stochastic step does (stochastic = 1).

The unrolled forward, its reverse sweep, the parameter-gradient reduction and the Adam step all run in libmetrpo.so
(csrc/bptt.hip + the gradient kernels of the TRPO update); nothing is differentiated by a framework."""
import numpy as np
import torch


class BPTT(object):
    """policy_opt_params of the reference: T, gamma, learning_rate, grad_norm_clipping, batch_size.  stochastic=True: the
    'bptt-stochastic' branch; the Philox key of step n is `seed` * 1000003 + n (a running per-object counter, as sampler.py keys its
    rollouts), never the iteration number of the caller."""

    def __init__(self, engine, T, gamma=1.0, learning_rate=1e-3, grad_norm_clipping=None, batch_size=100, stochastic=False, seed=0):
        self.engine, self.T, self.gamma = engine, int(T), float(gamma)
        self.learning_rate, self.grad_norm_clipping, self.batch_size = float(learning_rate), grad_norm_clipping, int(batch_size)
        self.stochastic, self.seed, self._draws = bool(stochastic), int(seed), 0
        self.n_saturates = None                                      # [B, na] int32 of the last stochastic step (model_based_rl.py:1212)
        engine.policy_adam_reset()                                   # sess.run(policy_adam_init)

    def reset_optimizer(self):
        self.engine.policy_adam_reset()

    def training_cost_and_grad(self, x_batch):
        if not self.stochastic:
            return self.engine.bptt_grad(x_batch, self.T, self.gamma)
        key = (self.seed * 1000003 + self._draws) & 0xFFFFFFFFFFFFFFFF
        self._draws += 1
        costs, grad, self.n_saturates = self.engine.bptt_grad_stochastic(x_batch, self.T, self.gamma, seed=key, n_saturates=True)
        return costs, grad

    def step(self, x_batch):
        """One sess.run([policy_opt_op, training_policy_cost]): returns the training cost evaluated BEFORE the update (a 0-d device
        tensor; `float()` it to synchronise, as np.squeeze(training_cost) does in the reference)."""
        costs, grad = self.training_cost_and_grad(x_batch)
        self.engine.policy_adam_step(grad, self.learning_rate, self.grad_norm_clipping)
        return costs.mean()

    def optimize_policy_iteration(self, env_or_pool):
        """:1183: fresh initial states from the real env's reset() (or an InitStatePool), then one step."""
        if hasattr(env_or_pool, 'sample'):
            x_batch = env_or_pool.sample(self.batch_size)
        else:
            x_batch = np.array([env_or_pool.reset() for _ in range(self.batch_size)])
        return self.step(x_batch)
