"""algos/batch_polopt.py, algos/npo.py, algos/trpo.py, algos/vpg.py, algos/ppo.py of the reference with the same constructor
arguments, attributes and methods (start_worker / obtain_samples / process_samples /
optimize_policy), so that the reference's outer loop (model_based_rl.py:1171-1180) drives them
unchanged:

    algo.start_worker(); paths = algo.obtain_samples(j); samples_data = algo.process_samples(j, paths)
    algo.optimize_policy(j, samples_data)
"""
import numpy as np

from .optimizer import ConjugateGradientOptimizer, AdamOptimizer
from .parallel import Comm
from .sampler import VectorizedSampler
from .tracing import PhaseTimers


class BatchPolopt(object):
    def __init__(self, env, policy, baseline, scope=None, n_itr=500, start_itr=0, batch_size=5000,
                 max_path_length=500, discount=0.99, gae_lambda=1, plot=False, pause_for_plot=False,
                 center_adv=True, positive_adv=False, store_paths=False, whole_paths=True, fixed_horizon=False,
                 sampler_cls=None, sampler_args=None, force_batch_sampler=False, comm=None, seed=0, **kwargs):
        self.env, self.policy, self.baseline = env, policy, baseline
        self.scope, self.n_itr, self.start_itr = scope, n_itr, start_itr
        self.batch_size, self.max_path_length = batch_size, max_path_length
        self.discount, self.gae_lambda = discount, gae_lambda
        self.plot, self.pause_for_plot = plot, pause_for_plot
        self.center_adv, self.positive_adv = center_adv, positive_adv
        self.store_paths, self.whole_paths, self.fixed_horizon = store_paths, whole_paths, fixed_horizon
        self.kwargs = kwargs
        self.engine = policy.engine
        self.comm = comm or Comm()
        # Sharded runs: `batch_size` and the sampler's n_envs are PER RANK (the job collects world x batch_size samples; weak
        # scaling).  The stop rule of early-terminating envs (sampler._obtain_until_enough) is applied by every rank to its own
        # envs against this per-rank batch_size -- divide by comm.world beforehand for a fixed global batch.
        self.seed = seed
        self.timers = PhaseTimers()          # rollout / process / policy_opt GPU times (tracing.py); off until .enable()
        assert not force_batch_sampler, "BatchSampler is unreachable on this path (batch_polopt.py:86-90)"
        if sampler_cls is None:
            assert self.policy.vectorized
            sampler_cls = VectorizedSampler
        if sampler_args is None:
            sampler_args = dict()
        self.sampler = sampler_cls(self, **sampler_args)
        self.init_opt()

    def start_worker(self):
        self.sampler.start_worker()

    def shutdown_worker(self):
        self.sampler.shutdown_worker()

    def obtain_samples(self, itr, determ=False, **kw):
        with self.timers.phase('rollout'):
            paths = self.sampler.obtain_samples(itr, determ, **kw)
            # async_line_search: the previous optimize_policy only ENQUEUED its update (the accept test of the first line-search trials
            # runs on the device), so the rollout above went out without the host waiting for it.  Now the update is closed; in the rare
            # case that it was accepted at a later trial than the speculative ones, the policy changed after the rollout was enqueued
            # and the rollout is repeated -- results are those of the synchronous order, always.
            opt = getattr(self, 'optimizer', None)
            if opt is not None and getattr(opt, 'pending', False):
                if opt.finish().get('late'):
                    paths = self.sampler.obtain_samples(itr, determ, **kw)
            return paths

    def process_samples(self, itr, paths):
        with self.timers.phase('process'):
            return self.sampler.process_samples(itr, paths)

    def init_opt(self):
        raise NotImplementedError

    def optimize_policy(self, itr, samples_data):
        raise NotImplementedError


class NPO(BatchPolopt):
    """Natural Policy Optimization (algos/npo.py)."""

    def __init__(self, optimizer=None, optimizer_args=None, step_size=0.01, **kwargs):
        if optimizer is None:
            raise NotImplementedError("PenaltyLbfgsOptimizer (NPO's default, npo.py:24) is outside the hot path; "
                                      "use TRPO or pass an optimizer")
        self.optimizer = optimizer
        self.step_size = step_size
        super(NPO, self).__init__(**kwargs)

    def init_opt(self):
        # npo.py:85-91; the surrogate / mean-KL graph itself (npo.py:68-75) is what the HIP kernels compute
        self.optimizer.update_opt(loss=None, target=self.policy, leq_constraint=(None, self.step_size),
                                  inputs=None, constraint_name="mean_kl")
        return dict()

    def optimize_policy(self, itr, samples_data):
        """npo.py:95-121: inputs = (observations, actions, advantages, agent_infos[mean], agent_infos[log_std])."""
        agent_infos = samples_data["agent_infos"]
        batch = self.engine.make_batch(samples_data["observations"], samples_data["actions"], samples_data["advantages"],
                                       agent_infos["mean"], agent_infos["log_std"], valid=samples_data.get("valids"),
                                       n_global=samples_data.get("n_valid_global"))
        with self.timers.phase('policy_opt'):
            # async_line_search (off by default: the reference decides every trial on the host): see obtain_samples
            self.optimizer.optimize(self.engine, batch, comm=self.comm, defer=bool(getattr(self, 'async_line_search', False)))
        if hasattr(self.sampler, 'finish_baseline_fit') and not getattr(self, 'defer_baseline_fit', False):
            self.sampler.finish_baseline_fit()
        return dict()

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)


class TRPO(NPO):
    """Trust Region Policy Optimization (algos/trpo.py)."""

    def __init__(self, optimizer=None, optimizer_args=None, **kwargs):
        if optimizer is None:
            if optimizer_args is None:
                optimizer_args = dict()
            optimizer = ConjugateGradientOptimizer(**optimizer_args)
        super(TRPO, self).__init__(optimizer=optimizer, **kwargs)


class FirstOrderOptimizer(object):
    """[rllab] sandbox.rocky.tf.optimizers.first_order_optimizer.FirstOrderOptimizer as VPG builds it (vpg.py:26-33): tf_optimizer_cls =
    tf.train.AdamOptimizer(learning_rate=1e-3) with TF's defaults (beta1 0.9, beta2 0.999, epsilon 1e-8), no gradient clipping.
    batch_size=None and max_epochs=1 make every optimize() ONE step on the gradient of the whole batch; the loss before / after the
    epoch feeds only a tolerance break that cannot fire with one epoch (and VPG's LossBefore / LossAfter logging is commented out,
    vpg.py:119-124), so only the loss at the entry theta -- free from the gradient pass -- is kept (`last_loss`, a device tensor).
    The Adam state is the engine's policy optimizer state (Engine.get_policy_adam / set_policy_adam); it is never reset here."""

    def __init__(self, tf_optimizer_cls=None, tf_optimizer_args=None, max_epochs=1, tolerance=1e-6, batch_size=None, callback=None,
                 verbose=False, learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, **kwargs):
        if tf_optimizer_cls is not None:
            raise NotImplementedError("FirstOrderOptimizer: only the AdamOptimizer VPG builds runs on this path")
        if max_epochs != 1 or batch_size is not None:
            raise NotImplementedError("FirstOrderOptimizer: VPG's setting (batch_size=None, max_epochs=1) is the one built")
        args = dict(learning_rate=learning_rate, beta1=beta1, beta2=beta2, epsilon=epsilon)
        args.update(tf_optimizer_args or {})
        self.learning_rate, self.beta1, self.beta2, self.epsilon = (float(args['learning_rate']), float(args['beta1']), float(args['beta2']),
                                                                    float(args['epsilon']))
        self.max_epochs, self.tolerance, self.batch_size = max_epochs, tolerance, batch_size
        self.last_loss = None

    def update_opt(self, loss, target, inputs, extra_inputs=None, **kwargs):
        self._target = target            # the surrogate graph itself (vpg.py:88) is what the HIP kernels compute

    def optimize(self, engine, batch, comm=None):
        """One Adam step.  With a communicator attached to the engine (Comm.attach_engine) or at world size 1 the whole step is
        Engine.vpg_update (gradient kernel + reduction carrying the step); otherwise the gradient share is all-reduced on the host
        (Comm, e.g. gloo) and the step follows as Engine.policy_adam_step with no clipping."""
        comm = comm or Comm()
        need = comm.world > 1 or comm.always_reduce
        if need and not getattr(engine, 'comm_world', 0):
            lg = comm.allreduce_sum_(engine.vpg_loss_grad(batch))
            engine.policy_adam_step(lg[1:], self.learning_rate, clip_val=None, beta1=self.beta1, beta2=self.beta2, eps=self.epsilon)
            self.last_loss = lg[:1]
        else:
            self.last_loss = engine.vpg_update(batch, lr=self.learning_rate, beta1=self.beta1, beta2=self.beta2, eps=self.epsilon)
        return self.last_loss


class VPG(BatchPolopt):
    """Vanilla Policy Gradient (algos/vpg.py): surr_obj = -mean(logli * adv) (vpg.py:88), minimised by a FirstOrderOptimizer with
    batch_size=None, max_epochs=1 -- one Adam step per optimize_policy.  process_samples is BatchPolopt's (linear baseline, gae_lambda 1,
    center_adv), as for TRPO."""

    def __init__(self, env, policy, baseline, optimizer=None, optimizer_args=None, **kwargs):
        if optimizer is None:
            default_args = dict(batch_size=None, max_epochs=1)
            optimizer_args = default_args if optimizer_args is None else dict(default_args, **optimizer_args)
            optimizer = FirstOrderOptimizer(**optimizer_args)
        self.optimizer = optimizer
        self.opt_info = None
        super(VPG, self).__init__(env=env, policy=policy, baseline=baseline, **kwargs)

    def init_opt(self):
        self.optimizer.update_opt(loss=None, target=self.policy, inputs=None)
        self.opt_info = dict()

    def optimize_policy(self, itr, samples_data):
        """vpg.py:100-118: inputs = (observations, actions, advantages); the old distribution is not an input."""
        batch = self.engine.make_batch(samples_data["observations"], samples_data["actions"], samples_data["advantages"], None, None,
                                       valid=samples_data.get("valids"), n_global=samples_data.get("n_valid_global"))
        with self.timers.phase('policy_opt'):
            self.optimizer.optimize(self.engine, batch, comm=self.comm)
        if hasattr(self.sampler, 'finish_baseline_fit') and not getattr(self, 'defer_baseline_fit', False):
            self.sampler.finish_baseline_fit()
        return dict()

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)


class PPO(BatchPolopt):
    """Proximal Policy Optimization (algos/ppo.py) with the reference's constructor signature.  The loss is ppo.py:107-119's clipped
    likelihood-ratio surrogate with the entropy bonus; the optimiser ppo.py:61-62 names is never defined there and is optimizer.AdamOptimizer
    here.  use_kl_penalty=True adds ppo.py:120-121's kl_penalty * max(0, mean_kl - step_size): self.kl_penalty (the TF variable kl_penalty_var,
    a float32 that starts at initial_kl_penalty) and self.step_size go to the optimiser with every call; f_increase_penalty / f_decrease_penalty /
    f_reset_penalty do ppo.py:133-153's arithmetic on it -- the reference never calls them, and neither does any loop here.  It needs a policy
    whose engine has the penalty's entry points (Engine.ppo_kl_update / ppo_kl_loss_grad) and raises NotImplementedError without one.  The other
    arguments the reference's constructor stores and never reads (use_line_search, max_backtracks, backtrack_ratio, min_n_epochs,
    adaptive_learning_rate, max / min_learning_rate, gradient_clipping, log_loss_kl_before / _after) are stored and not acted on, as there.  Recurrent policies are out of scope (ppo.py:103)."""

    def __init__(self, clip_lr=0.3, increase_penalty_factor=2, decrease_penalty_factor=0.5, min_penalty=1e-3, max_penalty=1e6,
                 entropy_bonus_coeff=0., gradient_clipping=40., log_loss_kl_before=True, log_loss_kl_after=True, use_kl_penalty=False,
                 initial_kl_penalty=1., use_line_search=True, max_backtracks=10, backtrack_ratio=0.5, optimizer=None, step_size=0.01,
                 min_n_epochs=2, adaptive_learning_rate=False, max_learning_rate=1e-3, min_learning_rate=1e-5, **kwargs):
        if use_kl_penalty:
            # the penalty runs in the engine's OP_PPOKL kernels: refuse, before anything is built, where there is no engine that has them (no policy, an
            # engine object of another kind) instead of failing at the first optimize_policy
            eng = getattr(kwargs.get('policy'), 'engine', None)
            if not (hasattr(eng, 'ppo_kl_update') and hasattr(eng, 'ppo_kl_loss_grad')):
                raise NotImplementedError("PPO: use_kl_penalty (ppo.py:120-121) needs a policy whose engine has ppo_kl_update / ppo_kl_loss_grad "
                                          "(metrpo_amd.Engine); got engine %r" % (eng,))
        self.clip_lr, self.entropy_bonus_coeff = clip_lr, entropy_bonus_coeff
        self.increase_penalty_factor, self.decrease_penalty_factor = increase_penalty_factor, decrease_penalty_factor
        self.min_penalty, self.max_penalty, self.initial_kl_penalty = min_penalty, max_penalty, initial_kl_penalty
        self.gradient_clipping = gradient_clipping
        self.log_loss_kl_before, self.log_loss_kl_after = log_loss_kl_before, log_loss_kl_after
        self.use_kl_penalty, self.use_line_search = use_kl_penalty, use_line_search
        self.max_backtracks, self.backtrack_ratio, self.step_size = max_backtracks, backtrack_ratio, step_size
        self.min_n_epochs, self.adaptive_learning_rate = min_n_epochs, adaptive_learning_rate
        self.max_learning_rate, self.min_learning_rate = max_learning_rate, min_learning_rate
        if kwargs.get('policy') is not None and getattr(kwargs['policy'], 'recurrent', False):
            raise NotImplementedError("PPO: recurrent policies are out of scope (ppo.py:103 asserts the same)")
        if optimizer is None:
            optimizer = AdamOptimizer()
        self.optimizer = optimizer
        self.opt_info = None
        self.kl_penalty = float(np.float32(initial_kl_penalty))      # kl_penalty_var (a float32 TF variable)
        super(PPO, self).__init__(**kwargs)

    # ppo.py:133-153: assignments to kl_penalty_var, computed and stored in float32 as TF does; each returns the new value
    def f_increase_penalty(self):
        self.kl_penalty = float(np.minimum(np.float32(self.kl_penalty) * np.float32(self.increase_penalty_factor), np.float32(self.max_penalty)))
        return self.kl_penalty

    def f_decrease_penalty(self):
        self.kl_penalty = float(np.maximum(np.float32(self.kl_penalty) * np.float32(self.decrease_penalty_factor), np.float32(self.min_penalty)))
        return self.kl_penalty

    def f_reset_penalty(self):
        self.kl_penalty = float(np.float32(self.initial_kl_penalty))
        return self.kl_penalty

    def _penalty_args(self):
        return dict(kl_penalty=self.kl_penalty, step_size=self.step_size) if self.use_kl_penalty else dict()

    def init_opt(self):
        self.optimizer.update_opt(loss=None, target=self.policy, inputs=None)
        self.opt_info = dict()
        return dict()

    def optimize_policy(self, itr, samples_data):
        """ppo.py:157-183: inputs = (observations, actions, advantages, agent_infos[mean], agent_infos[log_std]); loss and mean KL before,
        optimizer.optimize, mean KL and loss after (both losses with the KL penalty under use_kl_penalty).  The reference computes the five diagnostics and returns an empty dict (its record_tabular
        lines are commented out); they are returned here, as 1-element device tensors (no synchronisation)."""
        agent_infos = samples_data["agent_infos"]
        batch = self.engine.make_batch(samples_data["observations"], samples_data["actions"], samples_data["advantages"],
                                       agent_infos["mean"], agent_infos["log_std"], valid=samples_data.get("valids"),
                                       n_global=samples_data.get("n_valid_global"))
        eng, comm = self.engine, self.comm
        reduce_ = (lambda t: comm.allreduce_sum_(t)) if (comm.world > 1 or comm.always_reduce) else (lambda t: t)
        with self.timers.phase('policy_opt'):
            lk_before = reduce_(eng.loss_kl(batch))                              # [unclipped surrogate, mean KL] at the entry theta
            losses = self.optimizer.optimize(eng, batch, self.clip_lr, self.entropy_bonus_coeff, comm=comm, **self._penalty_args())
            lk_after = reduce_(eng.loss_kl(batch))
            loss_after = self.optimizer.loss(eng, batch, self.clip_lr, self.entropy_bonus_coeff, comm=comm, **self._penalty_args())
        if hasattr(self.sampler, 'finish_baseline_fit') and not getattr(self, 'defer_baseline_fit', False):
            self.sampler.finish_baseline_fit()
        loss_before = losses[:1] if len(losses) else loss_after
        return dict(LossBefore=loss_before, LossAfter=loss_after, MeanKLBefore=lk_before[1:2], MeanKL=lk_after[1:2], UnclippedSurrLoss=lk_after[:1])

    def get_itr_snapshot(self, itr, samples_data):
        return dict(itr=itr, policy=self.policy, baseline=self.baseline, env=self.env)
