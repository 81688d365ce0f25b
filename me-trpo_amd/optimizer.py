"""[rllab] sandbox.rocky.tf.optimizers.conjugate_gradient_optimizer.ConjugateGradientOptimizer with
PerlmutterHvp and rllab.misc.krylov.cg, as wired by algos/trpo.py:18-20 (all defaults) and driven by
algos/npo.py:85-91 (update_opt) and :111 (optimize).

Two execution forms over the same kernels:
  fused=True  (default)  one C call (metrpo_trpo_update): CG vectors stay on the GPU in float64, the only
                         host synchronisation is the accept test of each line-search trial.
  fused=False            the reference-shaped host loop (NumPy float64 vectors, one kernel call per
                         f_loss / f_grad / f_Hx / f_loss_constraint evaluation).  Same arithmetic; used for
                         debugging and by the multi-process CPU tests with an injected evaluator.
subsample_factor < 1 ([rllab] optimize(): inds = np.random.choice(n, int(n * subsample_factor), replace=False)): loss, gradient and line search
see the whole batch; Hx -- the cg_iters products of krylov.cg and the d.Hd of the step scale -- sees the rows `inds` of it, gathered on the device
(Engine.subsample_batch), its mean KL being the mean over the subsample.  One draw per optimize() call, from a torch.Generator this optimiser owns
(seeded from `seed` and the rank; rllab draws from NumPy's global RNG on the host, which this cannot be pinned to: pass subsample_indices for that
stream).  Both execution forms build the same sub-batch and walk the same arithmetic.
Sharded runs: every evaluation returns this rank's pre-scaled share; a sum all-reduce (Comm) makes it the
global mean, so every rank walks the identical CG / line-search trajectory."""
import numpy as np
import torch

from .parallel import Comm


def cg(f_Ax, b, cg_iters=10, residual_tol=1e-10):
    """rllab.misc.krylov.cg"""
    p, r, x = b.copy(), b.copy(), np.zeros_like(b)
    rdotr = r.dot(r)
    for _ in range(cg_iters):
        z = f_Ax(p)
        v = rdotr / p.dot(z)
        x += v * p
        r -= v * z
        newrdotr = r.dot(r)
        mu = newrdotr / rdotr
        p = r + mu * p
        rdotr = newrdotr
        if rdotr < residual_tol:
            break
    return x


class EngineEvaluator(object):
    """f_loss/f_grad/f_Hx_plain/f_loss_constraint of the compiled graph, served by the HIP kernels."""

    def __init__(self, engine, batch, fvp_batch=None):
        self.engine, self.batch = engine, batch
        self.fvp_batch = batch if fvp_batch is None else fvp_batch      # what f_Hx_plain sees (subsample_inputs)

    @property
    def n_samples(self):
        return int(self.batch.N)

    def subsample(self, idx, comm=None):
        """f_Hx_plain sees the rows idx of the batch from now on (ConjugateGradientOptimizer.optimize with subsample_factor < 1)."""
        self.fvp_batch = build_sub_batch(self.engine, self.batch, idx, comm or Comm())

    def loss_grad(self):
        return self.engine.loss_grad(self.batch)                  # tensor [1+P] f64 (this rank's share)

    def hvp(self, v):
        return self.engine.fvp(self.fvp_batch, v)                 # tensor [P] f64

    def loss_constraint(self, theta):
        return self.engine.loss_kl(self.batch, theta)             # tensor [2] f64

    def get_params(self):
        return self.engine.get_policy().double().cpu().numpy()

    def set_params(self, theta):
        self.engine.set_policy(np.asarray(theta, dtype=np.float32))


def build_sub_batch(engine, batch, idx, comm):
    """The sub-batch of rows idx with the denominator of its means.  A batch known to be all valid on every rank (1 / inv_n_global == world * N: the
    fixed-horizon case of sampler.py) gives world * len(idx) without a host read; otherwise the gather's valid count is summed over the ranks and
    read once (the read the sampler already takes for those envs)."""
    m = int(idx.numel())
    if abs(1.0 / batch.inv_n_global - comm.world * int(batch.N)) < 0.5:
        return engine.subsample_batch(batch, idx, n_global_sub=comm.world * m)
    sub = engine.subsample_batch(batch, idx, n_global_sub=comm.world * m)      # (placeholder denominator, replaced below)
    n = int(comm.allreduce_sum_(sub.valid_count).item())
    if n == 0:
        raise ValueError("subsampled Hx: none of the gathered rows is valid on any rank (%d rows drawn here)" % m)
    sub.inv_n_global = 1.0 / n
    return sub


class ConjugateGradientOptimizer(object):
    def __init__(self, cg_iters=10, reg_coeff=1e-5, subsample_factor=1.0, backtrack_ratio=0.8, max_backtracks=15,
                 accept_violation=False, hvp_approach=None, num_slices=1, fused=True, seed=0):
        subsample_factor = float(subsample_factor)
        if not (0.0 < subsample_factor <= 1.0):
            raise ValueError("subsample_factor = %r: must be in (0, 1]" % (subsample_factor,))
        self._subsample_factor, self._seed = subsample_factor, int(seed)
        self._gen = None                     # torch.Generator of the subsample draws: made at the first draw, on the batch's device
        self._cg_iters, self._reg_coeff = cg_iters, reg_coeff
        self._backtrack_ratio, self._max_backtracks = backtrack_ratio, max_backtracks
        self._accept_violation, self._fused = accept_violation, fused
        self._max_constraint_val = None
        self._constraint_name = None
        self._last_diag = None
        self._open = None                    # engine whose update was only enqueued (optimize(..., defer=True)); finish() closes it
        self.spec_trials = 2                 # line-search trials decided on the device by a deferred update (the first two cover ~95 % of C1's updates)

    @property
    def pending(self):
        return self._open is not None

    @property
    def last_diag(self):
        """Diagnostics of the last optimize(); closes a deferred update first."""
        if self._open is not None:
            self.finish()
        return self._last_diag

    @last_diag.setter
    def last_diag(self, d):
        self._last_diag = d

    def finish(self):
        """Second half of optimize(..., defer=True): waits for the update, stores and returns its diagnostics.  diag['late'] is True
        when the policy changed only now (accepted at a later trial than the speculative ones): launches enqueued since optimize()
        used the previous policy."""
        if self._open is None:
            return self._last_diag
        eng, self._open = self._open, None
        self._last_diag = eng.trpo_update_end()
        return self._last_diag

    def update_opt(self, loss=None, target=None, leq_constraint=None, inputs=None, extra_inputs=None,
                   constraint_name="constraint", *args, **kwargs):
        """algos/npo.py:85-91: leq_constraint = (mean_kl, step_size); the symbolic loss/inputs of the
        reference have no counterpart here (the kernels implement that exact graph)."""
        constraint_term, constraint_value = leq_constraint
        self._max_constraint_val = float(constraint_value)
        self._constraint_name = constraint_name
        self._target = target

    # -- diagnostics the reference exposes (commented out at npo.py:106-120) ---------------------
    def loss(self, evaluator, comm=None):
        out = self._reduce(evaluator.loss_constraint(None), comm)
        return float(out[0])

    def constraint_val(self, evaluator, comm=None):
        out = self._reduce(evaluator.loss_constraint(None), comm)
        return float(out[1])

    @staticmethod
    def _reduce(t, comm):
        comm = comm or Comm()
        t = comm.allreduce_sum_(t)
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    def subsample_size(self, n_local):
        """m = int(n * subsample_factor) of rllab's optimize(); a factor that leaves no row raises."""
        m = int(n_local * self._subsample_factor)
        if m == 0:
            raise ValueError("subsample_factor = %r leaves no row of this rank's N = %d samples" % (self._subsample_factor, n_local))
        return m

    def draw_indices(self, n_local, device='cpu', rank=0):
        """np.random.choice(n, m, replace=False) of rllab's optimize(), as the head of a device permutation: int32 [m], no host read."""
        m = self.subsample_size(n_local)
        device = torch.device(device)
        if self._gen is None or self._gen.device.type != device.type:
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed((self._seed * 1000003 + 7919 * int(rank)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randperm(n_local, generator=self._gen, device=device)[:m].to(torch.int32)

    def optimize(self, engine_or_evaluator, batch=None, comm=None, defer=False, subsample_indices=None):
        """defer=True (fused form only): enqueue the update with its first `spec_trials` line-search trials decided on the device and
        return at once (None); finish() / last_diag complete it.  The caller may enqueue the next rollout in between (algos.BatchPolopt).
        subsample_indices: the rows Hx sees, instead of this call's draw (tests; callers who bring rllab's own np.random.choice stream)."""
        comm = comm or Comm()
        if self._open is not None:
            self.finish()
        if self._subsample_factor < 1.0 or subsample_indices is not None:
            return self._optimize_subsampled(engine_or_evaluator, batch, comm, defer, subsample_indices)
        if self._fused and batch is not None:
            # ranks > 1: the ctx's own RCCL communicator when one is attached (all-reduces issued from C), else a host callback
            need = comm.world > 1 or comm.always_reduce
            ar = (lambda t: comm.allreduce_sum_(t)) if (need and not getattr(engine_or_evaluator, 'comm_world', 0)) else None
            if defer and ar is None:
                engine_or_evaluator.trpo_update(
                    batch, max_kl=self._max_constraint_val, cg_iters=self._cg_iters, reg_coeff=self._reg_coeff,
                    backtrack_ratio=self._backtrack_ratio, max_backtracks=self._max_backtracks,
                    accept_violation=self._accept_violation, spec_trials=self.spec_trials)
                self._open = engine_or_evaluator
                return None
            self.last_diag = engine_or_evaluator.trpo_update(
                batch, max_kl=self._max_constraint_val, cg_iters=self._cg_iters, reg_coeff=self._reg_coeff,
                backtrack_ratio=self._backtrack_ratio, max_backtracks=self._max_backtracks,
                accept_violation=self._accept_violation, allreduce=ar)
            return self.last_diag
        ev = engine_or_evaluator if batch is None else EngineEvaluator(engine_or_evaluator, batch)
        self.last_diag = self._optimize_host(ev, comm)
        return self.last_diag

    def _optimize_subsampled(self, engine_or_evaluator, batch, comm, defer, indices):
        """optimize() with Hx on a sub-batch: one draw, one gather, then the same two forms."""
        ev = engine_or_evaluator if batch is None else None
        if ev is not None and not (hasattr(ev, 'n_samples') and hasattr(ev, 'subsample')):
            raise TypeError("subsampled Hx needs an evaluator with n_samples and subsample(idx, comm) (EngineEvaluator has them)")
        n_local = int(ev.n_samples) if ev is not None else int(batch.N)
        if indices is None:
            device = getattr(engine_or_evaluator, 'device', None) or getattr(getattr(ev, 'engine', None), 'device', 'cpu')
            indices = self.draw_indices(n_local, device=device, rank=comm.rank)
        else:
            indices = torch.as_tensor(indices).reshape(-1).to(torch.int32)
            if indices.numel() == 0:
                raise ValueError("subsample_indices is empty (N = %d)" % n_local)
        if ev is not None or not self._fused:
            if ev is None:
                ev = EngineEvaluator(engine_or_evaluator, batch)
            ev.subsample(indices, comm)
            self.last_diag = self._optimize_host(ev, comm)
            return self.last_diag
        eng = engine_or_evaluator
        sub = build_sub_batch(eng, batch, indices, comm)
        need = comm.world > 1 or comm.always_reduce
        ar = (lambda t: comm.allreduce_sum_(t)) if (need and not getattr(eng, 'comm_world', 0)) else None
        kw = dict(max_kl=self._max_constraint_val, cg_iters=self._cg_iters, reg_coeff=self._reg_coeff, backtrack_ratio=self._backtrack_ratio,
                  max_backtracks=self._max_backtracks, accept_violation=self._accept_violation, fvp_batch=sub)
        if defer and ar is None:
            eng.trpo_update(batch, spec_trials=self.spec_trials, **kw)
            self._open = eng
            return None
        self.last_diag = eng.trpo_update(batch, allreduce=ar, **kw)
        return self.last_diag

    def _optimize_host(self, ev, comm):
        """Line-by-line restatement of ConjugateGradientOptimizer.optimize."""
        prev_param = np.copy(ev.get_params())
        lg = self._reduce(ev.loss_grad(), comm)
        loss_before, flat_g = float(lg[0]), np.array(lg[1:], dtype=np.float64)

        def Hx(x):
            return self._reduce(ev.hvp(x), comm) + self._reg_coeff * x

        descent_direction = cg(Hx, flat_g, cg_iters=self._cg_iters)
        initial_step_size = np.sqrt(2.0 * self._max_constraint_val * (1. / (descent_direction.dot(Hx(descent_direction)) + 1e-8)))
        if np.isnan(initial_step_size):
            initial_step_size = 1.
        flat_descent_step = initial_step_size * descent_direction
        n_iter, loss, constraint_val = 0, np.nan, np.nan
        cur_param = prev_param
        for n_iter, ratio in enumerate(self._backtrack_ratio ** np.arange(self._max_backtracks)):
            cur_step = ratio * flat_descent_step
            cur_param = (prev_param - cur_step).astype(np.float32)
            lk = self._reduce(ev.loss_constraint(cur_param), comm)
            loss, constraint_val = float(lk[0]), float(lk[1])
            if loss < loss_before and constraint_val <= self._max_constraint_val:
                break
        accepted = True
        if (np.isnan(loss) or np.isnan(constraint_val) or loss >= loss_before or
                constraint_val >= self._max_constraint_val) and not self._accept_violation:
            accepted = False                       # "Line search condition violated. Rejecting the step!"
            ev.set_params(prev_param)
        else:
            ev.set_params(cur_param)
        return dict(loss_before=loss_before, loss=loss, kl=constraint_val, beta=float(initial_step_size),
                    n_backtrack=int(n_iter), accepted=accepted, g=flat_g, d=descent_direction)


class AdamOptimizer(object):
    """The optimiser algos/ppo.py:61-62 names (`AdamOptimizer()`) but never imports or defines; stated here: n_epochs full-batch
    tf.train.AdamOptimizer steps (beta1 0.9, beta2 0.999, epsilon 1e-8, no gradient clipping) on every policy parameter including log_std.
    The Adam state is the engine's policy optimizer state (Engine.get_policy_adam / set_policy_adam); it is never reset here, exactly as
    FirstOrderOptimizer treats it for VPG.  Minibatches (batch_size other than None) are not built.
    loss / optimize take PPO's KL penalty as kl_penalty and step_size (ppo.py:120-121; None: the loss without it)."""

    def __init__(self, learning_rate=1e-3, n_epochs=10, batch_size=None, beta1=0.9, beta2=0.999, epsilon=1e-8, **kwargs):
        if batch_size is not None:
            raise NotImplementedError("AdamOptimizer: full-batch epochs (batch_size=None) are the setting built")
        self.learning_rate, self.n_epochs, self.batch_size = float(learning_rate), int(n_epochs), batch_size
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.last_losses = None
        self._target = None

    def update_opt(self, loss, target, inputs, diagnostic_vars=None, **kwargs):
        self._target = target            # the loss graph itself (ppo.py:107-119) is what the HIP kernels compute

    @staticmethod
    def _kl_loss_grad(engine, batch, clip_lr, ent, kl_penalty, step_size, comm, need):
        """ppo_kl_loss_grad behind the global mean KL: a host-driven all-reduce sums loss_kl's share first and hands the result to the gradient call."""
        if need and not getattr(engine, 'comm_world', 0):
            mean_kl = comm.allreduce_sum_(engine.loss_kl(batch))[1:2]
            return engine.ppo_kl_loss_grad(batch, clip_lr, ent, kl_penalty, step_size, mean_kl=mean_kl)
        return engine.ppo_kl_loss_grad(batch, clip_lr, ent, kl_penalty, step_size)

    def loss(self, engine, batch, clip_lr, entropy_bonus_coeff, comm=None, kl_penalty=None, step_size=0.01):
        """ppo.py:169 / :177 optimizer.loss: the penalised clipped surrogate at the current theta, summed over the ranks (1-element tensor)."""
        comm = comm or Comm()
        need = comm.world > 1 or comm.always_reduce
        if kl_penalty is None:
            out = engine.ppo_loss_grad(batch, clip_lr, entropy_bonus_coeff / max(1, comm.world))[:1].clone()
        else:
            out = self._kl_loss_grad(engine, batch, clip_lr, entropy_bonus_coeff / max(1, comm.world), kl_penalty, step_size, comm, need)[:1].clone()
        return comm.allreduce_sum_(out) if need else out

    def optimize(self, engine, batch, clip_lr, entropy_bonus_coeff, comm=None, kl_penalty=None, step_size=0.01):
        """n_epochs Adam steps.  With a communicator attached to the engine (Comm.attach_engine) or at world size 1 the whole of it is
        Engine.ppo_update (no host involvement between the epochs); otherwise each epoch's gradient share is all-reduced on the host (Comm,
        e.g. gloo) and the step follows as Engine.policy_adam_step with no clipping.  -> the losses at the theta entering each epoch."""
        comm = comm or Comm()
        need = comm.world > 1 or comm.always_reduce
        if need and not getattr(engine, 'comm_world', 0):
            losses = []
            for _ in range(self.n_epochs):
                if kl_penalty is None:
                    lg = engine.ppo_loss_grad(batch, clip_lr, entropy_bonus_coeff / comm.world)
                else:                                   # the ranks' KL shares are summed first: the gate is taken on the global mean
                    lg = self._kl_loss_grad(engine, batch, clip_lr, entropy_bonus_coeff / comm.world, kl_penalty, step_size, comm, True)
                lg = comm.allreduce_sum_(lg)
                engine.policy_adam_step(lg[1:], self.learning_rate, clip_val=None, beta1=self.beta1, beta2=self.beta2, eps=self.epsilon)
                losses.append(lg[:1])
            self.last_losses = torch.cat(losses) if losses else torch.empty(0, dtype=torch.float64, device=engine.device)
        elif kl_penalty is not None:
            self.last_losses = engine.ppo_kl_update(batch, n_epochs=self.n_epochs, clip_lr=clip_lr, entropy_bonus_coeff=entropy_bonus_coeff,
                                                    kl_penalty=kl_penalty, step_size=step_size, lr=self.learning_rate, beta1=self.beta1,
                                                    beta2=self.beta2, eps=self.epsilon)
        else:
            self.last_losses = engine.ppo_update(batch, n_epochs=self.n_epochs, clip_lr=clip_lr, entropy_bonus_coeff=entropy_bonus_coeff,
                                                 lr=self.learning_rate, beta1=self.beta1, beta2=self.beta2, eps=self.epsilon)
        return self.last_losses
