"""Float64 side of the subsampled TRPO update (tests/test_gpu_subsample_fvp.py, tests/test_subsample_host.py), CPU only: [rllab]
ConjugateGradientOptimizer.optimize with subsample_factor < 1 restated over the oracle's own functions -- loss_before, the gradient and every
line-search trial on the whole batch, Hx = f_Hx_plain(inputs[inds]) + reg_coeff x inside krylov.cg and in d.Hx(d)."""
import numpy as np
from oracle import metrpo_oracle as O
import tolerances as TOL


def cg_optimize_sub(theta, dims, obs, act, adv, om, ols, idx=None, valid=None, max_kl=0.01, cg_iters=10, reg_coeff=1e-5, backtrack_ratio=0.8,
                    max_backtracks=15):
    """O.cg_optimize with the Fisher-vector products on the rows `idx` (None: all).  `valid` (uint8 [N] or None): invalid rows are left out of
    both sides, as the reference drops unfinished paths before the optimiser sees them.  Also returns every trial's (loss, kl) and `clear`:
    each trial's accept test is decided with room to spare (see is_clear)."""
    obs, act, adv, om, ols = (np.asarray(x, np.float64) for x in (obs, act, adv, om, ols))
    keep = np.ones(len(obs), bool) if valid is None else np.asarray(valid).astype(bool)
    full = tuple(x[keep] for x in (obs, act, adv, om, ols))
    if idx is None:
        fobs = full[0]
    else:
        idx = np.asarray(idx).astype(np.int64)
        fobs = obs[idx][keep[idx]]
    prev = np.asarray(theta, np.float64).copy()
    loss_before, g = O.surrogate_loss_grad(prev, dims, *full)
    Hx = lambda x: O.fisher_vector_product(prev, dims, fobs, x, reg_coeff)
    d = O.cg(Hx, g, cg_iters=cg_iters)
    beta = np.sqrt(2.0 * max_kl * (1.0 / (d.dot(Hx(d)) + 1e-8)))
    if np.isnan(beta):
        beta = 1.0
    step = beta * d
    trials, n_iter, loss, kl, cur = [], 0, np.nan, np.nan, prev
    for n_iter, ratio in enumerate(backtrack_ratio ** np.arange(max_backtracks)):
        cur = prev - ratio * step
        loss, kl = O.surrogate_loss_kl(cur, dims, *full)
        trials.append((float(loss), float(kl)))
        if loss < loss_before and kl <= max_kl:
            break
    accepted = not (np.isnan(loss) or np.isnan(kl) or loss >= loss_before or kl >= max_kl)
    if not accepted:
        cur = prev
    return dict(theta_new=cur, loss_before=float(loss_before), g=g, d=d, beta=float(beta), n_backtrack=int(n_iter), loss=float(loss), kl=float(kl),
                accepted=accepted, trials=trials, clear=is_clear(trials, float(loss_before), max_kl), n_fvp_rows=len(fobs))


def is_clear(trials, loss_before, max_kl):
    """Is every trial's accept test away from a tie?  The device's loss and KL at a trial theta are held to POST_UPDATE_RTOL of the oracle's, so a
    comparison is safe when its two sides differ by more than twice that: |kl - max_kl| > 2 rtol max_kl and |loss - loss_before| > 2 rtol max(|loss|,
    |loss_before|).  A rejected trial needs only ONE of its two failing comparisons to be clear, an accepted one both."""
    r = 2.0 * TOL.POST_UPDATE_RTOL
    for loss, kl in trials:
        loss_gap = abs(loss - loss_before) > r * max(abs(loss), abs(loss_before))
        kl_gap = abs(kl - max_kl) > r * max_kl
        ok = loss < loss_before and kl <= max_kl
        if ok and not (loss_gap and kl_gap):
            return False
        if not ok and not ((loss >= loss_before and loss_gap) or (kl > max_kl and kl_gap)):
            return False
    return True
