"""Float64 NumPy restatement of the 'ppo' update with its KL penalty (algos/ppo.py:120-121, use_kl_penalty), built on tests/ppo_ref.py:

  * kl_n = DiagonalGaussian.kl_sym(old, new) of sample n = sum_j (dm_j^2 + s_old_j^2 - s_j^2) / (2 s_j^2 + kl_eps) + ls_j - ols_j with
    dm = old_mean - mean, s = exp(ls), ls the log_std clamped at log(1e-6); kl_eps = 1e-8 is rllab's constant (the value metrpo_loss_kl returns);
    mean_kl = mean over the valid samples;
  * loss = ppo_ref's loss + beta * max(0, mean_kl - delta);
  * the gate is TF's MaximumGrad: the penalty carries gradient iff mean_kl - delta > 0, strictly; it is taken on `mean_kl_global` when that is
    given (a rank's share of a sharded batch: the mean over ALL ranks' samples decides);
  * gate open: sample n adds beta / N * d kl_n / d theta, with the derivatives as include/metrpo.h states them (those of the exact KL, kl_eps = 0):
    d kl / d mean_j = (mean_j - old_mean_j) / s_j^2, d kl / d ls_j = 1 - (s_old_j^2 + dm_j^2) / s_j^2, zero on a clamped log_std slot; a sample
    whose surrogate is clipped still carries it; under the open gate the loss term is sum_n beta / N (kl_n - delta) over this call's samples, so
    that the ranks' losses add up to the global loss;
  * the optimiser: ppo_ref's Adam epochs, the mean KL re-evaluated at the theta entering each epoch.

With beta = 0 every result equals ppo_ref's exactly."""
import numpy as np

import ppo_ref as R
from vpg_ref import LOG_MIN_STD, adam_step


def kl_terms(theta, dims, obs, old_mean, old_log_std, kl_eps=1e-8):
    """-> (kl [N] of every sample, hidden activations, clamped log_std, dm [N, na], s2 [na], os2 [N, na])."""
    obs, old_mean = np.asarray(obs, dtype=np.float64), np.asarray(old_mean, dtype=np.float64)
    Ws, bs, raw_ls = R.unflatten(theta, dims)
    hs = [obs]
    for l in range(len(Ws)):
        pre = hs[-1] @ Ws[l] + bs[l]
        hs.append(np.tanh(pre) if l < len(Ws) - 1 else pre)
    ls = np.maximum(raw_ls, LOG_MIN_STD)
    ols = np.broadcast_to(np.asarray(old_log_std, dtype=np.float64), old_mean.shape)
    s2, os2, dm = np.exp(2.0 * ls), np.exp(2.0 * ols), old_mean - hs[-1]
    kl = ((dm * dm + os2 - s2) / (2.0 * s2 + kl_eps) + ls - ols).sum(1)
    return kl, hs, ls, dm, s2, os2


def mean_kl(theta, dims, obs, old_mean, old_log_std, valid=None, n_global=None, kl_eps=1e-8):
    kl = kl_terms(theta, dims, obs, old_mean, old_log_std, kl_eps)[0]
    keep = np.ones(len(kl), bool) if valid is None else np.asarray(valid).astype(bool)
    n = float(n_global if n_global is not None else keep.sum())
    return float((kl * keep).sum() / n)


def kl_grad(theta, dims, obs, old_mean, old_log_std, valid=None, n_global=None):
    """Gradient of the mean KL (exact KL: no kl_eps) -> grad [P]."""
    kl, hs, ls, dm, s2, os2 = kl_terms(theta, dims, obs, old_mean, old_log_std)
    keep = np.ones(len(kl), bool) if valid is None else np.asarray(valid).astype(bool)
    n = float(n_global if n_global is not None else keep.sum())
    Ws, bs, raw_ls = R.unflatten(theta, dims)
    w = keep[:, None] / n
    d = w * (-dm) / s2                                          # d kl / d mean = (mean - old_mean) / s^2
    dls = (w * (1.0 - (os2 + dm * dm) / s2)).sum(0)
    dls = np.where(raw_ls > LOG_MIN_STD, dls, 0.0)
    gW, gb = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        gW[l] = hs[l].T @ d
        gb[l] = d.sum(0)
        if l > 0:
            d = (d @ Ws[l].T) * (1.0 - hs[l] * hs[l])
    parts = []
    for W, b in zip(gW, gb):
        parts += [W.reshape(-1), b]
    return np.concatenate(parts + [dls])


def loss_grad(theta, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff=0.0, kl_penalty=1.0, step_size=0.01, valid=None,
              n_global=None, mean_kl_global=None, kl_eps=1e-8):
    """-> (loss, grad [P], info).  info: mean_kl (this call's share), open (the gate), g_ppo / g_kl (the surrogate + entropy gradient and the
    gradient of the mean KL, before kl_penalty), lr, clip_gate."""
    l0, g0, lr, gate = R.loss_grad(theta, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff, valid, n_global)
    mk = mean_kl(theta, dims, obs, old_mean, old_log_std, valid, n_global, kl_eps)
    decide = mk if mean_kl_global is None else float(mean_kl_global)
    is_open = decide - step_size > 0.0
    gk = kl_grad(theta, dims, obs, old_mean, old_log_std, valid, n_global)
    info = dict(mean_kl=mk, open=is_open, g_ppo=g0, g_kl=gk, lr=lr, clip_gate=gate)
    if not is_open:
        return l0, g0, info
    keep = np.ones(len(lr), bool) if valid is None else np.asarray(valid).astype(bool)
    n = float(n_global if n_global is not None else keep.sum())
    share = keep.sum() / n                                      # sum_n 1 / N over this call's samples (1 unless n_global says the batch is a shard)
    return l0 + kl_penalty * (mk - step_size * share), g0 + kl_penalty * gk, info


def adam_epochs(theta, m, v, t, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff=0.0, kl_penalty=1.0, step_size=0.01, valid=None,
                n_epochs=10, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """-> (theta, m, v, t, losses [n_epochs], mean_kls [n_epochs]): entry e of both belongs to the theta entering epoch e."""
    losses, kls = [], []
    for _ in range(n_epochs):
        loss, g, info = loss_grad(theta, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff, kl_penalty, step_size, valid)
        losses.append(loss); kls.append(info['mean_kl'])
        theta, m, v, t = adam_step(theta, m, v, t, g, lr=lr, beta1=beta1, beta2=beta2, eps=eps)
    return theta, m, v, t, np.array(losses), np.array(kls)
