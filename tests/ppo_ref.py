"""Float64 NumPy restatement of the 'ppo' policy update, written from its formulas (algos/ppo.py:107-119 name the graph):

  * lr_n = exp(logli_theta(a_n | o_n) - logli_old(a_n | o_n)), logli = DiagonalGaussian.log_likelihood_sym of the UNCLIPPED stored action;
    the current log_std is clamped at log(1e-6) ([rllab] GaussianMLPPolicy min_std, as in the TRPO kernels), the old distribution is the
    batch's (old_mean, old_log_std) as stored;
  * loss = -mean_n min(lr_n A_n, clip(lr_n, 1 - c, 1 + c) A_n) - ent_coeff * mean_n H_n, H = sum_j ls_j + na / 2 (1 + log 2 pi) of the clamped
    log_std (the same for every sample), means over the valid samples;
  * the gradient follows tf.minimum / tf.clip_by_value: sample n contributes -A_n lr_n grad(logli_n) / N when lr_n A_n <= clip(lr_n) A_n (a
    tie goes to the unclipped branch) and nothing otherwise; the entropy term adds -ent_coeff on every unclamped log_std slot;
  * the optimiser: n_epochs full-batch tf.train.AdamOptimizer steps (vpg_ref.adam_step), the old distribution fixed while theta moves.

`valid` samples at 0 are left out of both the sums and the divisor unless n_global is given.  theta layout: vpg_ref's (metrpo_get_policy)."""
import math

import numpy as np

from vpg_ref import LOG_MIN_STD, adam_step

ENT_CONST = 0.5 * (1.0 + math.log(2.0 * math.pi))


def unflatten(theta, dims):
    theta = np.asarray(theta, dtype=np.float64)
    Ws, bs, o = [], [], 0
    for i, j in zip(dims[:-1], dims[1:]):
        Ws.append(theta[o:o + i * j].reshape(i, j)); o += i * j
        bs.append(theta[o:o + j]); o += j
    return Ws, bs, theta[o:o + dims[-1]]


def ratios(theta, dims, obs, act, old_mean, old_log_std):
    """Likelihood ratio of EVERY sample (valid or not) -> (lr [N], hidden activations, z, clamped log_std)."""
    obs, act, old_mean = (np.asarray(x, dtype=np.float64) for x in (obs, act, old_mean))
    Ws, bs, raw_ls = unflatten(theta, dims)
    hs = [obs]
    for l in range(len(Ws)):
        pre = hs[-1] @ Ws[l] + bs[l]
        hs.append(np.tanh(pre) if l < len(Ws) - 1 else pre)
    ls = np.maximum(raw_ls, LOG_MIN_STD)
    ols = np.broadcast_to(np.asarray(old_log_std, dtype=np.float64), old_mean.shape)
    z = (act - hs[-1]) * np.exp(-ls)
    zo = (act - old_mean) * np.exp(-ols)
    llr = ((ols - ls) + 0.5 * (zo * zo - z * z)).sum(1)
    return np.exp(llr), hs, z, ls


def loss_grad(theta, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff=0.0, valid=None, n_global=None):
    """-> (loss, grad [P], lr [N], gate [N] bool).  gate[n]: sample n is on the unclipped branch (it carries gradient); lr and gate cover
    every sample, the sums only the valid ones."""
    adv = np.asarray(adv, dtype=np.float64)
    keep = np.ones(len(adv), bool) if valid is None else np.asarray(valid).astype(bool)
    n = float(n_global if n_global is not None else keep.sum())
    Ws, bs, raw_ls = unflatten(theta, dims)
    lr, hs, z, ls = ratios(theta, dims, obs, act, old_mean, old_log_std)
    na = len(ls)
    un = lr * adv
    cl = np.clip(lr, 1.0 - clip_lr, 1.0 + clip_lr) * adv
    gate = un <= cl
    ent = ls.sum() + na * ENT_CONST
    loss = -(np.where(gate, un, cl) * keep).sum() / n - ent_coeff * ent
    w = np.where(gate & keep, -un / n, 0.0)                     # d loss / d logli_n
    d = w[:, None] * z * np.exp(-ls)                            # d logli / d mean = z / std
    dls = (w[:, None] * (z * z - 1.0)).sum(0) - ent_coeff       # d logli / d ls = z^2 - 1; d H / d ls = 1
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
    return float(loss), np.concatenate(parts + [dls]), lr, gate


def adam_epochs(theta, m, v, t, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff=0.0, valid=None, n_epochs=10, lr=1e-3,
                beta1=0.9, beta2=0.999, eps=1e-8):
    """n_epochs full-batch Adam steps on the PPO loss -> (theta, m, v, t, losses [n_epochs]); losses[e] is the loss at the theta entering epoch e."""
    losses = []
    for _ in range(n_epochs):
        loss, g, _, _ = loss_grad(theta, dims, obs, act, adv, old_mean, old_log_std, clip_lr, ent_coeff, valid)
        losses.append(loss)
        theta, m, v, t = adam_step(theta, m, v, t, g, lr=lr, beta1=beta1, beta2=beta2, eps=eps)
    return theta, m, v, t, np.array(losses)
