"""Float64 torch restatement of the 'vpg' policy update (algos/vpg.py; training.py:337-352), written from its formulas:

  * surr_obj = -mean_n(logli_n * adv_n) (vpg.py:88) over the valid samples, logli = DiagonalGaussian.log_likelihood_sym of the UNCLIPPED
    stored action under the policy mean and log_std:  -sum(ls) - 0.5 sum(z^2) - 0.5 na log(2 pi),  z = (a - mean) exp(-ls),
    ls = max(log_std, log(1e-6)) ([rllab] GaussianMLPPolicy min_std, as in the TRPO kernels);
  * its gradient, back-propagated by hand through the tanh MLP (identity output layer); the log_std slots get zero where the clamp holds;
  * one tf.train.AdamOptimizer step (vpg.py:26-33: FirstOrderOptimizer with batch_size=None, max_epochs=1 -> one step on the whole batch):
    t += 1, lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, theta -= lr_t m / (sqrt(v) + eps).

Assumptions (rllab is not vendored): TF's Adam defaults (1e-3, 0.9, 0.999, 1e-8), no gradient clipping, every trainable policy variable
including log_std.  theta layout: W_0 [n_0][n_1] row-major, b_0, ..., W_{L-1}, b_{L-1}, log_std [na] (metrpo_get_policy)."""
import math

import numpy as np
import torch

LOG_MIN_STD = math.log(1e-6)


def unflatten(theta, dims):
    theta = torch.as_tensor(theta, dtype=torch.float64)
    Ws, bs, o = [], [], 0
    for i, j in zip(dims[:-1], dims[1:]):
        Ws.append(theta[o:o + i * j].reshape(i, j)); o += i * j
        bs.append(theta[o:o + j]); o += j
    return Ws, bs, theta[o:o + dims[-1]]


def _select(obs, act, adv, valid):
    obs, act, adv = (torch.as_tensor(x, dtype=torch.float64) for x in (obs, act, adv))
    if valid is not None:
        keep = torch.as_tensor(np.asarray(valid).astype(bool))
        obs, act, adv = obs[keep], act[keep], adv[keep]
    return obs, act, adv


def loss_grad(theta, dims, obs, act, adv, valid=None, n_global=None):
    """-> (loss, grad [P]) as float64 numpy, by the hand-written backward pass.  n_global: the divisor (default: valid samples)."""
    obs, act, adv = _select(obs, act, adv, valid)
    n = float(n_global if n_global is not None else obs.shape[0])
    Ws, bs, raw_ls = unflatten(theta, dims)
    hs = [obs]
    for l in range(len(Ws)):
        pre = hs[-1] @ Ws[l] + bs[l]
        hs.append(torch.tanh(pre) if l < len(Ws) - 1 else pre)
    mean = hs[-1]
    ls = torch.clamp(raw_ls, min=LOG_MIN_STD)
    z = (act - mean) * torch.exp(-ls)
    na = mean.shape[1]
    logli = -ls.sum() - 0.5 * (z * z).sum(1) - 0.5 * na * math.log(2 * math.pi)
    loss = -(logli * adv).sum() / n
    w = -adv / n                                               # d loss / d logli
    dmean = w[:, None] * z * torch.exp(-ls)                    # d logli / d mean = z / std
    dls = (w[:, None] * (z * z - 1.0)).sum(0)                  # d logli / d ls = z^2 - 1
    dls = torch.where(raw_ls > LOG_MIN_STD, dls, torch.zeros_like(dls))
    gW, gb = [None] * len(Ws), [None] * len(Ws)
    d = dmean
    for l in range(len(Ws) - 1, -1, -1):
        gW[l] = hs[l].T @ d
        gb[l] = d.sum(0)
        if l > 0:
            d = (d @ Ws[l].T) * (1.0 - hs[l] * hs[l])
    parts = []
    for W, b in zip(gW, gb):
        parts += [W.reshape(-1), b]
    return float(loss), torch.cat(parts + [dls]).numpy()


def loss_autograd(theta, dims, obs, act, adv, valid=None, n_global=None):
    """The same loss as a torch graph; -> (loss, grad) through autograd (the check of loss_grad's hand-written backward pass)."""
    obs, act, adv = _select(obs, act, adv, valid)
    n = float(n_global if n_global is not None else obs.shape[0])
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    Ws, bs, raw_ls = unflatten(th, dims)
    h = obs
    for l in range(len(Ws)):
        h = h @ Ws[l] + bs[l]
        if l < len(Ws) - 1:
            h = torch.tanh(h)
    ls = torch.clamp(raw_ls, min=LOG_MIN_STD)
    na = h.shape[1]
    logli = -ls.sum() - 0.5 * (((act - h) / torch.exp(ls)) ** 2).sum(1) - 0.5 * na * math.log(2 * math.pi)
    loss = -(logli * adv).sum() / n
    loss.backward()
    return float(loss.detach()), th.grad.numpy()


def adam_step(theta, m, v, t, g, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer.apply_gradients, float64 -> (theta, m, v, t)."""
    theta, m, v, g = (np.asarray(x, dtype=np.float64) for x in (theta, m, v, g))
    t = int(t) + 1
    lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return theta - lr_t * m / (np.sqrt(v) + eps), m, v, t
