"""CPU checks of tests/ppo_ref.py, the float64 restatement of the 'ppo' update: its hand-written gradient against torch float64 autograd of
the loss as the issue states it (tf.minimum / tf.clip_by_value, entropy bonus, clamped log_std), with advantages of both signs, ratios on both
sides of both clip bounds, a clamped log_std slot, a nonzero entropy coefficient, and the tie lr = 1 (theta = theta_old)."""
import math

import numpy as np
import torch

import ppo_ref as R
from vpg_ref import LOG_MIN_STD


def _problem(dims=(6, 16, 12, 3), N=400, seed=5, move=0.08, clamped=True):
    rng = np.random.RandomState(seed)
    P = sum(i * j + j for i, j in zip(dims[:-1], dims[1:])) + dims[-1]
    th_old = rng.randn(P) * 0.3
    th_old[-dims[-1]:] = [-0.4, 0.3, -0.2]
    na, o_w = dims[-1], P - 2 * dims[-1] - dims[-2] * dims[-1]
    if clamped:                                                # the mean of the last action dim is its bias alone (see below)
        th_old[o_w:o_w + dims[-2] * na].reshape(dims[-2], na)[:, -1] = 0.0
    obs = rng.randn(N, dims[0])
    _, hs, _, ls = R.ratios(th_old, dims, obs, np.zeros((N, dims[-1])), np.zeros((N, dims[-1])), np.zeros(dims[-1]))
    old_mean, old_ls = hs[-1], np.broadcast_to(ls, hs[-1].shape).copy()
    act = old_mean + np.exp(old_ls) * rng.randn(N, dims[-1])
    adv = rng.randn(N)
    valid = rng.rand(N) > 0.2
    theta = th_old + move * rng.randn(P)
    if clamped:
        # the last log_std below log(1e-6): clamped, zero gradient.  At std = 1e-6 a mean that moves at all sends every ratio to 0 or inf, so
        # this dim's mean stays put (zero weight column, bias unmoved) and the old distribution sits at the clamp too: ratios stay O(1)
        theta[-1] = -20.0
        theta[o_w:o_w + dims[-2] * na].reshape(dims[-2], na)[:, -1] = 0.0
        theta[P - na - 1] = th_old[P - na - 1]
        old_ls[:, -1] = LOG_MIN_STD
        act[:, -1] = old_mean[:, -1] + 1e-6 * rng.randn(N)
    return th_old, theta, list(dims), obs, act, adv, old_mean, old_ls, valid


def autograd(theta, dims, obs, act, adv, old_mean, old_ls, clip_lr, ent_coeff, valid=None, n_global=None):
    T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    keep = torch.ones(len(adv), dtype=torch.bool) if valid is None else torch.as_tensor(np.asarray(valid).astype(bool))
    n = float(n_global if n_global is not None else keep.sum())
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    h, o = T(obs), 0
    for l, (i, j) in enumerate(zip(dims[:-1], dims[1:])):
        W = th[o:o + i * j].reshape(i, j); o += i * j
        h = h @ W + th[o:o + j]; o += j
        if l < len(dims) - 2:
            h = torch.tanh(h)
    ls = torch.clamp(th[o:], min=LOG_MIN_STD)
    na = dims[-1]
    logli = lambda m, s: -s.sum(-1) - 0.5 * (((T(act) - m) / torch.exp(s)) ** 2).sum(1) - 0.5 * na * math.log(2 * math.pi)
    lr = torch.exp(logli(h, ls.expand_as(h)) - logli(T(old_mean), T(np.broadcast_to(old_ls, old_mean.shape).copy())))
    A = T(adv)
    surr = torch.minimum(lr * A, torch.clamp(lr, 1.0 - clip_lr, 1.0 + clip_lr) * A)
    ent = ls.sum() + 0.5 * na * (1.0 + math.log(2 * math.pi))
    loss = -(surr * keep).sum() / n - ent_coeff * ent
    loss.backward()
    return float(loss.detach()), th.grad.numpy(), lr.detach().numpy()


def test_loss_grad_matches_autograd_with_both_gates_exercised():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem()
    c = 0.1
    for kw in (dict(), dict(valid=valid), dict(valid=valid, n_global=1000)):
        for ent in (0.0, 0.03):
            l1, g1, lr, gate = R.loss_grad(theta, dims, obs, act, adv, om, ols, c, ent, **kw)
            l2, g2, lr2 = autograd(theta, dims, obs, act, adv, om, ols, c, ent, **kw)
            np.testing.assert_allclose(lr, lr2, rtol=1e-10)
            assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
            np.testing.assert_allclose(g1, g2, rtol=1e-9, atol=1e-12)
            assert g1[-1] == 0.0 and g1[-3] != 0.0             # the clamped slot: no surrogate and no entropy gradient
    # every combination of (advantage sign, ratio below 1 - c / inside / above 1 + c) occurs, and the gate is what min / clip say
    lo, hi = lr < 1 - c, lr > 1 + c
    for pos in (adv > 0, adv < 0):
        for band in (lo, ~lo & ~hi, hi):
            assert (pos & band).sum() >= 5
    assert np.array_equal(gate, ~((adv > 0) & hi) & ~((adv < 0) & lo))
    assert 0.1 <= 1.0 - gate.mean() <= 0.9


def test_entropy_term_alone():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    l0, g0, _, _ = R.loss_grad(theta, dims, obs, act, adv, om, ols, 0.2, 0.0)
    l1, g1, _, _ = R.loss_grad(theta, dims, obs, act, adv, om, ols, 0.2, 0.5)
    na = dims[-1]
    H = theta[-na:].sum() + 0.5 * na * (1.0 + math.log(2 * math.pi))
    assert abs((l1 - l0) + 0.5 * H) <= 1e-12
    np.testing.assert_allclose(g1[:-na], g0[:-na], rtol=0, atol=0)
    np.testing.assert_allclose(g1[-na:] - g0[-na:], -0.5, rtol=1e-12)


def test_tie_at_ratio_one_goes_to_the_unclipped_branch():
    """theta = theta_old and the old distribution evaluated from it: lr = 1 exactly, lr A == clip(lr) A, and the whole gradient flows
    (tf.minimum passes the gradient to its first argument on a tie): it is the NPO surrogate's gradient whatever the clip."""
    th_old, _, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    for c in (0.3, 0.0):                                       # c = 0: every sample sits on BOTH bounds
        l1, g1, lr, gate = R.loss_grad(th_old, dims, obs, act, adv, om, ols, c, 0.0, valid=valid)
        assert np.all(lr == 1.0) and gate.all()
        l2, g2, _ = autograd(th_old, dims, obs, act, adv, om, ols, c, 0.0, valid=valid)
        l3, g3, _ = autograd(th_old, dims, obs, act, adv, om, ols, 1e9, 0.0, valid=valid)
        assert abs(l1 - l3) <= 1e-12 and abs(l1 - l2) <= 1e-12
        np.testing.assert_allclose(g1, g3, rtol=1e-9, atol=1e-12)
        if c > 0:                                              # (at c = 0 torch's own tie rules for clamp and minimum are not TF's: not compared)
            np.testing.assert_allclose(g1, g2, rtol=1e-9, atol=1e-12)


def test_adam_epochs_keeps_the_old_distribution_fixed():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(N=200, clamped=False)
    P = len(theta)
    th, m, v, t, losses = R.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, valid, n_epochs=4, lr=1e-2)
    assert t == 4 and len(losses) == 4
    assert losses[0] == R.loss_grad(th_old, dims, obs, act, adv, om, ols, 0.2, 0.01, valid)[0]
    assert np.all(np.diff(losses) < 0)                          # full-batch steps of 1e-2 from theta_old: the loss falls
    # second epoch's loss is the loss at the theta the first epoch produced, against the ORIGINAL old distribution
    th1, m1, v1, t1, _ = R.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, valid, n_epochs=1, lr=1e-2)
    assert losses[1] == R.loss_grad(th1, dims, obs, act, adv, om, ols, 0.2, 0.01, valid)[0]
