"""CPU checks of tests/ppo_kl_ref.py, the float64 restatement of the 'ppo' update with its KL penalty (ppo.py:120-121): loss and gradient against
torch float64 autograd of loss = [PPO loss] + beta * max(0, mean_kl - delta) with the gate open and closed, with a clamped log_std slot, a rank's
share under the global gate, and beta = 0 against ppo_ref exactly."""
import numpy as np
import torch

import ppo_kl_ref as K
import ppo_ref as R
from vpg_ref import LOG_MIN_STD
from test_ppo_ref import _problem, autograd as ppo_autograd


def autograd(theta, dims, obs, act, adv, old_mean, old_ls, clip_lr, ent_coeff, beta, delta, valid=None, n_global=None, kl_eps=0.0):
    """PPO's loss by test_ppo_ref.autograd plus beta * relu-like max(0, mean_kl - delta) by torch: -> (loss, grad, mean_kl)."""
    l0, g0, _ = ppo_autograd(theta, dims, obs, act, adv, old_mean, old_ls, clip_lr, ent_coeff, valid=valid, n_global=n_global)
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
    ols = T(np.broadcast_to(old_ls, old_mean.shape).copy())
    s2, os2, dm = torch.exp(2 * ls), torch.exp(2 * ols), T(old_mean) - h
    kl = ((dm * dm + os2 - s2) / (2 * s2 + kl_eps) + ls - ols).sum(1)
    mk = (kl * keep).sum() / n
    pen = beta * torch.clamp(mk - delta, min=0.0)
    pen.backward()
    # torch's clamp passes no gradient below min and the full gradient at or above it; MaximumGrad sends a tie to the constant: the cases keep off the tie
    return l0 + float(pen.detach()), g0 + th.grad.numpy(), float(mk.detach())


def test_loss_grad_matches_autograd_gate_open_and_closed():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    mk = K.mean_kl(theta, dims, obs, om, ols, valid)
    assert mk > 1e-3
    for kw in (dict(), dict(valid=valid), dict(valid=valid, n_global=int(valid.sum()))):
        mk = K.mean_kl(theta, dims, obs, om, ols, kl_eps=0.0, **kw)
        for delta, want_open in ((0.5 * mk, True), (2.0 * mk, False)):
            for beta, ent in ((3.0, 0.0), (0.7, 0.03)):
                l1, g1, info = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, ent, beta, delta, kl_eps=0.0, **kw)
                l2, g2, mk2 = autograd(theta, dims, obs, act, adv, om, ols, 0.1, ent, beta, delta, **kw)
                assert info['open'] is want_open and abs(info['mean_kl'] - mk2) <= 1e-12 * mk2
                assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
                np.testing.assert_allclose(g1, g2, rtol=1e-9, atol=1e-12)
                if want_open:
                    assert np.linalg.norm(g1 - info['g_ppo']) > 1e-3 * np.linalg.norm(info['g_ppo'])      # the penalty is not a no-op
                    # a clipped sample still carries its KL gradient: the KL part is the gradient of the mean over ALL valid samples
                    assert not info['clip_gate'].all()
                    np.testing.assert_allclose(g1 - info['g_ppo'], beta * info['g_kl'], rtol=1e-12, atol=1e-15)
                else:
                    l0, g0, _, _ = R.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, ent, **kw)
                    assert l1 == l0 and np.array_equal(g1, g0)


def test_rllab_kl_constant_moves_the_gradient_by_its_stated_share():
    """kl_sym's 1e-8 in the denominator is in the VALUE the restatement (and metrpo_loss_kl) reports; the derivatives are the exact KL's.  Against
    autograd of the formula with the constant the gradient differs by at most 1e-8 / (2 s_min^2) relative per element of the KL part."""
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    mk = K.mean_kl(theta, dims, obs, om, ols, valid)
    l1, g1, info = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.0, 2.0, 0.5 * mk, valid)
    l2, g2, _ = autograd(theta, dims, obs, act, adv, om, ols, 0.1, 0.0, 2.0, 0.5 * mk, valid=valid, kl_eps=1e-8)
    s2_min = np.exp(2.0 * theta[-dims[-1]:]).min()
    assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
    assert np.linalg.norm(g1 - g2) <= 2.0 * 1e-8 / (2.0 * s2_min) * np.linalg.norm(2.0 * info['g_kl'])


def test_clamped_log_std_slot():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=True)
    na = dims[-1]
    mk = K.mean_kl(theta, dims, obs, om, ols, valid, kl_eps=0.0)
    l1, g1, info = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.03, 2.0, 0.5 * mk, valid, kl_eps=0.0)
    l2, g2, _ = autograd(theta, dims, obs, act, adv, om, ols, 0.1, 0.03, 2.0, 0.5 * mk, valid=valid)
    assert info['open']
    assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
    np.testing.assert_allclose(g1, g2, rtol=1e-9, atol=1e-12)
    assert g1[-1] == 0.0 and info['g_kl'][-1] == 0.0 and np.all(info['g_kl'][-na:-1] != 0.0)


def test_beta_zero_is_ppo_ref_exactly():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    P = len(theta)
    for delta in (0.0, 1e9):
        l1, g1, _ = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.03, 0.0, delta, valid)
        l0, g0, _, _ = R.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.03, valid)
        assert l1 == l0 and np.array_equal(g1, g0)
        a = K.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, 0.0, delta, valid, n_epochs=3, lr=1e-2)
        b = R.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, valid, n_epochs=3, lr=1e-2)
        assert all(np.array_equal(x, y) for x, y in zip(a[:5], b))


def test_tie_goes_to_the_constant_and_the_global_mean_decides():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(clamped=False)
    mk = K.mean_kl(theta, dims, obs, om, ols, valid)
    l1, g1, info = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.0, 2.0, mk, valid)           # mean_kl - delta == 0: closed
    assert not info['open'] and np.array_equal(g1, info['g_ppo'])
    # two shards under the global gate: losses and gradients add up to the whole batch's; on its own share each shard's gate would be closed
    N, n = len(adv), int(valid.sum())
    delta = 0.75 * mk
    whole = K.loss_grad(theta, dims, obs, act, adv, om, ols, 0.1, 0.0, 2.0, delta, valid)
    assert whole[2]['open']
    tot_l, tot_g = 0.0, 0.0
    for lo, hi in ((0, N // 2), (N // 2, N)):
        sl = slice(lo, hi)
        alone = K.loss_grad(theta, dims, obs[sl], act[sl], adv[sl], om[sl], ols[sl], 0.1, 0.0, 2.0, delta, valid[sl], n_global=n)
        assert not alone[2]['open'] and alone[2]['mean_kl'] < delta
        part = K.loss_grad(theta, dims, obs[sl], act[sl], adv[sl], om[sl], ols[sl], 0.1, 0.0, 2.0, delta, valid[sl], n_global=n, mean_kl_global=mk)
        tot_l, tot_g = tot_l + part[0], tot_g + part[1]
    assert abs(tot_l - whole[0]) <= 1e-12 * max(1.0, abs(whole[0]))
    np.testing.assert_allclose(tot_g, whole[1], rtol=1e-9, atol=1e-12)


def test_adam_epochs_reports_the_mean_kl_entering_each_epoch():
    th_old, theta, dims, obs, act, adv, om, ols, valid = _problem(N=200, clamped=False)
    P = len(theta)
    th, m, v, t, losses, kls = K.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, 5.0, 1e-4, valid,
                                              n_epochs=4, lr=1e-2)
    assert t == 4 and len(losses) == len(kls) == 4
    assert kls[0] == 0.0 and kls[1] > 1e-4                       # from theta_old the gate is closed at epoch 0 and open from epoch 1 on ...
    free = K.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, 0.0, 1e-4, valid, n_epochs=4, lr=1e-2)[5]
    assert kls[1] == free[1] and kls[2] < free[2] and kls[3] < free[3]      # ... where the penalty holds the KL below the unpenalised run's
    th1 = K.adam_epochs(th_old, np.zeros(P), np.zeros(P), 0, dims, obs, act, adv, om, ols, 0.2, 0.01, 5.0, 1e-4, valid, n_epochs=1, lr=1e-2)[0]
    assert kls[1] == K.mean_kl(th1, dims, obs, om, ols, valid)
