"""CPU checks of tests/score_grad_ref.py (the float64 restatement of metrpo_score_actions_grad) and of tests/score_grad_cases.py (the case table and
kink guard of tests/test_gpu_score_grad.py), without the library:
  * the restatement against torch float64 autograd of the unrolled return, per env, with a masked Ant case and stop_at_done = False;
  * against central differences of score_actions_ref.score_actions;
  * against a one-step case worked out by hand;
  * its float32 mode uses a small share of every bound the GPU test holds (printed; below 0.25);
  * each wrong restatement misses a bound by a wide factor (printed)."""
import numpy as np
import pytest
import torch

from oracle import metrpo_oracle as O
import score_actions_ref as SA
import score_grad_ref as R
import score_grad_cases as SC


def case(path, env, variant='plain', stop=True, T=11):
    return next(c for c in SC.CASES if c.path == path and c.env == env and c.variant == variant and c.stop == stop and c.T == T and c.dh == (64, 64))


ENV_CASES = [case('fused', env) for env in SC.FUSED_ENVS] + [case('fused', 'ant', 'ant_plant'), case('fused', 'ant', stop=False),
                                                            next(c for c in SC.CASES if c.env == 'humanoid'), next(c for c in SC.CASES if c.act == 'tanh')]


def torch_return_grad(dm, env, init, actions, gamma, stop, ref):
    """Autograd of sum_b R[k][b] per head: the unrolled return written in torch float64, the mask and the weights taken from the restatement as constants."""
    t64 = lambda x: torch.as_tensor(np.asarray(x, np.float64))
    T, B = actions.shape[:2]
    ns = dm.ns
    grads, lams, rets = [], [], []
    for k in range(dm.K):
        a = t64(actions).requires_grad_(True)
        s0 = t64(SA.start_rows(init, B)).requires_grad_(True)
        x, total = s0, 0.0
        for t in range(T):
            u = torch.clamp(a[t], -1.0, 1.0)
            h = ((torch.cat([x, u], dim=1) - t64(dm.in_mean)) / t64(dm.in_std))[:, dm.n_drop:]
            for l in range(len(dm.Ws)):
                h = h @ t64(dm.Ws[l][k]) + t64(dm.bs[l][k])
                if l < len(dm.Ws) - 1:
                    h = torch.relu(h) if dm.acts[l] == 'relu' else torch.tanh(h)
            xn = t64(dm.diff_mean[:ns]) + t64(dm.diff_std[:ns]) * h + x
            su2 = (u ** 2).sum(dim=1)
            if env == 'swimmer':
                c = -(xn[:, 5] - 1e-2 * (u ** 2).mean(dim=1))
            elif env == 'half_cheetah':
                c = -torch.clamp(xn[:, 9] - 1e-1 * 0.5 * su2, -10, 10)
            elif env == 'ant':
                c = -(xn[:, 15] - 1e-2 * 0.5 * su2 + 0.05)
            elif env == 'humanoid':
                c = (xn[:, -1] - 1.5) ** 2 + 1e-2 * 1e-3 * su2
            elif env == 'hopper':
                c = -(xn[:, 5] - 0.01 * 0.5 * su2 - 10 * torch.relu(0.45 - xn[:, 0]) - 10 * torch.relu(xn[:, 1].abs() - .2)
                      - torch.relu(xn[:, 2:].abs() - 100).sum(dim=1))
            elif env == 'snake':
                c = -(xn[:, 7] - 1e-2 * 0.5 * su2)
            total = total - t64(ref['w'][k, t]) * c
            x = xn
        total.sum().backward()
        grads.append(a.grad.numpy()); lams.append(s0.grad.numpy()); rets.append(total.detach().numpy())
    return np.stack(rets), np.stack(grads), np.stack(lams)


@pytest.mark.parametrize('c', ENV_CASES, ids=[c.id for c in ENV_CASES])
def test_restatement_is_autograd_of_the_unrolled_return(c):
    d = SC.case_data(c)
    ref = SC.reference(d)
    ret, grad, lam = torch_return_grad(d['dm'], c.env, d['init'], d['actions'], c.gamma, c.stop, ref)
    rel = lambda a, b: float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    # the weights of the restatement are fp32-rounded gamma^t (the header's rule) while its ret sums float64 gamma^t: compare ret with those weights
    ret_w = (ref['w'] * ref['rew']).sum(axis=1)
    print("%s: grad %.3g, lam0 %.3g, ret %.3g relative" % (c.id, rel(ref['grad'], grad), rel(ref['lam0'], lam), rel(ret_w, ret)))
    assert rel(ref['grad'], grad) <= 1e-9 and rel(ref['lam0'], lam) <= 1e-9 and rel(ret_w, ret) <= 1e-9
    sa = SA.score_actions(d['dm'], c.env, d['init'], d['actions'], gamma=c.gamma, stop_at_done=c.stop)
    assert np.array_equal(ref['len'], sa['len']) and np.allclose(ref['ret'], sa['ret'], rtol=1e-13, atol=1e-13)       # R is metrpo_score_actions' ret
    if c.variant == 'ant_plant':                               # candidates end at assorted steps: some at once, some mid-horizon, some never
        assert (ref['len'] == 1).any() and ((ref['len'] > 1) & (ref['len'] < c.T)).any() and (ref['len'] == c.T).any()
        behind = np.arange(c.T)[None, :, None] >= ref['len'][:, None, :]
        assert np.all(ref['grad'][behind] == 0)
    if c.env == 'ant' and not c.stop:
        assert np.all(ref['len'] == c.T)
    clipped = np.abs(d['actions']) > 1
    assert clipped.any() and np.all(ref['grad'][:, clipped] == 0)


def test_restatement_against_central_differences():
    c = case('fused', 'hopper')
    d = SC.case_data(c)
    dm, init = d['dm'], d['init']
    actions = d['actions'][:3, :6].copy()                      # T = 3, B = 6, S = 3
    ref = R.score_actions_grad(dm, c.env, init, actions, c.gamma, c.stop)
    h = 1e-6
    worst = 0.0
    for t in range(3):
        for j in range(dm.na):
            ap, am = actions.copy(), actions.copy()
            ap[t, :, j] += h; am[t, :, j] -= h
            fd = (SA.score_actions(dm, c.env, init, ap, c.gamma, c.stop)['ret'] - SA.score_actions(dm, c.env, init, am, c.gamma, c.stop)['ret']) / (2 * h)
            inside = np.abs(np.abs(actions[t, :, j]) - 1) > 10 * h
            # ret sums float64 gamma^t, the gradient's weights are fp32(gamma^t): 6e-8 relative apart
            err = np.abs(fd - ref['grad'][:, t, :, j])[:, inside] / (np.abs(ref['grad'][:, t, :, j])[:, inside] + 1e-3)
            worst = max(worst, float(err.max()))
    for i in range(dm.ns):
        ip, im = init.copy(), init.copy()
        ip[:, i] += h; im[:, i] -= h
        fd = (SA.score_actions(dm, c.env, ip, actions, c.gamma, c.stop)['ret'] - SA.score_actions(dm, c.env, im, actions, c.gamma, c.stop)['ret']) / (2 * h)
        worst = max(worst, float((np.abs(fd - ref['lam0'][:, :, i]) / (np.abs(ref['lam0'][:, :, i]) + 1e-3)).max()))
    print("central differences: worst relative difference %.3g" % worst)
    assert worst < 1e-5


def test_hand_computed_one_step_case():
    """Swimmer with a head that is one linear layer: R = x'_5 - 0.01 mean(u^2), x' = diff_mean + diff_std ([(x, u) - m) / s][2:] W + b) + x."""
    ns, na, nd = 10, 2, 2
    rng = np.random.RandomState(3)
    W, b = rng.randn(1, ns + na - nd, ns), rng.randn(1, ns)
    m, s = rng.randn(ns + na), 0.5 + rng.rand(ns + na)
    dmean, dstd = rng.randn(ns), 0.1 + rng.rand(ns)
    dm = O.DynamicsEnsemble([W], [b], [], m, s, dmean, dstd, nd, ns, na)
    init = rng.randn(1, ns)
    actions = np.array([[[0.3, -0.6], [1.7, 0.2]]])            # T = 1, B = 2; candidate 1's first action is clipped
    out = R.score_actions_grad(dm, 'swimmer', init, actions, gamma=0.9, stop_at_done=True)
    u = np.clip(actions[0], -1, 1)
    want_g = np.stack([dstd[5] * W[0, ns - nd + j, 5] / s[ns + j] - 0.01 * 2 * u[:, j] / na for j in range(na)], axis=1)
    want_g[1, 0] = 0.0
    want_l = np.array([(1.0 if i == 5 else 0.0) + (dstd[5] * W[0, i - nd, 5] / s[i] if i >= nd else 0.0) for i in range(ns)])
    xn = dmean + dstd * (((np.concatenate([np.repeat(init, 2, axis=0), u], axis=1) - m) / s)[:, nd:] @ W[0] + b[0]) + init
    np.testing.assert_allclose(out['grad'][0, 0], want_g, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out['lam0'][0], np.stack([want_l, want_l]), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(out['ret'][0], xn[:, 5] - 0.01 * np.mean(u ** 2, axis=1), rtol=1e-12)
    assert np.array_equal(out['len'], [[1, 1]]) and np.array_equal(out['grad_mean'], out['grad'][0])


def uses(got, ref, c):
    """Worst share of the bounds of tests/test_gpu_score_grad.py over the heads: (grad whole, per step, per candidate, lam0 whole, per candidate, ret)"""
    return SC.shares(got, ref, c)


def test_case_table_and_kink_guard():
    ids = [c.id for c in SC.CASES]
    assert len(set(ids)) == len(ids)
    fused = [c for c in SC.CASES if c.path == 'fused']
    assert {c.env for c in fused} == set(SC.FUSED_ENVS) and {c.K for c in fused} >= {1, 5, 8, 9} and {c.B for c in fused} == set(SC.SIZES_B)
    assert {c.T for c in fused} == {1, 2, 11} and {c.gamma for c in fused} == {1.0, 0.99} and {c.stop for c in fused} == {True, False}
    assert any(c.S == 1 for c in fused) and any(c.S == 3 for c in fused) and any(c.S == c.B > 1 for c in fused) and any(max(c.dh) < 64 for c in fused)
    worst = 0.0
    for c in SC.CASES:
        d = SC.case_data(c)
        assert d['accepted'] == c.B and d['replaced'] <= SC.MAX_REPLACED * c.B, (c.id, d['replaced'], d['accepted'])
        assert d['margin'] >= SC.KINK_FACTOR
        a = np.abs(d['actions'])
        assert (a > 1).any() and (a < 1).any(), c.id           # the clip gate is exercised, and not everything is gated away
        worst = max(worst, d['replaced'] / float(c.B))
    print("kink guard: at most %.3f of a case's candidates replaced" % worst)


F32_CASES = [case('fused', env) for env in SC.FUSED_ENVS] + [case('fused', 'ant', 'ant_plant')]


def test_float32_restatement_uses_a_small_share_of_every_bound():
    worst = np.zeros(6)
    for c in F32_CASES:
        d = SC.case_data(c)
        ref = SC.reference(d)
        got = R.walk(d['dm'], c.env, d['init'], d['actions'], c.gamma, c.stop, dtype=np.float32)
        assert np.array_equal(got['len'], ref['len'])
        worst = np.maximum(worst, uses(got, ref, c))
    print("float32 restatement, shares of the bounds: grad whole %.3g, per step %.3g, per candidate %.3g; lam0 whole %.3g, per candidate %.3g; ret %.3g"
          % tuple(worst))
    assert worst.max() < 0.25


@pytest.mark.parametrize('mut', R.MUTS)
def test_wrong_restatements_miss_a_bound_by_a_wide_factor(mut):
    c = case('fused', 'ant', 'ant_plant') if mut == 'mask_first' else case('fused', 'half_cheetah')
    d = SC.case_data(c)
    ref = SC.reference(d)
    got = R.walk(d['dm'], c.env, d['init'], d['actions'], c.gamma, c.stop, mut=mut)
    factor = float(np.max(uses(got, ref, c)[:5]))
    print("%s: misses a gradient bound by a factor %.3g" % (mut, factor))
    assert factor > 10.0
