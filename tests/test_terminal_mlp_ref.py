"""CPU tests of the MLP terminal value's float64 side (tests/terminal_mlp_ref.py, tests/terminal_mlp_cases.py) and of its host code
(metrpo_amd.planning.ValueMLP, value_targets, ShootingController(terminal_value=ValueMLP)): the table meets the kink guard's cap, the bounds have room
for fp32 arithmetic and none for a wrong restatement, the gradients are those of the return, and the host side does what it says -- without the
library."""
import numpy as np
import pytest
import torch

import terminal_mlp_cases as MC
import terminal_mlp_ref as R
import terminal_value_cases as TC

# the share of every bound the float32 walk (the device's number format, NumPy's summation order) may use: the rest is the device's own orders
F32_SHARE = 0.1


def test_the_table_meets_the_redraw_cap():
    worst = 0.0
    for case, loop in MC.RUNS:
        d = MC.case_data(case, loop)
        assert d['accepted'] == case.B, (case.id, loop, d['accepted'], d['replaced'])
        assert d['replaced'] <= MC.MAX_REPLACED * case.B, (case.id, loop, d['replaced'])
        assert d['margin'] >= MC.KINK_FACTOR
        worst = max(worst, d['replaced'] / case.B)
    print("worst share of candidates redrawn: %.3g" % worst)


def test_the_table_holds_what_it_says():
    ids = [c.id for c in MC.CASES]
    assert len(set(ids)) == len(ids) and len(MC.CASES) == len(TC.CASES)
    assert MC.KINK_FACTOR == 16.0 and MC.MAX_REPLACED == 0.25
    for path in ('fused', 'generic'):
        cs = [c for c in MC.CASES if c.path == path]
        assert {c.B for c in cs if c.env == 'swimmer' and c.T == 2 and c.calls == 'all'} >= {1, 15, 16, 17, 33}
        assert {c.B for c in cs if c.calls == 'grad'} == {63, 64, 65}
        assert any(c.T == 1 for c in cs) and {c.K for c in cs} >= {1, 5, 9}
        assert {c.env for c in cs if (c.B, c.T, c.S, c.nb) == (33, 11, 3, 3)} >= set(MC.FUSED_ENVS)
        assert any(c.dh == (48, 48) for c in cs) and any(not c.stop for c in cs) and any(c.gamma == 1.0 for c in cs)
        assert any(c.variant == 'tv_far' for c in cs) and any(not c.noise for c in cs)
        assert {c.in_std for c in cs} == {False, True}
        assert {c.hid for c in cs} == {(32, 32), (17, 5), (1, 1), (32, 8)}
    assert {c.env for c in MC.CASES if c.path == 'generic' and (c.dh != (64, 64) or c.act != 'relu')} >= {'humanoid', 'swimmer', 'half_cheetah'}
    # Ant: a done at the first step, in the middle, at the last step (no bootstrap there either), and never
    for case in (c for c in MC.CASES if c.variant == 'ant_plant'):
        for loop in MC.LOOPS:
            ref = MC.reference(MC.case_data(case, loop))
            n, T, wT = ref['len'], case.T, ref['wT']
            assert (n == 1).any() and ((n > 1) & (n < T)).any() and ((n == T) & (wT == 0)).any() and ((n == T) & (wT != 0)).any(), (case.id, loop)
    # tv_far: the value's clip acts on some dims of some candidates and not on others
    for case in (c for c in MC.CASES if c.variant == 'tv_far'):
        site = MC.reference(MC.case_data(case, 'open'))['sites']['tv_clip']
        assert (site > 0).any() and (site < 0).all(axis=1).any()


def test_without_a_value_the_walk_is_the_quadratic_restatements_walk():
    for case in (c for c in MC.CASES if c.path == 'fused' and c.T == 11 and c.noise):
        for loop in MC.LOOPS:
            d = MC.case_data(case, loop)
            a = MC.walk(d, tv=None)
            b = TC.R.walk(d['dm'], case.env, d['init'], d['seq'], None, **MC.walk_kw(case, loop, d['theta'], d['pdims']))
            for w in ('ret', 'len', 'grad', 'lam0', 'act'):
                assert np.array_equal(a[w], b[w]), (case.id, loop, w)


def test_the_float32_walk_uses_a_stated_share_of_every_bound():
    worst = np.zeros(6)
    for case, loop in MC.RUNS:
        d = MC.case_data(case, loop)
        ref = MC.reference(d)
        w32 = MC.walk(d, dtype=np.float32)
        assert np.array_equal(w32['len'], ref['len'])
        use = MC.shares(w32, ref, case)
        assert use.max() <= F32_SHARE, (case.id, loop, use)
        worst = np.maximum(worst, use)
    print("float32 walk, worst shares (grad whole / step / candidate, lam0 whole / candidate, ret):", worst)


@pytest.mark.parametrize('mut', R.MUTS)
def test_every_mutation_exceeds_a_bound(mut):
    caught = []
    for case, loop in MC.RUNS:
        if case.path != 'fused' or (mut == 'tv_no_policy_path' and loop == 'open'):
            continue
        d = MC.case_data(case, loop)
        use = MC.shares(MC.walk(d, mut=mut), MC.reference(d), case)
        if use.max() > 1.0:
            caught.append((case.id, loop, float(use.max())))
    print("%s: caught on %d runs, worst share %.3g" % (mut, len(caught), max([c[2] for c in caught] or [0.0])))
    assert caught, mut


@pytest.mark.parametrize('loop', MC.LOOPS)
def test_float64_gradients_are_those_of_the_return(loop):
    """grad and lam0 against central differences of the float64 return along a random direction, per head and candidate (per start state for
    lam0: a start state's candidates move together), on the candidates whose every kink argument is at least CLEAR away from its kink: the step
    moves an argument by a few eps."""
    eps, CLEAR, rng = 1e-7, 1e-5, np.random.RandomState(3)
    picked = [c for c in MC.CASES if c.path == 'fused' and c.noise and (c.variant in ('tv_far', 'ant_plant') or (c.T == 11 and c.env in ('hopper', 'half_cheetah'))
                                                                         or (c.env == 'swimmer' and c.B == 17 and c.K == 5))]
    assert len(picked) >= 6 and len({c.hid for c in picked}) >= 3
    for case in picked:
        d = MC.case_data(case, loop)
        ref = MC.reference(d)
        da = rng.randn(*d['seq'].shape); ds = rng.randn(*d['init'].shape)
        clear = np.min([np.abs(v).min(axis=1) for v in ref['sites'].values()], axis=0) >= CLEAR
        assert clear.sum() >= (case.B + 3) // 4, (case.id, loop, clear.sum())

        def ret_at(seq, init):
            return R.walk(d['dm'], case.env, init, seq, d['tv'], grad=False, **MC.walk_kw(case, loop, d['theta'], d['pdims']))['ret']
        num_a = (ret_at(d['seq'] + eps * da, d['init']) - ret_at(d['seq'] - eps * da, d['init'])) / (2 * eps)              # [K, B]
        ana_a = np.einsum('ktbd,tbd->kb', ref['grad'], da)
        num_s = (ret_at(d['seq'], d['init'] + eps * ds) - ret_at(d['seq'], d['init'] - eps * ds)) / (2 * eps)
        ana_s = np.einsum('kbd,bd->kb', ref['lam0'], np.repeat(ds, case.B // case.S, axis=0))
        for num, ana in ((num_a, ana_a), (num_s, ana_s)):
            scale = np.abs(ana).max()
            assert np.abs(num - ana)[:, clear].max() <= 1e-6 * scale + 1e-7, (case.id, loop, np.abs(num - ana)[:, clear].max(), scale)


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------------
def _net(ns, hid, seed):
    from metrpo_amd import planning as P
    rng = np.random.RandomState(seed)
    tv = MC.draw_net(rng, ns, hid, 1)
    net = P.ValueMLP(ns, hid)
    net.W0, net.b0, net.W1, net.b1, net.W2, net.b2 = (torch.as_tensor(np.asarray(x, np.float64)) for x in tv[:6])
    return net, tv


@pytest.mark.parametrize('hid', MC.WIDTHS, ids=lambda h: '%dx%d' % h)
def test_value_mlp_predict_is_the_restatement_and_packed_folds_the_normaliser(hid):
    from metrpo_amd import planning as P
    ns = 7
    net, tv = _net(ns, hid, 0)
    rng = np.random.RandomState(1)
    s = rng.randn(40, ns) * 6.0                                                       # some entries beyond the clip
    want = R.value_terms(tv[:6] + (np.zeros(1),), s, 1)[0]
    np.testing.assert_allclose(net.predict(s).numpy(), want, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(net.packed().numpy(), R.pack(tv))                    # no normaliser: the arrays as they are, rounded to fp32
    assert net.packed().dtype == torch.float32 and net.packed().shape == (ns * hid[0] + hid[0] + hid[0] * hid[1] + 2 * hid[1] + 1,)
    net.bias = 0.75
    np.testing.assert_allclose(net.predict(s).numpy(), want + 0.75, rtol=1e-13, atol=1e-13)
    net.bias = 0.0
    # with a normaliser: the folded net, evaluated WITHOUT one in float64, is the unfolded net to rounding
    net.mean, net.std = torch.as_tensor(rng.randn(ns)), torch.as_tensor(0.5 + rng.rand(ns))
    o = np.clip(s, -10, 10)
    x = (o - net.mean.numpy()) / net.std.numpy()
    direct = np.tanh(np.tanh(x @ tv[0].astype(np.float64) + tv[1]) @ tv[2].astype(np.float64) + tv[3]) @ tv[4].astype(np.float64) + tv[5]
    np.testing.assert_allclose(net.predict(s).numpy(), direct, rtol=1e-13, atol=1e-13)
    dev = net.W0.device
    W0f = net.W0 / net.std.to(dev)[:, None]
    b0f = net.b0 - (net.mean / net.std) @ net.W0
    folded = R.value_terms((W0f.numpy(), b0f.numpy()) + tuple(np.asarray(t, np.float64) for t in tv[2:6]) + (np.zeros(1),), s, 1)[0]
    np.testing.assert_allclose(folded, direct, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(net.packed().numpy()[:ns * hid[0] + hid[0]], np.concatenate([W0f.numpy().reshape(-1), b0f.numpy()]).astype(np.float32))
    with pytest.raises(ValueError, match='hidden'):
        P.ValueMLP(ns, (33, 4))
    with pytest.raises(ValueError, match='hidden'):
        P.ValueMLP(ns, (8,))


def test_value_mlp_fit_learns_a_coupling_the_diagonal_quadratic_cannot():
    from metrpo_amd import planning as P
    rng = np.random.RandomState(0)
    ns, N = 4, 512
    s = rng.randn(N, ns) * np.array([1.0, 2.0, 0.5, 3.0]) + np.array([0.0, 1.0, -2.0, 0.5])
    y = 0.5 * s[:, 0] ** 2 - 0.3 * s[:, 1] + 1.5 * s[:, 0] * s[:, 2] + 0.4 * s[:, 1] * s[:, 3]        # quadratic plus couplings
    # the best diagonal quadratic (least squares on [o, o^2, 1]) leaves the couplings unexplained
    F = np.concatenate([s, s ** 2, np.ones((N, 1))], axis=1)
    quad = float(np.mean((F @ np.linalg.lstsq(F, y, rcond=None)[0] - y) ** 2))
    net = P.ValueMLP(ns, (32, 32), generator=torch.Generator().manual_seed(0))
    losses = net.fit(s, y, 600, 1e-2)
    assert losses.shape == (601,) and np.isfinite(losses).all()
    assert losses[-1] < 0.25 * quad and losses[-1] < 0.05 * losses[0], (losses[0], losses[-1], quad)
    np.testing.assert_allclose(float(torch.mean((net.predict(s) - torch.as_tensor(y)) ** 2)), losses[-1], rtol=1e-9)
    assert abs(float(net.mean[1]) - s[:, 1].mean()) < 1e-9                               # normalise=True took the states' statistics
    # the packed net, evaluated by the restatement without a normaliser, is the fitted net to fp32 rounding of the weights
    p = net.packed().numpy().astype(np.float64)
    h1, h2 = net.hidden
    cut = np.cumsum([ns * h1, h1, h1 * h2, h2, h2, 1])
    parts = np.split(p, cut[:-1])
    tv = (parts[0].reshape(ns, h1), parts[1], parts[2].reshape(h1, h2), parts[3], parts[4], parts[5], np.zeros(1))
    np.testing.assert_allclose(R.value_terms(tv, s, 1)[0], net.predict(s).numpy(), rtol=0, atol=1e-4 * np.abs(y).max())
    with pytest.raises(ValueError, match='targets'):
        net.fit(s, y[:-1], 1, 1e-2)


def test_value_targets_are_discounted_returns_to_go():
    from metrpo_amd import planning as P
    rng = np.random.RandomState(2)
    paths = [dict(observations=rng.randn(L, 3), rewards=rng.randn(L)) for L in (5, 1, 8)]
    gamma = 0.9
    states, targets = P.value_targets(None, None, paths, gamma)
    assert states.shape == (14, 3) and targets.shape == (14,) and states.dtype == torch.float64
    want = np.concatenate([[sum(gamma ** (u - t) * p['rewards'][u] for u in range(t, len(p['rewards']))) for t in range(len(p['rewards']))] for p in paths])
    np.testing.assert_allclose(targets.numpy(), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(states.numpy(), np.concatenate([p['observations'] for p in paths]))

    class Const(object):
        def predict(self, path):
            return np.full(len(path['rewards']), 7.0)
    paths[2]['truncated'] = True                                                       # the last row's reward gives way to the baseline's estimate there
    _, boot = P.value_targets(None, Const(), paths, gamma)
    r = paths[2]['rewards'].copy(); r[-1] = 7.0
    np.testing.assert_allclose(boot.numpy()[6:], [sum(gamma ** (u - t) * r[u] for u in range(t, 8)) for t in range(8)], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(boot.numpy()[:6], want[:6], rtol=1e-12, atol=1e-12)      # paths that ended are left alone
    with pytest.raises(ValueError, match='rewards'):
        P.value_targets(None, None, [dict(observations=np.zeros((3, 2)), rewards=np.zeros(4))], gamma)


class _StubEngine(object):
    """What ShootingController needs of an engine when it is given a scorer: the shape, and somewhere to set the value"""
    device, ns, na = torch.device('cpu'), 4, 2

    def __init__(self):
        self.log, self.value = [], None

    def set_terminal_value_mlp(self, params, hidden, bias=0.0):
        self.value = (np.asarray(params), tuple(hidden), np.asarray(bias, np.float64).reshape(-1))
        self.log.append(('set_mlp', self.value))

    def set_terminal_value(self, w1, w2, bias):
        self.log.append(('set',))

    def clear_terminal_value(self):
        self.value = None
        self.log.append(('clear',))


def test_shooting_controller_sets_the_net_and_clears_it_around_a_plan():
    from metrpo_amd import planning as P
    eng = _StubEngine()
    net, _ = _net(eng.ns, (17, 5), 4)
    H, S = 5, 3
    seen = []

    def scorer(actions, init):
        seen.append(None if eng.value is None else eng.value)                          # what a scoring call would find set
        return -actions.pow(2).sum(dim=(0, 2)).unsqueeze(0)

    ctl = P.ShootingController(eng, H, 8, 2, 2, scorer=scorer, terminal_value=net, generator=torch.Generator().manual_seed(0))
    obs = np.zeros((S, eng.ns))
    ctl.get_actions(obs)
    assert [e[0] for e in eng.log] == ['set_mlp', 'clear'] and eng.value is None
    par, hid, bias = eng.log[0][1]
    np.testing.assert_array_equal(par, net.packed().numpy())
    assert hid == (17, 5) and np.array_equal(bias, [0.0])                               # a scalar bias unless the caller gives [S]
    assert len(seen) >= 2 and all(s is not None and s[1] == (17, 5) for s in seen)      # every scoring call of the plan
    net.bias = np.array([0.5, -1.0, 2.0])
    ctl.get_actions(obs); ctl.reset([False, True, False]); ctl.get_actions(obs)
    assert [e[0] for e in eng.log] == ['set_mlp', 'clear'] * 3
    np.testing.assert_array_equal(eng.log[-2][1][2], [0.5, -1.0, 2.0])

    # a scorer that raises: the value is cleared all the same
    def broken(actions, init):
        raise RuntimeError('no')
    bad = P.ShootingController(eng, H, 8, 2, 2, scorer=broken, terminal_value=net)
    with pytest.raises(RuntimeError):
        bad.get_actions(obs)
    assert eng.log[-1] == ('clear',) and eng.value is None
    with pytest.raises(ValueError, match='terminal_value needs an engine'):
        P.ShootingController(None, H, 8, 2, 2, scorer=scorer, na=2, terminal_value=net)


def test_the_new_names_are_exported():
    import metrpo_amd
    from metrpo_amd import planning as P
    for name in ('ValueMLP', 'value_targets', 'baseline_terminal_value'):
        assert name in metrpo_amd.__all__ and getattr(metrpo_amd, name) is getattr(P, name)
    assert hasattr(metrpo_amd.Engine, 'set_terminal_value_mlp') and isinstance(metrpo_amd.Engine.terminal_value_kind, property)
