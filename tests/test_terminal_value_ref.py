"""CPU tests of the terminal value's float64 side (tests/terminal_value_ref.py, tests/terminal_value_cases.py) and of its host code
(metrpo_amd.planning.baseline_terminal_value, ShootingController(terminal_value=...)): the table meets the kink guard's cap, the bounds have room
for fp32 arithmetic and none for a wrong restatement, the gradients are those of the return, and the host side does what it says -- without the
library."""
import numpy as np
import pytest
import torch

import score_grad_ref as G0
import score_policy_grad_ref as P0
import terminal_value_cases as TC
import terminal_value_ref as R

# the share of every bound the float32 walk (the device's number format, NumPy's summation order) may use: the rest is the device's own orders
F32_SHARE = 0.1


def test_the_table_meets_the_redraw_cap():
    worst = 0.0
    for case, loop in TC.RUNS:
        d = TC.case_data(case, loop)
        assert d['accepted'] == case.B, (case.id, loop, d['accepted'], d['replaced'])
        assert d['replaced'] <= TC.MAX_REPLACED * case.B, (case.id, loop, d['replaced'])
        assert d['margin'] >= TC.KINK_FACTOR
        worst = max(worst, d['replaced'] / case.B)
    print("worst share of candidates redrawn: %.3g" % worst)


def test_the_table_holds_what_it_says():
    ids = [c.id for c in TC.CASES]
    assert len(set(ids)) == len(ids)
    for path in ('fused', 'generic'):
        cs = [c for c in TC.CASES if c.path == path]
        assert {c.B for c in cs if c.env == 'swimmer' and c.T == 2 and c.calls == 'all'} >= {1, 15, 16, 17, 33}
        assert {c.B for c in cs if c.calls == 'grad'} == {63, 64, 65}
        assert any(c.T == 1 for c in cs) and {c.K for c in cs} >= {1, 5, 9}
        assert {c.env for c in cs if (c.B, c.T, c.S, c.nb) == (33, 11, 3, 3)} >= set(TC.FUSED_ENVS)
        assert any(c.dh == (48, 48) for c in cs) and any(not c.stop for c in cs) and any(c.gamma == 1.0 for c in cs)
        assert any(c.variant == 'tv_far' for c in cs) and any(not c.noise for c in cs)
        assert {c.in_std for c in cs} == {False, True}
    # Ant: a done at the first step, in the middle, at the last step (no bootstrap there either), and never
    for case in (c for c in TC.CASES if c.variant == 'ant_plant'):
        for loop in TC.LOOPS:
            ref = TC.reference(TC.case_data(case, loop))
            n, T, wT = ref['len'], case.T, ref['wT']
            assert (n == 1).any() and ((n > 1) & (n < T)).any() and ((n == T) & (wT == 0)).any() and ((n == T) & (wT != 0)).any(), (case.id, loop)
    # tv_far: the value's clip acts on some dims of some candidates and not on others
    for case in (c for c in TC.CASES if c.variant == 'tv_far'):
        site = TC.reference(TC.case_data(case, 'open'))['sites']['tv_clip']
        assert (site > 0).any() and (site < 0).all(axis=1).any()


def test_without_a_value_the_walk_is_the_walks_it_restates():
    for case in (c for c in TC.CASES if c.path == 'fused' and c.T == 11 and c.noise):
        d = TC.case_data(case, 'open')
        a, b = TC.walk(d, tv=None), G0.walk(d['dm'], case.env, d['init'], d['seq'], case.gamma, case.stop)
        for w in ('ret', 'len', 'grad', 'lam0'):
            assert np.array_equal(a[w], b[w]), (case.id, w)
        d = TC.case_data(case, 'closed')
        a = TC.walk(d, tv=None)
        b = P0.walk(d['dm'], d['theta'], d['pdims'], case.env, d['init'], d['seq'], gamma=case.gamma, stop_at_done=case.stop, noise_in_std=case.in_std)
        for w in ('ret', 'len', 'grad', 'lam0', 'act'):
            assert np.array_equal(a[w], b[w]), (case.id, w)


def test_the_float32_walk_uses_a_stated_share_of_every_bound():
    worst = np.zeros(6)
    for case, loop in TC.RUNS:
        d = TC.case_data(case, loop)
        ref = TC.reference(d)
        w32 = TC.walk(d, dtype=np.float32)
        assert np.array_equal(w32['len'], ref['len'])
        use = TC.shares(w32, ref, case)
        assert use.max() <= F32_SHARE, (case.id, loop, use)
        worst = np.maximum(worst, use)
    print("float32 walk, worst shares (grad whole / step / candidate, lam0 whole / candidate, ret):", worst)


@pytest.mark.parametrize('mut', R.MUTS)
def test_every_mutation_exceeds_a_bound(mut):
    caught = []
    for case, loop in TC.RUNS:
        if case.path != 'fused' or (mut == 'tv_no_policy_path' and loop == 'open'):
            continue
        d = TC.case_data(case, loop)
        use = TC.shares(TC.walk(d, mut=mut), TC.reference(d), case)
        if use.max() > 1.0:
            caught.append((case.id, loop, float(use.max())))
    print("%s: caught on %d runs, worst share %.3g" % (mut, len(caught), max([c[2] for c in caught] or [0.0])))
    assert caught, mut


@pytest.mark.parametrize('loop', TC.LOOPS)
def test_float64_gradients_are_those_of_the_return(loop):
    """grad and lam0 against central differences of the float64 return along a random direction, per head and candidate (per start state for
    lam0: a start state's candidates move together), on the candidates whose every kink argument is at least CLEAR away from its kink: the step
    moves an argument by a few eps."""
    eps, CLEAR, rng = 1e-7, 1e-5, np.random.RandomState(3)
    picked = [c for c in TC.CASES if c.path == 'fused' and c.noise and (c.variant in ('tv_far', 'ant_plant') or (c.T == 11 and c.env in ('hopper', 'half_cheetah'))
                                                                         or (c.env == 'swimmer' and c.B == 17 and c.K == 5))]
    assert len(picked) >= 6
    for case in picked:
        d = TC.case_data(case, loop)
        ref = TC.reference(d)
        da = rng.randn(*d['seq'].shape); ds = rng.randn(*d['init'].shape)
        clear = np.min([np.abs(v).min(axis=1) for v in ref['sites'].values()], axis=0) >= CLEAR
        assert clear.sum() >= (case.B + 3) // 4, (case.id, loop, clear.sum())

        def ret_at(seq, init):
            c = d['case']
            return R.walk(d['dm'], c.env, init, seq, d['tv'], grad=False, **TC.walk_kw(c, loop, d['theta'], d['pdims']))['ret']
        num_a = (ret_at(d['seq'] + eps * da, d['init']) - ret_at(d['seq'] - eps * da, d['init'])) / (2 * eps)              # [K, B]
        ana_a = np.einsum('ktbd,tbd->kb', ref['grad'], da)
        num_s = (ret_at(d['seq'], d['init'] + eps * ds) - ret_at(d['seq'], d['init'] - eps * ds)) / (2 * eps)
        ana_s = np.einsum('kbd,bd->kb', ref['lam0'], np.repeat(ds, case.B // case.S, axis=0))
        for num, ana in ((num_a, ana_a), (num_s, ana_s)):
            scale = np.abs(ana).max()
            assert np.abs(num - ana)[:, clear].max() <= 1e-6 * scale + 1e-7, (case.id, loop, np.abs(num - ana)[:, clear].max(), scale)


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------------
def test_baseline_terminal_value_is_predict_at_the_row():
    from metrpo_amd import planning as P
    from metrpo_amd.baseline import LinearFeatureBaseline
    rng = np.random.RandomState(0)
    ns, L = 7, 40
    bl = LinearFeatureBaseline()
    bl.set_param_values(rng.randn(2 * ns + 4))
    path = dict(observations=rng.randn(L, ns) * 6.0, rewards=np.zeros(L))           # some entries beyond the clip
    want = bl.predict(path)
    o = np.clip(path['observations'], -10, 10)
    for coeffs in (bl, bl.coeffs, torch.as_tensor(bl.coeffs)):
        for t in (0, 7, L - 1):
            w1, w2, bias = (np.asarray(x) for x in P.baseline_terminal_value(coeffs, t, ns))
            assert w1.shape == (ns,) and w2.shape == (ns,) and bias.shape == ()
            np.testing.assert_allclose(bias + o[t] @ w1 + (o[t] ** 2) @ w2, want[t], rtol=1e-12, atol=1e-12)
        ts = np.array([3, 0, 39, 12])
        w1, w2, bias = (np.asarray(x) for x in P.baseline_terminal_value(coeffs, ts, ns))
        assert bias.shape == (4,)
        np.testing.assert_allclose(bias + o[ts] @ w1 + (o[ts] ** 2) @ w2, want[ts], rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match='coefficients'):
        P.baseline_terminal_value(np.zeros(2 * ns + 3), 0, ns)
    with pytest.raises(ValueError, match='not been fitted'):
        P.baseline_terminal_value(LinearFeatureBaseline(), 0, ns)


class _StubEngine(object):
    """What ShootingController needs of an engine when it is given a scorer: the shape, and somewhere to set the value"""
    device, ns, na = torch.device('cpu'), 4, 2

    def __init__(self):
        self.log, self.value = [], None

    def set_terminal_value(self, w1, w2, bias):
        self.value = (np.asarray(w1), np.asarray(w2), np.asarray(bias).reshape(-1))
        self.log.append(('set', self.value[2].copy()))

    def clear_terminal_value(self):
        self.value = None
        self.log.append(('clear',))


def test_shooting_controller_counts_steps_and_sets_and_clears_around_a_plan():
    from metrpo_amd import planning as P
    eng = _StubEngine()
    ns, H, S = eng.ns, 5, 3
    coeffs = np.arange(2 * ns + 4, dtype=np.float64) / 10.0
    seen = []

    def scorer(actions, init):
        seen.append(None if eng.value is None else eng.value[2].copy())                # what a scoring call would find set
        return -actions.pow(2).sum(dim=(0, 2)).unsqueeze(0)

    bias_at = lambda steps: np.asarray(P.baseline_terminal_value(coeffs, np.asarray(steps) + H, ns)[2])
    ctl = P.ShootingController(eng, H, 8, 2, 2, scorer=scorer, terminal_value=coeffs, generator=torch.Generator().manual_seed(0))
    obs = np.zeros((S, ns))
    ctl.get_actions(obs)
    assert eng.log[0][0] == 'set' and eng.log[-1] == ('clear',) and len(eng.log) == 2 and eng.value is None
    np.testing.assert_array_equal(eng.log[0][1], bias_at([0, 0, 0]))
    assert len(seen) >= 2 and all(s is not None and np.array_equal(s, bias_at([0, 0, 0])) for s in seen)      # every scoring call of the plan
    ctl.get_actions(obs); ctl.get_actions(obs)
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([2, 2, 2]))
    ctl.reset([False, True, False])                                                    # env 1 starts a new path
    ctl.get_actions(obs)
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([3, 0, 3]))
    assert len(set(eng.log[-2][1])) == 2                                               # per-environment biases
    ctl.get_actions(obs)
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([4, 1, 4]))
    ctl.reset()
    ctl.get_actions(obs)
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([0, 0, 0]))
    assert [e[0] for e in eng.log] == ['set', 'clear'] * 6
    # another number of envs between calls: get_actions starts the counters afresh, and so does a reset whose dones no longer fit them
    ctl.get_actions(obs); ctl.get_actions(obs[:2])
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([0, 0]))
    ctl.reset([False, True, False])                                                    # three dones, two counters
    ctl.get_actions(obs)
    np.testing.assert_array_equal(eng.log[-2][1], bias_at([0, 0, 0]))

    # a scorer that raises: the value is cleared all the same
    def broken(actions, init):
        raise RuntimeError('no')
    bad = P.ShootingController(eng, H, 8, 2, 2, scorer=broken, terminal_value=coeffs)
    with pytest.raises(RuntimeError):
        bad.get_actions(obs)
    assert eng.log[-1] == ('clear',) and eng.value is None
    # the default leaves the controller as it is: nothing set, cleared or counted
    n = len(eng.log)
    plain = P.ShootingController(eng, H, 8, 2, 2, scorer=scorer, generator=torch.Generator().manual_seed(0))
    plain.get_actions(obs); plain.reset([True, False, False]); plain.get_actions(obs)
    assert len(eng.log) == n and plain._steps is None and seen[-1] is None
    with pytest.raises(ValueError, match='terminal_value needs an engine'):
        P.ShootingController(None, H, 8, 2, 2, scorer=scorer, na=2, terminal_value=coeffs)
