"""CPU checks of tests/score_policy_grad_ref.py (the float64 restatement of metrpo_score_policy_actions_grad) and of tests/score_policy_grad_cases.py
(the case table and kink guard of tests/test_gpu_score_policy_grad.py), without the library:
  * the restatement against central differences of score_policy_ref.score_policy_actions' float64 ret, in both noise units;
  * its ret / len / actions are that restatement's;
  * at noise = 0, averaged and contracted with d mean / d theta, it reproduces oracle.bptt_oracle's theta-gradient (the one pinned against the
    reference's own graph);
  * the kink guard's cap holds on every case;
  * its float32 mode stays below 0.1 of every bound the GPU test holds (printed);
  * each wrong restatement misses a bound (printed): the four of the closed loop at EVERY case with T >= 2 that they can touch ('sigma_missing'
    changes nothing where the noise is in action units: every such case in units of the std), score_grad_ref's six on the case that module's own
    test uses for each (a mask or a gamma mistake cannot show where no candidate ends or gamma = 1)."""
import numpy as np
import pytest

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
import score_policy_ref as SP
import score_policy_grad_ref as R
import score_policy_grad_cases as PC
import score_grad_ref as R0


def case(path, env, variant='plain', stop=True, T=11):
    return next(c for c in PC.CASES if c.path == path and c.env == env and c.variant == variant and c.stop == stop and c.T == T and c.dh == (64, 64))


@pytest.mark.parametrize('in_std', [False, True], ids=['act', 'std'])
def test_restatement_against_central_differences(in_std):
    c = case('fused', 'hopper')
    dm, theta, pdims, pool = PC.problem(c)
    rng = np.random.RandomState(11)
    T, B = 5, 3
    init = pool[rng.permutation(len(pool))[:B]].copy()                     # S = B
    sigma = np.exp(O.policy_log_std(theta, pdims)) if in_std else 1.0
    noise = 0.8 * rng.randn(T, B, dm.na) / sigma
    kw = dict(gamma=c.gamma, stop_at_done=c.stop, noise_in_std=in_std)
    ref = R.score_policy_actions_grad(dm, theta, pdims, c.env, init, noise, **kw)
    sp = SP.score_policy_actions(dm, theta, pdims, c.env, init, noise, keep=True, **kw)
    assert np.array_equal(ref['len'], sp['len']) and np.allclose(ref['ret'], sp['ret'], rtol=1e-13, atol=1e-13)     # R is score_policy_actions' ret
    assert np.allclose(ref['act'], sp['act'], rtol=1e-13, atol=1e-13)
    ret = lambda i, n: SP.score_policy_actions(dm, theta, pdims, c.env, i, n, **kw)['ret']
    h = 1e-6
    # a candidate whose action comes within 1e-4 of the clip on any head at any step is left out: the difference quotient straddles the kink there
    clear = np.all(np.abs(np.abs(ref['act']) - 1) > 1e-4, axis=(0, 1, 3))
    assert clear.any() and (np.abs(ref['act']) > 1).any()
    worst = 0.0
    for t in range(T):
        for j in range(dm.na):
            npl, nmi = noise.copy(), noise.copy()
            npl[t, :, j] += h; nmi[t, :, j] -= h
            fd = (ret(init, npl) - ret(init, nmi)) / (2 * h)
            g = ref['grad'][:, t, :, j]
            worst = max(worst, float((np.abs(fd - g) / (np.abs(g) + 1e-3))[:, clear].max()))
    for i in range(dm.ns):
        ip, im = init.copy(), init.copy()
        ip[:, i] += h; im[:, i] -= h
        fd = (ret(ip, noise) - ret(im, noise)) / (2 * h)
        worst = max(worst, float((np.abs(fd - ref['lam0'][:, :, i]) / (np.abs(ref['lam0'][:, :, i]) + 1e-3))[:, clear].max()))
    print("central differences (%s): worst relative difference %.3g" % ('std' if in_std else 'act', worst))
    # h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 |R| / h ~ 1e-9, and ret sums float64 gamma^t where the gradient's weights are fp32(gamma^t), 6e-8 apart
    assert worst < 1e-5


def test_theta_gradient_of_the_bptt_oracle_at_zero_noise():
    """grad_theta mean_k cost_k = -sum_{k, t, b} gm[k][t][b] . d mean(s_t) / d theta / (B K): ties the restatement to oracle.bptt_oracle"""
    c = next(x for x in PC.CASES if x.path == 'fused' and x.env == 'swimmer' and x.B == 17 and x.T == 2 and x.K == 5)
    dm, theta, pdims, pool = PC.problem(c)
    init = pool[:7].copy()
    T, gamma = 2, 0.99
    out = R.walk(dm, theta, pdims, c.env, init, None, T=T, gamma=gamma, stop_at_done=False)
    assert np.array_equal(out['grad'], out['gm'])
    Ws, bs, log_std = O.policy_unflatten(np.asarray(theta, np.float64), pdims)
    gWs = [np.zeros_like(W) for W in Ws]; gbs = [np.zeros_like(b) for b in bs]
    B = init.shape[0]
    for k in range(dm.K):
        for t in range(T):
            _, hs = O._policy_forward(Ws, bs, out['obs'][k, t])
            gW, gb = O._backward(Ws, hs, -out['gm'][k, t] / (B * dm.K))
            for l in range(len(Ws)):
                gWs[l] += gW[l]; gbs[l] += gb[l]
    mine = O.policy_flatten(gWs, gbs, np.zeros_like(log_std))
    costs, want = Bp.policy_costs_and_grad(dm, theta, pdims, c.env, init, T, gamma)
    rel = float(np.linalg.norm(mine - want) / np.linalg.norm(want))
    print("theta-gradient against bptt_oracle: %.3g relative" % rel)
    # the restatement's weights are fp32-rounded gamma^t (the header's rule), the oracle's float64: 0.99 rounds by 2e-8 relative
    assert rel < 1e-7
    np.testing.assert_allclose(-out['ret'].sum(axis=1) / B, costs, rtol=1e-12)


def test_case_table_and_kink_guard():
    ids = [c.id for c in PC.CASES]
    assert len(set(ids)) == len(ids) and len(ids) == len(PC.GC.CASES)
    for path in ('fused', 'generic'):
        assert {c.in_std for c in PC.CASES if c.path == path} == {False, True}
    worst, clip_lo = 0.0, 1.0
    for c in PC.CASES:
        d = PC.case_data(c)
        assert d['accepted'] == c.B and d['replaced'] <= PC.MAX_REPLACED * c.B, (c.id, d['replaced'], d['accepted'])
        assert d['margin'] >= PC.KINK_FACTOR
        a = np.abs(PC.reference(d)['act'])
        assert (a > 1).any() and (a < 1).any(), c.id           # the clip gate is exercised, and not everything is gated away
        worst = max(worst, d['replaced'] / float(c.B)); clip_lo = min(clip_lo, float((a > 1).mean()))
    print("kink guard: at most %.3f of a case's candidates replaced; at least %.3f of a case's actions clipped" % (worst, clip_lo))


F32_CASES = [case('fused', env) for env in PC.GC.FUSED_ENVS] + [case('fused', 'ant', 'ant_plant')]


def test_float32_restatement_uses_a_small_share_of_every_bound():
    worst = np.zeros(7)
    for c in F32_CASES:
        d = PC.case_data(c)
        ref = PC.reference(d)
        got = R.walk(d['dm'], d['theta'], d['pdims'], c.env, d['init'], d['noise'], gamma=c.gamma, stop_at_done=c.stop, noise_in_std=c.in_std,
                     dtype=np.float32)
        got['grad_mean'] = got['grad'].sum(axis=0) / d['dm'].K
        assert np.array_equal(got['len'], ref['len'])
        worst = np.maximum(worst, PC.shares(got, ref, c))
    print("float32 restatement, shares of the bounds: grad whole %.3g, per step %.3g, per candidate %.3g; lam0 whole %.3g, per candidate %.3g; ret %.3g; "
          "grad_mean %.3g" % tuple(worst))
    assert worst.max() < 0.1


def _mut_factor(c, mut):
    d = PC.case_data(c)
    ref = PC.reference(d)
    got = R.walk(d['dm'], d['theta'], d['pdims'], c.env, d['init'], d['noise'], gamma=c.gamma, stop_at_done=c.stop, noise_in_std=c.in_std, mut=mut)
    return float(np.max(PC.shares(got, ref, c)[:5]))


@pytest.mark.parametrize('mut', ('no_policy_path', 'gate_on_mean', 'sigma_missing', 'policy_at_next'))
def test_closed_loop_mistakes_miss_a_bound_at_every_case(mut):
    cases = [c for c in PC.CASES if c.T >= 2 and (c.in_std or mut != 'sigma_missing')]
    assert len(cases) >= 20
    factors = {c.id: _mut_factor(c, mut) for c in cases}
    lo = min(factors, key=factors.get)
    print("%s: misses a gradient bound by a factor of at least %.3g (%s), at most %.3g" % (mut, factors[lo], lo, max(factors.values())))
    assert factors[lo] > 1.0, (lo, factors[lo])


@pytest.mark.parametrize('mut', R0.MUTS)
def test_open_loop_mistakes_miss_a_bound_by_a_wide_factor(mut):
    c = case('fused', 'ant', 'ant_plant') if mut == 'mask_first' else case('fused', 'half_cheetah')
    factor = _mut_factor(c, mut)
    print("%s: misses a gradient bound by a factor %.3g" % (mut, factor))
    assert factor > 10.0
