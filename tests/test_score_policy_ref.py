"""CPU checks of tests/score_policy_ref.py, the float64 restatement the GPU tests of metrpo_score_policy_actions compare against: a two-step case by
hand, its identities (zero noise is no noise; its own actions fed to tests/score_actions_ref.py give the same returns; the policy's deterministic
actions close the loop with O.validation_costs), the fitness of every GPU case (the fp32 restatement agrees on len and uses at most half of the ret
bound), and four deliberately wrong restatements that each miss a bound."""
import numpy as np
import pytest

from oracle import metrpo_oracle as O
import tolerances as TOL
import score_actions_ref as SA
import score_policy_ref as SP


def reward_row(t):
    return TOL.REWARD if t <= 10 else TOL.LONG_RUN


def test_two_steps_by_hand():
    dm, theta, pdims, pool, env = SP.problem_data('swimmer')
    gamma, k = 0.9, 2
    s0 = pool[5].astype(np.float32).astype(np.float64)
    nz = np.array([[[0.3, -2.5]], [[-0.2, 0.6]]], np.float32)                      # [T = 2, B = 1, na = 2]
    sig = np.exp(np.maximum(theta[-dm.na:], np.log(1e-6)))
    for in_std in (False, True):
        s = s0[None]
        total, disc, acts = 0.0, 1.0, []
        for t in range(2):
            m = O.policy_mean(theta, pdims, s)
            a = m + (nz[t] * sig if in_std else nz[t])
            u = np.minimum(np.maximum(a, -1.0), 1.0)
            nxt = O.dynamics_forward(dm, k, s, u)
            total += disc * -O.cost_np_vec(env, s, u, nxt)[0]
            disc *= gamma
            acts.append(a)
            s = nxt
        got = SP.score_policy_actions(dm, theta, pdims, env, s0, nz, gamma=gamma, noise_in_std=in_std, keep=True)
        assert got['ret'].shape == (dm.K, 1) and got['len'].tolist() == [[2]] * dm.K
        np.testing.assert_allclose(got['ret'][k, 0], total, rtol=1e-14, atol=0)
        np.testing.assert_allclose(got['act'][k, :, 0], np.concatenate(acts), rtol=1e-14, atol=0)
        assert np.abs(np.concatenate(acts)).max() > 1.0                              # the clip acted in this case


@pytest.mark.parametrize('name', ['swimmer', 'ant'])
def test_zero_noise_is_no_noise_and_own_actions_replay(name):
    dm, theta, pdims, pool, env = SP.problem_data(name)
    B, T, gamma = 12, 6, 0.97
    init, noise = SP.inputs(name, B, T, B)
    none = SP.score_policy_actions(dm, theta, pdims, env, init, None, T=T, gamma=gamma, keep=True)
    for in_std in (False, True):
        zero = SP.score_policy_actions(dm, theta, pdims, env, init, np.zeros_like(noise), gamma=gamma, noise_in_std=in_std, keep=True)
        for w in ('ret', 'len', 'rew', 'done', 'obs', 'act'):
            assert np.array_equal(zero[w], none[w]), w
    for in_std in (False, True):                                                     # the restatement's own actions under score_actions_ref
        got = SP.score_policy_actions(dm, theta, pdims, env, init, noise, gamma=gamma, noise_in_std=in_std, keep=True)
        assert not np.array_equal(got['ret'], none['ret'])
        for k in range(dm.K):
            rep = SA.score_actions(dm, env, init, got['act'][k], gamma=gamma)
            assert np.array_equal(rep['ret'][k], got['ret'][k]) and np.array_equal(rep['len'][k], got['len'][k])
    if name == 'ant':
        assert (none['len'] == 1).any() and (none['len'] == T).any()                # the planted rows end at once


@pytest.mark.parametrize('env,plant', [('swimmer', False), ('ant', True)])
def test_deterministic_policy_gives_the_validation_cost(env, plant):
    """O.validation_costs(...)[k] = sum_t gamma^t mean_b cost_t (1 - dones) with head k fixed and the clipped policy acting: -mean_b ret[k] of the
    restatement without noise is the same number up to the order of the float64 sums."""
    dm, theta, pdims, pool, _ = SP.problem_data(env)
    B, T, gamma = 12, 9, 0.97
    s0 = pool[:B].copy()
    if plant:
        s0[2, 2], s0[7, 2] = 1.3, 0.05
    want = O.validation_costs(dm, theta, pdims, env, s0, T, gamma)
    got = SP.score_policy_actions(dm, theta, pdims, env, s0, None, T=T, gamma=gamma)
    np.testing.assert_allclose(-got['ret'].mean(axis=1), want, rtol=1e-12, atol=1e-13)
    if plant:
        assert np.all(got['len'][:, [2, 7]] == 1) and got['len'].max() == T


@pytest.mark.parametrize('name,B,T,S,gamma,stop,in_std,with_noise', SP.CASES)
def test_gpu_cases_are_fit_for_the_gpu_check(name, B, T, S, gamma, stop, in_std, with_noise):
    """A case whose fp32 restatement already spends more than half of the ret bound, or disagrees on len, has the wrong inputs for the GPU check."""
    env = SP.problem_data(name)[4]
    ref = SP.reference(name, B, T, S, gamma, stop, in_std, with_noise)
    r32 = SP.reference(name, B, T, S, gamma, stop, in_std, with_noise, dtype=np.float32)
    assert SP.z_clear(env, ref)
    assert np.array_equal(r32['len'], ref['len'])
    bnd = SP.bound(ref['rew'], gamma, reward_row)
    share = float((np.abs(r32['ret'] - ref['ret']) / bnd).max())
    print("%s B=%d T=%d S=%d gamma=%g stop=%d in_std=%d noise=%d: fp32 restatement uses %.3g of the ret bound" % (name, B, T, S, gamma, stop, in_std, with_noise, share))
    assert share <= 0.5
    if with_noise:
        assert np.abs(ref['act']).max() > 1.0 or ref['act'].size < 8                 # the clip acts
    if env == 'ant' and S >= 3 and stop:
        assert (ref['len'] == 1).any()


WRONG_CASES = {'noise_after_clip': ('swimmer', 33, 11, 3, 0.99, True, False), 'mean_at_next': ('swimmer', 33, 11, 3, 0.99, True, False),
               'std_when_plain': ('swimmer', 33, 11, 3, 0.99, True, False), 'mask_before_cost': ('ant', 33, 11, 3, 0.99, True, False)}


@pytest.mark.parametrize('wrong', SP.WRONG)
def test_wrong_restatements_miss_the_bound(wrong):
    """Each of these mistakes misses the ret bound of a GPU case (B = 33, T = 11, S = 3, gamma = 0.99) -- observed worst |ret - ref| / bound:
        noise_after_clip  (the head stepped with clip(mean) + noise, the sum not clipped)   4.05e+03
        mean_at_next      (the cost's action formed from s_t+1 instead of s_t)              23.3
        std_when_plain    (exp(log_std) applied with noise_in_std = 0)                      1.82e+03
        mask_before_cost  (Ant: the mask updated before the step's cost)                    4.92e+03  (and len is one short on the planted rows)
    The correct fp32 restatement uses at most 0.022 of the same bound (test_gpu_cases_are_fit_for_the_gpu_check prints every case's share)."""
    name, B, T, S, gamma, stop, in_std = WRONG_CASES[wrong]
    dm, theta, pdims, _, env = SP.problem_data(name)
    init, noise = SP.inputs(name, B, T, S)
    ref = SP.reference(name, B, T, S, gamma, stop, in_std, True)
    bad = SP.score_policy_actions(dm, theta, pdims, env, init, noise, gamma=gamma, stop_at_done=stop, noise_in_std=in_std, wrong=wrong)
    bnd = SP.bound(ref['rew'], gamma, reward_row)
    factor = float((np.abs(bad['ret'] - ref['ret']) / bnd).max())
    print("%s: %.3g times the bound" % (wrong, factor))
    assert factor > 10.0
    if wrong == 'mask_before_cost':
        assert not np.array_equal(bad['len'], ref['len'])
