"""CPU checks of tests/score_actions_ref.py, the float64 restatement the GPU tests of metrpo_score_actions compare against: it is the one-head
restatement tests/rollout_actions_ref.py discounted by hand, and it closes the loop with the oracle's validation cost (O.validation_costs,
model_based_rl.py:122-141) when it is fed the actions the clipped policy takes on head k."""
import numpy as np
import pytest

from oracle import metrpo_oracle as O
import helpers as Hh
import rollout_actions_ref as RA
import score_actions_ref as SA


def problem(env, K, hidden=(64, 64), seed=3):
    dm, theta, pdims, pool = Hh.problem_data(env, K, hidden, (32, 32), seed=seed, n_pool=64)
    return dm, theta, pdims, pool.astype(np.float32).astype(np.float64)


def policy_actions_on_head(dm, theta, pdims, env, s0, T, k):
    """The action sequence O.validation_costs' own loop takes on head k (:541-542, :550) -> [T, B, na], already inside [-1, 1]."""
    x = s0.copy()
    acts = []
    for t in range(T):
        u = np.clip(O.policy_mean(theta, pdims, x), -1.0, 1.0)
        acts.append(u)
        x = O.dynamics_forward(dm, k, x, u)
    return np.stack(acts)


@pytest.mark.parametrize('env,K,B,T,S,gamma,stop', [('swimmer', 5, 17, 11, 1, 0.99, True), ('swimmer', 3, 33, 5, 3, 1.0, False),
                                                    ('ant', 4, 16, 7, 16, 0.9, True), ('ant', 4, 16, 7, 16, 0.9, False), ('hopper', 2, 15, 3, 5, 1.0, True)])
def test_restatement_is_the_one_head_rollout_discounted_by_hand(env, K, B, T, S, gamma, stop):
    dm, _, _, pool = problem(env, K)
    rng = np.random.RandomState(10 * B + T)
    init = pool[rng.randint(len(pool), size=S)].astype(np.float32)
    if env == 'ant':
        init[1, 2], init[S - 1, 2] = 1.2, 0.1                       # outside 0.2 <= z <= 1.0: done at the first step, the mask acts
    actions = (1.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    got = SA.score_actions(dm, env, init, actions, gamma=gamma, stop_at_done=stop, keep=True)
    starts = SA.start_rows(init, B)
    assert np.array_equal(starts[0], init[0]) and np.array_equal(starts[-1], init[S - 1]) and np.array_equal(starts[B // S - 1], init[0])
    for k in range(K):
        ref = RA.rollout_actions(dm, env, starts, actions, model=k)
        assert np.array_equal(got['obs'][k], ref['obs']) and np.array_equal(got['rew'][k], ref['rew']) and np.array_equal(got['done'][k], ref['done'])
        ret = np.zeros(B); n = np.zeros(B, int)
        for b in range(B):                                          # by hand, one candidate at a time
            alive = True
            for t in range(T):
                if alive:
                    ret[b] += gamma ** t * ref['rew'][t, b]; n[b] += 1
                if stop and ref['done'][t, b]:
                    alive = False
        np.testing.assert_allclose(got['ret'][k], ret, rtol=1e-13, atol=1e-13)      # gamma ** t against repeated multiplication
        assert np.array_equal(got['len'][k], n)
        r2, n2 = SA.discount_and_sum(ref['rew'], ref['done'], gamma, stop)
        assert np.array_equal(r2, got['ret'][k]) and np.array_equal(n2, n)
    if env == 'ant':
        assert got['done'][:, 0].any()
        assert (got['len'] == 1).any() if stop else (got['len'] == T).all()
    np.testing.assert_allclose(got['mean'], got['ret'].mean(axis=0), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(got['std'], got['ret'].std(axis=0), rtol=1e-12, atol=1e-14)


def test_one_head_has_zero_std():
    dm, _, _, pool = problem('half_cheetah', 1)
    rng = np.random.RandomState(0)
    got = SA.score_actions(dm, 'half_cheetah', pool[:2].astype(np.float32), (1.5 * rng.randn(4, 6, dm.na)).astype(np.float32), gamma=0.95)
    assert np.array_equal(got['std'], np.zeros(6)) and np.array_equal(got['mean'], got['ret'][0])


@pytest.mark.parametrize('env,plant', [('swimmer', False), ('ant', True)])
def test_policy_actions_fed_back_give_the_validation_cost(env, plant):
    """O.validation_costs(...)[k] = sum_t gamma^t mean_b cost_t (1 - dones) with head k fixed and the clipped policy acting: feeding that action sequence
    back, -mean_b ret[k] is the same number up to the order of the float64 sums (gamma ** t against repeated multiplication, mean of sums against sum
    of means)."""
    K, B, T, gamma = 4, 12, 9, 0.97
    dm, theta, pdims, pool = problem(env, K, seed=5)
    s0 = pool[:B].copy()
    if plant:
        s0[2, 2], s0[7, 2] = 1.3, 0.05                              # out-of-range z: those rows are done at once, every later cost is masked
    want = O.validation_costs(dm, theta, pdims, env, s0, T, gamma)
    for k in range(K):
        acts = policy_actions_on_head(dm, theta, pdims, env, s0, T, k)
        got = SA.score_actions(dm, env, s0, acts, gamma=gamma, stop_at_done=True)
        np.testing.assert_allclose(-got['ret'][k].mean(), want[k], rtol=1e-12, atol=1e-13)
        if plant:
            assert got['len'][k, 2] == 1 and got['len'][k, 7] == 1 and got['len'][k].max() == T
            unmasked = SA.score_actions(dm, env, s0, acts, gamma=gamma, stop_at_done=False)
            assert abs(-unmasked['ret'][k].mean() - want[k]) > 1e-6                 # the mask is what makes them agree
