"""CPU pins of tests/rollout_actions_ref.py, the float64 restatement the GPU tests of metrpo_rollout_actions compare against: a two-step case
computed by hand, and the identity the model diagnostic rests on -- a deterministic replay does not depend on how long it will run."""
import numpy as np

from oracle import metrpo_oracle as O
import helpers as Hh
import rollout_actions_ref as RA


def hand_model():
    """Swimmer dims (ns 10, na 2, n_drop 2), K = 2, one hidden relu unit: head k computes h = relu((k + 1) * clip(a_0) / 2) -- the action's
    in_std is 2 -- and predicts s'_5 = 0.5 + h + s_5 (diff_mean_5 = 0.5), every other state dim unchanged."""
    ns, na, K = 10, 2, 2
    W0 = np.zeros((K, ns + na - 2, 1)); W0[0, 8, 0] = 1.0; W0[1, 8, 0] = 2.0          # feature 8 of the dropped input = action dim 0
    W1 = np.zeros((K, 1, ns)); W1[:, 0, 5] = 1.0
    in_std = np.ones(ns + na); in_std[ns:] = 2.0
    diff_mean = np.zeros(ns); diff_mean[5] = 0.5
    return O.DynamicsEnsemble([W0, W1], [np.zeros((K, 1)), np.zeros((K, ns))], ['relu'], np.zeros(ns + na), in_std, diff_mean, np.ones(ns), 2, ns, na)


def test_two_steps_by_hand():
    dm = hand_model()
    init = np.zeros((2, 10)); init[0, 3] = 7.0
    #                  env 0: clipped (1, 0.5)   env 1: clipped (-1, -1)          step 1: (0.4, 0)   (1, 1)
    actions = np.array([[[3.0, 0.5], [-2.0, -3.0]], [[0.4, 0.0], [1.0, 2.0]]])
    r = RA.rollout_actions(dm, 'swimmer', init, actions, model=-1)
    assert r['obs'].shape == (3, 2, 10) and r['rew'].shape == (2, 2) and r['done'].shape == (2, 2)
    assert np.array_equal(r['clipped'], [[[1.0, 0.5], [-1.0, -1.0]], [[0.4, 0.0], [1.0, 1.0]]])
    assert np.array_equal(r['obs'][0], init)
    # mean of the heads: h = (0.5 + 1.0) / 2 | relu(-0.5), relu(-1) = 0, then (0.2 + 0.4) / 2 | (0.5 + 1.0) / 2
    np.testing.assert_allclose(r['obs'][:, :, 5], [[0.0, 0.0], [1.25, 0.5], [2.05, 1.75]], rtol=0, atol=1e-15)
    # reward = s'_5 - 1e-2 * mean(u^2)
    np.testing.assert_allclose(r['rew'], [[1.25 - 0.00625, 0.5 - 0.01], [2.05 - 0.0008, 1.75 - 0.01]], rtol=0, atol=1e-15)
    other = np.delete(r['obs'], 5, axis=2)
    assert np.array_equal(other, np.broadcast_to(np.delete(init, 5, axis=1), other.shape))      # nothing else moves; s_3 = 7 is carried
    assert not r['done'].any()
    one = RA.rollout_actions(dm, 'swimmer', init, actions, model=1)
    np.testing.assert_allclose(one['obs'][:, :, 5], [[0.0, 0.0], [1.5, 0.5], [2.4, 2.0]], rtol=0, atol=1e-15)
    per_env = RA.rollout_actions(dm, 'swimmer', init, actions, model=np.array([0, 1]))
    np.testing.assert_allclose(per_env['obs'][:, :, 5], [[0.0, 0.0], [1.0, 0.5], [1.7, 2.0]], rtol=0, atol=1e-15)


def test_row_h_of_a_long_replay_is_the_h_step_replay():
    """... Ant's done included: a done neither stops nor resets."""
    dm, theta, pdims, pool = Hh.problem_data('ant', 3, (64, 64), (32, 32), seed=2, n_pool=16)
    rng = np.random.RandomState(0)
    init = pool[:7].copy(); init[1, 2] = 1.2; init[4, 2] = 0.1                      # done at their first step
    actions = 1.5 * rng.randn(6, 7, dm.na)
    for model in (-1, 2, rng.randint(3, size=7)):
        full = RA.rollout_actions(dm, 'ant', init, actions, model=model)
        assert full['done'][0, 1] and full['done'][0, 4] and np.isfinite(full['obs']).all()
        for h in (1, 3, 6):
            part = RA.rollout_actions(dm, 'ant', init, actions[:h], model=model)
            assert np.array_equal(part['obs'], full['obs'][:h + 1]) and np.array_equal(part['rew'], full['rew'][:h])
            assert np.array_equal(part['done'], full['done'][:h])
        # and a replay continued from row h with the remaining actions is the rest of the long one: no hidden state besides obs
        tail = RA.rollout_actions(dm, 'ant', full['obs'][3], actions[3:], model=model)
        assert np.array_equal(tail['obs'], full['obs'][3:]) and np.array_equal(tail['rew'], full['rew'][3:])
