"""CPU side of the model diagnostics (metrpo_amd.model_error; env_helpers.py:96-172, :175-269): the float64 restatement the GPU tests compare
with, pinned on a case computed by hand; the argument errors of the host functions (raised before the device is touched); the horizon-above-T skip;
the ABI's argument checks that need no device."""
import ctypes as C
import warnings

import numpy as np
import pytest

from oracle import metrpo_oracle as O
import model_error_ref as R


class FakeEngine(object):
    """What the host functions read of an Engine before they touch the device."""
    ns, na, K = 10, 2, 5
    device = 'cpu'
    _ctx = None


# ---- the hand case: a linear "model" s' = s + c through identity activations, zero policy, real system s' = s + d ----------------------------------
def hand_case():
    ns, na, n_drop = O.ENV_SPECS['swimmer']
    K, hid, nin = 2, 3, ns + na - n_drop
    rng = np.random.RandomState(0)
    c = np.stack([rng.randn(ns) * 0.1, rng.randn(ns) * 0.1])                 # per head
    Ws = [np.zeros((K, nin, hid)), np.zeros((K, hid, ns))]
    bs = [np.zeros((K, hid)), c.copy()]
    dm = O.DynamicsEnsemble(Ws, bs, ['identity'], np.zeros(ns + na), np.ones(ns + na), np.zeros(ns), np.ones(ns), n_drop, ns, na)
    pdims = O.policy_dims(ns, (4,), na)
    theta = np.zeros(O.policy_num_params(pdims))                            # mean action 0
    n, T = 2, 4
    d = rng.randn(ns) * 0.1
    base = rng.randn(n, ns)
    Os = base[:, None, :] + np.arange(T + 1)[None, :, None] * d[None, None, :]
    Rs = Os[:, 1:, 5].copy()                                                # the real reward: swimmer's x_next[5], zero action (com_swimmer_env.py:112-114)
    return dm, theta, pdims, c, d, Os, Rs, n, T


@pytest.mark.parametrize('model', [-1, 0, 1])
def test_restatement_on_the_hand_case(model):
    dm, theta, pdims, c, d, Os, Rs, n, T = hand_case()
    cm = c.mean(axis=0) if model < 0 else c[model]
    err = R.evaluate_model_predictions(dm, theta, pdims, 'swimmer', Os, Rs, timesteps=(1, 2, 4), model=model)
    assert err['dropped'] == [0, 0, 0]
    for p, h in enumerate((1, 2, 4)):
        e = err['per_h'][p]
        N = n * (T + 1 - h)                                                 # Os[:, :-h]: T + 1 - h windows per trajectory
        assert e['state_diff'].shape == (N, dm.ns) and e['keep'].all()
        assert err['state_diff']['batch_size'][p] == N and err['cost_diff']['batch_size'][p] == N
        np.testing.assert_allclose(e['state_diff'], np.broadcast_to(h * np.abs(cm - d), (N, dm.ns)), rtol=0, atol=1e-13)
        np.testing.assert_allclose(e['cost_diff'], h * (h + 1) / 2 * abs(d[5] - cm[5]), rtol=0, atol=1e-13)
        assert np.array_equal(e['i'], np.repeat(np.arange(n), T + 1 - h)) and np.array_equal(e['t'], np.tile(np.arange(T + 1 - h), n))
        np.testing.assert_allclose(err['l1_sum'][p], h * np.abs(cm - d).sum(), rtol=1e-13)
        assert err['l2_sum'][p] == err['l1_sum'][p]                         # env_helpers.py:163
        np.testing.assert_allclose(err['l1_state_cost'][p], h * abs(cm[-1] - d[-1]), rtol=1e-12)
        for k in ('0%', '25%', '50%', '75%', '100%', 'avg'):
            np.testing.assert_allclose(err['state_diff'][k][p], h * np.abs(cm - d), rtol=0, atol=1e-13)


def test_restatement_known_actions_and_error_distribution_on_the_hand_case():
    """With zero recorded actions the known_actions pass is the policy pass (the policy's mean is 0); get_error_distribution at horizon = T is
    the t = 0 window of the T-step pass, signed."""
    dm, theta, pdims, c, d, Os, Rs, n, T = hand_case()
    As = np.zeros((n, T, dm.na))
    a = R.horizon_errors(dm, theta, pdims, 'swimmer', Os, Rs, 2, model=1)
    b = R.horizon_errors(dm, theta, pdims, 'swimmer', Os, Rs, 2, model=1, As=As, known_actions=True)
    assert np.array_equal(a['state_diff'], b['state_diff']) and np.array_equal(a['cost_diff'], b['cost_diff'])
    real_costs = -Rs.sum(axis=1)
    e_cost, e_state, keep = R.get_error_distribution(dm, theta, pdims, 'swimmer', Os[:, 0], As, real_costs, Os[:, T], T, model=1, known_actions=True)
    assert keep.all()
    np.testing.assert_allclose(e_state, np.broadcast_to(T * (c[1] - d), (n, dm.ns)), rtol=0, atol=1e-13)
    np.testing.assert_allclose(e_cost, T * (T + 1) / 2 * (d[5] - c[1][5]), rtol=0, atol=1e-13)


def test_restatement_drops_a_window_behind_a_done():
    """Ant: a window whose predicted z leaves [0.2, 1.0] at step s serves horizons <= s only... the step's own state is still compared at no horizon
    above it: done at step index s (0-based) drops every h >= s + 1."""
    dm, theta, pdims, pool = O.make_problem('ant', K=2, dyn_hidden=(8, 8), pol_hidden=(4,), seed=3, n_pool=8)
    Os, As, Rs = R.recorded_trajectories(dm, theta, pdims, 'ant', pool, 2, 4, seed=1)
    Os[1, 2, 2] = 1.5                                                       # window (1, 2) starts outside the healthy range and stays there
    e1 = R.horizon_errors(dm, theta, pdims, 'ant', Os, Rs, 1)
    w = 1 * 4 + 2                                                           # T + 1 - h = 4 windows per trajectory at h = 1
    assert not e1['keep'][w] and e1['keep'].sum() == len(e1['keep']) - 1
    err = R.evaluate_model_predictions(dm, theta, pdims, 'ant', Os, Rs, timesteps=(1, 2))
    assert err['dropped'] == [1, 1] and err['state_diff']['batch_size'] == [7, 5]


# ---- host functions: argument errors before the device is touched ------------------------------------------------------------------------------------
def test_host_argument_errors():
    from metrpo_amd import model_error as M
    eng = FakeEngine()
    Os, As, Rs = np.zeros((3, 13, 10), np.float32), np.zeros((3, 12, 2), np.float32), np.zeros((3, 12), np.float32)
    with pytest.raises(ValueError, match=r'Os: expected \[n, T \+ 1, 10\]'):
        M.evaluate_model_predictions(eng, np.zeros((3, 13, 9)), As, Rs)
    with pytest.raises(ValueError, match='Os: expected'):
        M.evaluate_model_predictions(eng, np.zeros((3, 1, 10)), As, Rs)           # T = 0
    with pytest.raises(ValueError, match='positive integers'):
        M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(0, 3))
    with pytest.raises(ValueError, match='positive integers'):
        M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=())
    with pytest.raises(ValueError, match='must not repeat'):
        M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(1, 3, 3))
    with pytest.raises(ValueError, match='Rs: expected'):
        M.evaluate_model_predictions(eng, Os, As, np.zeros((3, 13)), timesteps=(1, 3))
    with pytest.raises(ValueError, match='neither -1'):
        M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(1, 3), model=5)
    with pytest.raises(ValueError, match='neither -1'):
        M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(1, 3), model=-2)
    with pytest.raises(ValueError, match='at most 32 horizons'):
        M.evaluate_model_predictions(eng, np.zeros((1, 41, 10)), None, np.zeros((1, 40)), timesteps=tuple(range(1, 34)))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match='no horizon'):
            M.evaluate_model_predictions(eng, Os, As, Rs, timesteps=(13, 100))
    init, fin, rc = np.zeros((4, 10)), np.zeros((4, 10)), np.zeros(4)
    with pytest.raises(ValueError, match='initial_states'):
        M.get_error_distribution(eng, np.zeros((4, 9)), None, rc, fin, 5)
    with pytest.raises(ValueError, match='horizon must be positive'):
        M.get_error_distribution(eng, init, None, rc, fin, 0)
    with pytest.raises(ValueError, match='real_final_states / real_costs'):
        M.get_error_distribution(eng, init, None, np.zeros(3), fin, 5)
    with pytest.raises(ValueError, match='actions: expected'):
        M.get_error_distribution(eng, init, np.zeros((4, 4, 2)), rc, fin, 5, known_actions=True)
    with pytest.raises(ValueError, match='neither -1'):
        M.get_error_distribution(eng, init, None, rc, fin, 5, model=7)


def test_horizons_above_T_are_skipped_with_a_warning():
    from metrpo_amd import model_error as M
    with pytest.warns(UserWarning, match=r'horizons \[15, 18, 20, 100\] exceed the recorded length T = 12'):
        assert M._horizons(M.TIMESTEPS, 12) == [1, 3, 5, 7, 10, 12]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert M._horizons((12, 1, 5), 12) == [1, 5, 12]                            # T itself is served, unsorted input is sorted, no warning
    assert M.TIMESTEPS == (1, 3, 5, 7, 10, 12, 15, 18, 20, 100)                     # env_helpers.py:107


def test_abi_symbols_struct_and_null_checks():
    from metrpo_amd import _lib
    lib = _lib.lib
    for n in ('metrpo_model_error', 'metrpo_model_error_windows'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    # 3 pointers, n, T, hs pointer, n_h + 4 flags (padded to 8), 4 outputs, 4 debug pointers (LP64; include/metrpo.h)
    assert C.sizeof(_lib.ModelErrorArgs) == 3 * 8 + 2 * 4 + 8 + 5 * 4 + 4 + 4 * 8 + 4 * 8
    assert _lib.ModelErrorArgs.hs.offset == 32 and _lib.ModelErrorArgs.d_state_diff.offset == 64
    assert lib.metrpo_model_error(None, None, None) == -2                           # METRPO_ENULL
    assert lib.metrpo_model_error_windows(None, None, 1, 1, None, None) == -2
    assert lib.metrpo_abi_version() == 4
