"""CPU checks of the 'vpg' policy update (algos/vpg.py; training.py:337-352): the params-file wiring, the float64 restatement
tests/vpg_ref.py against torch autograd, and the two C entry points' argument checks (no GPU needed: they fail before the device)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import vpg_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIMMER = os.path.join(REPO, 'tests', 'golden', 'params_swimmer.json')


def _params(algo, **vpg):
    p = json.load(open(SWIMMER))
    p['algo'] = algo
    p['policy_opt_params']['vpg'].update(vpg)
    return p


def test_shapes_from_params_reads_the_vpg_block():
    from metrpo_amd import shapes_from_params
    p = _params('vpg', batch_size=12000, discount=0.99, init_std=0.5, reset=False)
    sh = shapes_from_params(p)
    assert sh['algo'] == 'vpg'
    assert sh['vpg'] == dict(discount=0.99, init_std=0.5, batch_size=12000, reset=False)
    # the sampler's batch comes from the vpg block (training.py:345), not from the trpo block (50 000 in this file)
    assert sh['batch_size'] == 12000 and sh['n_envs'] == 60 and sh['rounds'] == 1
    assert sh['trpo']['step_size'] == 0.01                     # the trpo block is still read, and unchanged
    trpo = shapes_from_params(_params('trpo', batch_size=12000))
    assert trpo['batch_size'] == 50000


def test_from_params_builds_vpg_and_still_refuses_svg():
    from metrpo_amd import from_params, VPG
    with pytest.raises(ValueError, match='svg'):
        from_params(_params('svg'))
    with pytest.raises(ValueError, match='l-bfgs'):
        from_params(_params('l-bfgs'))
    # without a GPU the Engine cannot be created, but the algorithm check in front of it must pass
    try:
        s = from_params(_params('vpg', batch_size=2000))
    except ValueError as e:
        assert "'algo'" not in str(e), str(e)
    except Exception:                                          # noqa: BLE001 -- no device here: anything past the algorithm check
        pass
    else:
        assert isinstance(s.algo, VPG) and s.optimize_policy_kwargs['reset_log_std'] is True


def _problem(dims=(6, 16, 12, 3), N=300, seed=3):
    rng = np.random.RandomState(seed)
    P = sum(i * j + j for i, j in zip(dims[:-1], dims[1:])) + dims[-1]
    theta = rng.randn(P) * 0.3
    theta[-dims[-1]:] = [-0.4, 0.3, -20.0]                      # the last log_std below log(1e-6): clamped, zero gradient
    obs = rng.randn(N, dims[0])
    act = rng.randn(N, dims[-1]) * 0.7
    adv = rng.randn(N)
    valid = rng.rand(N) > 0.2
    return theta, list(dims), obs, act, adv, valid


def test_vpg_ref_matches_autograd():
    theta, dims, obs, act, adv, valid = _problem()
    for kw in (dict(), dict(valid=valid), dict(valid=valid, n_global=1000)):
        l1, g1 = vpg_ref.loss_grad(theta, dims, obs, act, adv, **kw)
        l2, g2 = vpg_ref.loss_autograd(theta, dims, obs, act, adv, **kw)
        assert abs(l1 - l2) <= 1e-12 * max(1.0, abs(l2))
        np.testing.assert_allclose(g1, g2, rtol=1e-10, atol=1e-12)
        assert g1[-1] == 0.0 and g1[-3] != 0.0


def test_vpg_ref_gradient_is_npo_gradient_at_ratio_one():
    """At theta_old the likelihood ratio is 1 and d ratio = d logli: the VPG gradient equals the NPO surrogate's (oracle)."""
    from oracle import metrpo_oracle as O
    theta, dims, obs, act, adv, _ = _problem()
    theta[-1] = -0.2                                            # (the oracle's clamp derivative is not what is compared here)
    mean = O.policy_mean(theta, dims, obs)
    ls = np.broadcast_to(O.policy_log_std(theta, dims), mean.shape)
    _, g_npo = O.surrogate_loss_grad(theta, dims, obs, act, adv, mean, ls)
    _, g = vpg_ref.loss_grad(theta, dims, obs, act, adv)
    np.testing.assert_allclose(g, g_npo, rtol=1e-9, atol=1e-12)


def test_adam_step_is_tf_adam():
    rng = np.random.RandomState(0)
    th, m, v, g = rng.randn(5), rng.randn(5) * 0.1, rng.rand(5) * 0.01, rng.randn(5)
    th1, m1, v1, t1 = vpg_ref.adam_step(th, m, v, 3, g, lr=1e-2)
    assert t1 == 4
    np.testing.assert_allclose(m1, 0.9 * m + 0.1 * g, rtol=1e-13)
    np.testing.assert_allclose(v1, 0.999 * v + 0.001 * g * g, rtol=1e-13)
    lr_t = 1e-2 * np.sqrt(1 - 0.999 ** 4) / (1 - 0.9 ** 4)
    np.testing.assert_allclose(th1, th - lr_t * m1 / (np.sqrt(v1) + 1e-8), rtol=1e-12)
    # the first step from zero state moves every coordinate by ~lr against the sign of its gradient
    th0, _, _, _ = vpg_ref.adam_step(th, np.zeros(5), np.zeros(5), 0, g, lr=1e-3)
    np.testing.assert_allclose(th0 - th, -1e-3 * np.sign(g), rtol=1e-5)


def test_vpg_abi_symbols_and_null_arguments():
    import metrpo_amd  # noqa: F401
    from metrpo_amd import _lib
    lib = _lib.lib
    for n in ('metrpo_vpg_loss_grad', 'metrpo_vpg_update'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.VpgParams) == 4 * 8
    assert lib.metrpo_abi_version() == 4
    b = _lib.Batch()
    p = _lib.VpgParams(1e-3, 0.9, 0.999, 1e-8)
    out = (C.c_double * 4)()
    assert lib.metrpo_vpg_loss_grad(None, C.byref(b), out, None) == -2          # METRPO_ENULL
    assert lib.metrpo_vpg_update(None, C.byref(b), C.byref(p), None, None) == -2
    assert lib.metrpo_vpg_update(None, C.byref(b), None, None, None) == -2


def test_first_order_optimizer_defaults():
    from metrpo_amd import FirstOrderOptimizer
    opt = FirstOrderOptimizer(batch_size=None, max_epochs=1)
    assert (opt.learning_rate, opt.beta1, opt.beta2, opt.epsilon) == (1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(NotImplementedError):
        FirstOrderOptimizer(batch_size=32, max_epochs=1)
    with pytest.raises(NotImplementedError):
        FirstOrderOptimizer(max_epochs=5)
    assert copy.copy(opt).last_loss is None
