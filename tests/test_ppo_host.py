"""CPU checks of the 'ppo' policy update's host side: the params-file 'ppo' block and its defaults (an extension: the reference's training.py
has no such branch), what PPO and AdamOptimizer refuse, the PPO constructor surface of algos/ppo.py, and the two C entry points' argument
checks (no GPU needed: they fail before the device)."""
import ctypes as C
import inspect
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIMMER = os.path.join(REPO, 'tests', 'golden', 'params_swimmer.json')


def _params(algo, **ppo):
    p = json.load(open(SWIMMER))
    p['algo'] = algo
    if ppo:
        p['policy_opt_params']['ppo'] = ppo
    return p


def test_shapes_from_params_reads_the_ppo_block_and_its_defaults():
    from metrpo_amd import shapes_from_params
    sh = shapes_from_params(_params('ppo'))
    # ppo.py's defaults (clip_lr, entropy_bonus_coeff), AdamOptimizer's (n_epochs, learning_rate), the vpg block's for the rest
    assert sh['ppo'] == dict(discount=1.0, init_std=1.0, batch_size=5000, reset=True, clip_lr=0.3, n_epochs=10, learning_rate=1e-3,
                             entropy_bonus_coeff=0.0)
    assert sh['algo'] == 'ppo' and sh['batch_size'] == 5000
    sh = shapes_from_params(_params('ppo', batch_size=12000, discount=0.99, init_std=0.5, reset=False, clip_lr=0.2, n_epochs=4,
                                    learning_rate=3e-4, entropy_bonus_coeff=0.01))
    assert sh['ppo'] == dict(discount=0.99, init_std=0.5, batch_size=12000, reset=False, clip_lr=0.2, n_epochs=4, learning_rate=3e-4,
                             entropy_bonus_coeff=0.01)
    assert sh['batch_size'] == 12000 and sh['n_envs'] == 60            # the sampler's batch comes from the block of the algorithm that runs
    assert shapes_from_params(_params('trpo', batch_size=12000))['batch_size'] == 50000
    assert shapes_from_params(_params('vpg', batch_size=12000))['vpg'] == shapes_from_params(_params('vpg'))['vpg']      # the other blocks are unchanged


class _StubEngine(object):
    """What from_params' constructors ask of an Engine (shape attributes, set_policy / get_policy), with no device and no library call: the
    'ppo' branch of from_params -- PPO, AdamOptimizer, the sampler, the kwargs of the early-stop loop -- is host code and runs through."""
    device = 'cpu'

    def __init__(self, env, K, dyn_hidden, pol_hidden, n_drop=0, dyn_act='relu', device=0):
        from metrpo_amd import synthetic
        self.env_name, self.K, self.dyn_hidden, self.pol_hidden = env, K, tuple(dyn_hidden), tuple(pol_hidden)
        self.ns, self.na = synthetic.ENV_SPECS[env][:2]
        dims = (self.ns,) + self.pol_hidden + (self.na,)
        self.P = sum(a * b + b for a, b in zip(dims[:-1], dims[1:])) + self.na
        self.theta = None

    def set_policy(self, theta):
        import numpy as np
        theta = np.asarray(theta, dtype=np.float32)
        assert theta.size == self.P
        self.theta = theta.copy()


def test_from_params_builds_ppo_and_still_refuses_svg_and_lbfgs(monkeypatch):
    import numpy as np
    import metrpo_amd.engine
    from metrpo_amd import from_params, PPO, AdamOptimizer
    with pytest.raises(ValueError, match='svg'):
        from_params(_params('svg'))
    with pytest.raises(ValueError, match='l-bfgs'):
        from_params(_params('l-bfgs'))
    monkeypatch.setattr(metrpo_amd.engine, 'Engine', _StubEngine)
    s = from_params(_params('ppo', batch_size=2000, n_epochs=3, clip_lr=0.2, learning_rate=3e-4, entropy_bonus_coeff=0.01, discount=0.99,
                            init_std=0.5, reset=False))
    assert isinstance(s.engine, _StubEngine) and isinstance(s.algo, PPO) and isinstance(s.algo.optimizer, AdamOptimizer)
    assert (s.algo.optimizer.n_epochs, s.algo.optimizer.learning_rate, s.algo.optimizer.batch_size) == (3, 3e-4, None)
    assert (s.algo.clip_lr, s.algo.entropy_bonus_coeff, s.algo.discount, s.algo.batch_size) == (0.2, 0.01, 0.99, 2000)
    assert s.algo.max_path_length == s.shapes['T'] and s.algo.use_kl_penalty is False
    assert s.optimize_policy_kwargs['reset_log_std'] is False and s.bptt is None
    na = s.engine.na
    np.testing.assert_allclose(s.engine.theta[-na:], np.log(0.5), rtol=1e-6)       # init_std of the ppo block reached the policy
    d = from_params(_params('ppo'))                                                # the block's defaults
    assert (d.algo.clip_lr, d.algo.entropy_bonus_coeff, d.algo.optimizer.n_epochs, d.algo.optimizer.learning_rate) == (0.3, 0.0, 10, 1e-3)
    assert d.optimize_policy_kwargs['reset_log_std'] is True and d.algo.batch_size == 5000


def test_adam_optimizer_defaults_and_minibatch_raises():
    from metrpo_amd import AdamOptimizer, FirstOrderOptimizer
    opt = AdamOptimizer()
    assert (opt.learning_rate, opt.n_epochs, opt.batch_size, opt.beta1, opt.beta2, opt.epsilon) == (1e-3, 10, None, 0.9, 0.999, 1e-8)
    assert AdamOptimizer(learning_rate=3e-4, n_epochs=2).n_epochs == 2
    with pytest.raises(NotImplementedError):
        AdamOptimizer(batch_size=32)
    with pytest.raises(NotImplementedError):                   # the existing class keeps its pinned behaviour
        FirstOrderOptimizer(batch_size=32, max_epochs=1)


def test_ppo_constructor_surface():
    """The reference's signature (ppo.py:17-40), name by name and default by default; use_kl_penalty raises before anything is built."""
    from metrpo_amd import PPO, BatchPolopt
    assert issubclass(PPO, BatchPolopt)
    sig = inspect.signature(PPO.__init__)
    want = dict(clip_lr=0.3, increase_penalty_factor=2, decrease_penalty_factor=0.5, min_penalty=1e-3, max_penalty=1e6, entropy_bonus_coeff=0.,
                gradient_clipping=40., log_loss_kl_before=True, log_loss_kl_after=True, use_kl_penalty=False, initial_kl_penalty=1.,
                use_line_search=True, max_backtracks=10, backtrack_ratio=0.5, optimizer=None, step_size=0.01, min_n_epochs=2,
                adaptive_learning_rate=False, max_learning_rate=1e-3, min_learning_rate=1e-5)
    got = {k: v.default for k, v in sig.parameters.items() if k not in ('self', 'kwargs')}
    assert got == want and list(got) == list(want)
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())
    with pytest.raises(NotImplementedError, match='use_kl_penalty'):
        PPO(use_kl_penalty=True, env=None, policy=None, baseline=None)
    for name in ('init_opt', 'optimize_policy', 'get_itr_snapshot', 'start_worker', 'obtain_samples', 'process_samples'):
        assert callable(getattr(PPO, name))


def test_ppo_abi_symbols_and_null_arguments():
    import metrpo_amd  # noqa: F401
    from metrpo_amd import _lib
    lib = _lib.lib
    for n in ('metrpo_ppo_loss_grad', 'metrpo_ppo_update'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.PpoParams) == 6 * 8
    assert [f[0] for f in _lib.PpoParams._fields_] == ['clip_lr', 'entropy_bonus_coeff', 'lr', 'beta1', 'beta2', 'eps']
    assert lib.metrpo_abi_version() == 4
    b = _lib.Batch()
    p = _lib.PpoParams(0.3, 0.0, 1e-3, 0.9, 0.999, 1e-8)
    out = (C.c_double * 4)()
    assert lib.metrpo_ppo_loss_grad(None, C.byref(b), C.byref(p), out, None) == -2          # METRPO_ENULL
    assert lib.metrpo_ppo_update(None, C.byref(b), C.byref(p), 1, None, None) == -2
