"""CPU checks of the host side of PPO's KL penalty (use_kl_penalty, algos/ppo.py:120-153): PPO(use_kl_penalty=True) constructs, the three
penalty methods' float32 arithmetic and bounds, the params-file keys through from_params on a stub engine, what AdamOptimizer hands to the
engine, and the two C entry points' argument checks (no GPU needed: they fail before the device)."""
import ctypes as C

import numpy as np
import pytest

from test_ppo_host import _StubEngine, _params


class _KlStubEngine(_StubEngine):
    """test_ppo_host's stub engine plus the two entry points PPO(use_kl_penalty=True) asks its engine for (never called here)."""

    def ppo_kl_update(self, batch, **kw):
        raise AssertionError("host test: no device")

    def ppo_kl_loss_grad(self, batch, *a, **kw):
        raise AssertionError("host test: no device")


def _stub_setup(monkeypatch, **ppo):
    import metrpo_amd.engine
    from metrpo_amd import from_params
    monkeypatch.setattr(metrpo_amd.engine, 'Engine', _KlStubEngine)
    return from_params(_params('ppo', **ppo))


def test_ppo_with_use_kl_penalty_constructs(monkeypatch):
    from metrpo_amd import PPO
    s = _stub_setup(monkeypatch, use_kl_penalty=True)
    assert isinstance(s.algo, PPO) and s.algo.use_kl_penalty is True
    assert s.algo.kl_penalty == 1.0 and s.algo.step_size == 0.01          # ppo.py's constructor defaults
    assert s.algo._penalty_args() == dict(kl_penalty=1.0, step_size=0.01)
    algo = PPO(use_kl_penalty=True, initial_kl_penalty=0.3, step_size=0.02, env=s.algo.env, policy=s.algo.policy, baseline=s.algo.baseline)
    assert algo.kl_penalty == float(np.float32(0.3)) and algo.step_size == 0.02
    assert PPO(env=s.algo.env, policy=s.algo.policy, baseline=s.algo.baseline)._penalty_args() == dict()


def test_use_kl_penalty_needs_an_engine_with_the_penalty_entry_points(monkeypatch):
    import metrpo_amd.engine
    from metrpo_amd import PPO, from_params
    with pytest.raises(NotImplementedError, match='use_kl_penalty'):
        PPO(use_kl_penalty=True, env=None, policy=None, baseline=None)
    monkeypatch.setattr(metrpo_amd.engine, 'Engine', _StubEngine)          # an engine object without ppo_kl_update / ppo_kl_loss_grad
    with pytest.raises(NotImplementedError, match='ppo_kl_update'):
        from_params(_params('ppo', use_kl_penalty=True))
    assert from_params(_params('ppo')).algo.use_kl_penalty is False      # ... which still serves the unpenalised PPO


def test_from_params_reads_the_penalty_keys_and_their_defaults(monkeypatch):
    from metrpo_amd import shapes_from_params
    assert shapes_from_params(_params('ppo'))['ppo_kl'] == dict(use_kl_penalty=False, initial_kl_penalty=1.0, step_size=0.01)
    sh = shapes_from_params(_params('ppo', use_kl_penalty=True, initial_kl_penalty=4.0, step_size=0.05))
    assert sh['ppo_kl'] == dict(use_kl_penalty=True, initial_kl_penalty=4.0, step_size=0.05)
    s = _stub_setup(monkeypatch, use_kl_penalty=True, initial_kl_penalty=4.0, step_size=0.05, n_epochs=3)
    assert (s.algo.use_kl_penalty, s.algo.initial_kl_penalty, s.algo.kl_penalty, s.algo.step_size) == (True, 4.0, 4.0, 0.05)
    assert s.algo.optimizer.n_epochs == 3
    d = _stub_setup(monkeypatch)
    assert d.algo.use_kl_penalty is False and d.algo.kl_penalty == 1.0 and d.algo.step_size == 0.01


def test_penalty_methods_do_the_float32_arithmetic_of_the_tf_variable(monkeypatch):
    """ppo.py:133-153: min(beta * increase_factor, max_penalty), max(beta * decrease_factor, min_penalty), reset -- on a float32 variable."""
    from metrpo_amd import PPO
    s = _stub_setup(monkeypatch, use_kl_penalty=True)
    kw = dict(env=s.algo.env, policy=s.algo.policy, baseline=s.algo.baseline, use_kl_penalty=True)
    a = PPO(initial_kl_penalty=0.3, increase_penalty_factor=1.7, decrease_penalty_factor=0.3, min_penalty=1e-3, max_penalty=10.0, **kw)
    f = np.float32
    want = f(0.3)
    assert a.kl_penalty == float(want)
    for _ in range(3):
        want = np.minimum(want * f(1.7), f(10.0))
        assert a.f_increase_penalty() == float(want) == a.kl_penalty
    assert float(f(0.3) * f(1.7) * f(1.7) * f(1.7)) == a.kl_penalty != 0.3 * 1.7 ** 3            # float32 products, not float64 ones
    for _ in range(10):
        a.f_increase_penalty()
    assert a.kl_penalty == float(f(10.0))                        # the upper bound
    for _ in range(2):
        want = np.maximum(f(a.kl_penalty) * f(0.3), f(1e-3))
        assert a.f_decrease_penalty() == float(want)
    for _ in range(20):
        a.f_decrease_penalty()
    assert a.kl_penalty == float(f(1e-3))                        # the lower bound, as the float32 the variable holds
    assert a.f_reset_penalty() == float(f(0.3)) == a.kl_penalty
    d = PPO(**kw)                                                # the defaults: 1 -> 2 -> 4 ... 1e6; 1 -> 0.5 ... 1e-3
    assert [d.f_increase_penalty() for _ in range(3)] == [2.0, 4.0, 8.0]
    assert d.f_reset_penalty() == 1.0 and [d.f_decrease_penalty() for _ in range(2)] == [0.5, 0.25]
    assert d._penalty_args() == dict(kl_penalty=0.25, step_size=0.01)


class _RecordingEngine(object):
    comm_world = 0
    device = 'cpu'

    def __init__(self):
        self.calls = []

    def ppo_update(self, batch, **kw):
        self.calls.append(('ppo_update', kw)); return 'plain'

    def ppo_kl_update(self, batch, **kw):
        self.calls.append(('ppo_kl_update', kw)); return 'kl'


def test_adam_optimizer_dispatches_on_the_penalty():
    from metrpo_amd import AdamOptimizer
    opt, eng = AdamOptimizer(learning_rate=3e-4, n_epochs=2), _RecordingEngine()
    assert opt.optimize(eng, None, 0.2, 0.01) == 'plain'
    assert opt.optimize(eng, None, 0.2, 0.01, kl_penalty=2.0, step_size=0.05) == 'kl'
    assert [c[0] for c in eng.calls] == ['ppo_update', 'ppo_kl_update']
    kw = eng.calls[1][1]
    assert (kw['kl_penalty'], kw['step_size'], kw['n_epochs'], kw['clip_lr'], kw['entropy_bonus_coeff'], kw['lr']) == (2.0, 0.05, 2, 0.2, 0.01, 3e-4)
    assert 'kl_penalty' not in eng.calls[0][1]


def test_ppo_kl_abi_symbols_and_null_arguments():
    import metrpo_amd  # noqa: F401
    from metrpo_amd import _lib
    lib = _lib.lib
    for n in ('metrpo_ppo_kl_loss_grad', 'metrpo_ppo_kl_update'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert C.sizeof(_lib.PpoKlParams) == 2 * 8 and [f[0] for f in _lib.PpoKlParams._fields_] == ['kl_penalty', 'step_size']
    assert lib.metrpo_abi_version() == 4                         # entry points were added, none changed
    b, p, kp = _lib.Batch(), _lib.PpoParams(0.3, 0.0, 1e-3, 0.9, 0.999, 1e-8), _lib.PpoKlParams(1.0, 0.01)
    out = (C.c_double * 4)()
    assert lib.metrpo_ppo_kl_loss_grad(None, C.byref(b), C.byref(p), C.byref(kp), None, out, None) == -2          # METRPO_ENULL
    assert lib.metrpo_ppo_kl_update(None, C.byref(b), C.byref(p), C.byref(kp), 1, None, None, None) == -2
