"""CPU checks of the 'svg' policy update's host side (me-trpo_amd/svg.py, the SVG branch of early_stop.optimize_policy) on a stub engine, and of the
two C entry points' argument checks that fail before the device."""
import ctypes as C

import numpy as np
import pytest


class _StubEngine(object):
    """What SVG and the early-stop loop ask of an Engine: shapes, svg_grad / svg_update, get_policy / set_policy, validation_cost.  The "gradient"
    is a fixed vector, so the policy after k updates is known; validation costs are scripted."""
    device = 'cpu'
    env_name = 'swimmer'

    def __init__(self, costs, ns=10, na=2, P=7):
        import torch
        self.ns, self.na, self.P, self.K = ns, na, P, 2
        self.theta = torch.zeros(P)
        self.costs = list(costs)
        self.calls = []

    def get_policy(self):
        return self.theta

    def set_policy(self, theta):
        self.theta = theta.clone()

    def validation_cost(self, s0, T, gamma):
        import torch
        return torch.full((self.K,), float(self.costs.pop(0)), dtype=torch.float64)

    def svg_grad(self, obs, act, lengths=None, model=0, gamma=1.0, path=0, chunk=0, jacobians=False):
        import torch
        self.calls.append(('grad', tuple(obs.shape), tuple(act.shape), lengths.tolist(), model, gamma))
        return dict(theta=torch.ones(self.P, dtype=torch.float64), state=torch.zeros(self.ns, dtype=torch.float64))

    def svg_update(self, obs, act, lr, lengths=None, model=0, gamma=1.0, path=0, chunk=0, jacobians=False):
        self.calls.append(('update', tuple(obs.shape), tuple(act.shape), lengths.tolist(), model, gamma, lr))
        self.theta = self.theta - lr                                    # theta += -lr * 1
        return self.svg_grad(obs, act, lengths, model, gamma)


def _rollouts(lens, ns=10, na=2, seed=0):
    from metrpo_amd import rollout_triplets
    rng = np.random.RandomState(seed)
    Os = [rng.randn(L + 1, ns) for L in lens]
    As = [rng.randn(L, na) for L in lens]
    return Os, As, rollout_triplets(Os, As)


def test_rollout_triplets_and_pack_rollouts():
    from metrpo_amd import pack_rollouts
    from metrpo_amd.svg import check_lengths
    Os, As, data = _rollouts([4, 1, 3])
    assert [len(r) for r in data] == [4, 1, 3] and all(len(t) == 3 for r in data for t in r)
    assert data[2][1][0] is not None and np.array_equal(data[2][1][0], Os[2][1]) and np.array_equal(data[2][1][1], As[2][1]) \
        and np.array_equal(data[2][1][2], Os[2][2])                                        # (o[t], a[t], o[t+1]), model_based_rl.py:804
    obs, act, lengths = pack_rollouts(data)
    assert obs.shape == (3, 4, 10) and act.shape == (3, 4, 2) and obs.dtype == np.float32 and lengths.dtype == np.int32
    assert lengths.tolist() == [4, 1, 3]
    for r, L in enumerate(lengths):
        assert np.array_equal(obs[r, :L], Os[r][:L].astype(np.float32)) and np.array_equal(act[r, :L], As[r][:L].astype(np.float32))
        assert not obs[r, L:].any() and not act[r, L:].any()                                # zero padding, s_t+1 not packed
    with pytest.raises(ValueError, match='no rollout'):
        pack_rollouts([])
    with pytest.raises(ValueError, match='empty'):
        pack_rollouts([data[0], []])
    with pytest.raises(ValueError, match='expected 10 and 2'):
        pack_rollouts([data[0], [(np.zeros(9), np.zeros(2), np.zeros(9))]])
    with pytest.raises(ValueError, match='expected 11 and 2'):
        pack_rollouts(data, ns=11)
    assert check_lengths(np.array([4, 1, 3]), 3, 4).dtype == np.int32
    for bad in (np.array([4, 0, 3]), np.array([5, 1, 3]), np.array([4, 1]), np.array([4., 1., 3.])):
        with pytest.raises(ValueError, match='lengths'):
            check_lengths(bad, 3, 4)


def test_svg_object_packs_once_and_passes_its_settings():
    from metrpo_amd import SVG
    _, _, data = _rollouts([4, 1, 3])
    eng = _StubEngine([])
    svg = SVG(eng, learning_rate=0.25, model=1, gamma=0.9)
    g = svg.svg_gradient(data)
    assert set(g) == {'theta', 'state'} and g['theta'].shape == (eng.P,) and g['state'].shape == (eng.ns,)
    assert eng.calls[-1] == ('grad', (3, 4, 10), (3, 4, 2), [4, 1, 3], 1, 0.9)
    packed = svg._packed[1]
    svg.svg_update(data)
    assert svg._packed[1] is packed                                                         # the same rollout_data is not packed again
    assert eng.calls[-2][0] == 'update' and eng.calls[-2][-1] == 0.25 and float(eng.theta[0]) == -0.25
    with pytest.raises(ValueError, match='rollout_data'):
        svg.optimize_policy_iteration(None)
    svg.rollout_data = data
    assert svg.optimize_policy_iteration(None) == 0.0 and float(eng.theta[0]) == -0.5        # training cost 0.0, model_based_rl.py:1206
    ant = _StubEngine([]); ant.env_name = 'ant'
    with pytest.raises(ValueError, match='Ant'):
        SVG(ant, 0.1)


def test_early_stop_branch_keeps_or_restores_and_reports_zero_training_cost():
    from metrpo_amd import SVG, early_stop
    _, _, data = _rollouts([4, 1, 3])
    # entry cost 10; validation rounds (log_every = 2) after iterations 2, 4, 6: better, worse, worse -> the policy of iteration 2 is kept
    eng = _StubEngine([10.0, 5.0, 50.0, 60.0])
    svg = SVG(eng, learning_rate=1.0)
    res = early_stop.optimize_policy(svg, np.zeros((4, 10), np.float32), 3, 1.0, mode='estimated', log_every=2, num_iters_threshold=4, max_iters=6,
                                     init_pool=data)
    assert res['training_costs'] == [0.0] * 6 and res['last_index'] == 6 and res['best_index'] == 2
    assert [c[0] for c in eng.calls].count('update') == 6                                   # one svg_update on the same rollout_data per iteration
    assert float(eng.theta[0]) == -2.0                                                      # restored to the snapshot of iteration 2, not the entry policy
    assert [h[0] for h in res['history']] == [2, 4, 6]
    # nothing ever better: the entry policy is restored
    eng = _StubEngine([1.0, 5.0, 6.0])
    res = early_stop.optimize_policy(SVG(eng, 1.0), np.zeros((4, 10), np.float32), 3, 1.0, log_every=1, num_iters_threshold=2, max_iters=9, init_pool=data)
    assert res['best_index'] == 0 and res['last_index'] == 2 and float(eng.theta[0]) == 0.0
    with pytest.raises(ValueError, match='rollout_data'):
        early_stop.optimize_policy(SVG(_StubEngine([1.0]), 1.0), np.zeros((4, 10), np.float32), 3, 1.0)


def test_from_params_still_refuses_svg_and_the_package_exports_the_new_names():
    import json
    import os
    import metrpo_amd
    p = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'params_swimmer.json')))
    p['algo'] = 'svg'
    with pytest.raises(ValueError, match='svg'):
        metrpo_amd.from_params(p)
    for name in ('SVG', 'rollout_triplets', 'pack_rollouts', 'svg'):
        assert name in metrpo_amd.__all__ and hasattr(metrpo_amd, name)
    for name in ('svg_grad', 'svg_update', 'last_svg_path'):
        assert callable(getattr(metrpo_amd.Engine, name))


def test_svg_abi_symbols_struct_and_null_arguments():
    import metrpo_amd  # noqa: F401
    from metrpo_amd import _lib
    lib = _lib.lib
    for n in ('metrpo_svg_grad', 'metrpo_svg_update', 'metrpo_last_svg_path'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert [f[0] for f in _lib.SvgArgs._fields_] == ['d_obs', 'd_act', 'd_len', 'n', 'T', 'model', 'path', 'chunk', 'gamma', 'd_grad', 'd_state_grad',
                                                     'd_mean_adj', 'd_dyn_jac', 'd_pol_jac']
    assert C.sizeof(_lib.SvgArgs) == 3 * 8 + 5 * 4 + 4 + 8 + 5 * 8 and _lib.SvgArgs.gamma.offset == 48 and _lib.SvgArgs.n.offset == 24
    assert lib.metrpo_abi_version() == 4
    a = _lib.SvgArgs()
    assert lib.metrpo_svg_grad(None, C.byref(a), None) == -2                                # METRPO_ENULL
    assert lib.metrpo_svg_update(None, C.byref(a), 0.1, None) == -2
    assert lib.metrpo_last_svg_path(None) == -2
