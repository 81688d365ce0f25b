"""CPU checks of metrpo_amd.planning with a stand-in scorer (no GPU): the planner's logic is torch on whatever device the states live on, the device
only scores.  The GPU side is tests/test_gpu_score_actions.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrpo_amd
from metrpo_amd import planning as P

NS = 3


class Recorder(object):
    """A stand-in scorer that keeps everything it was shown: ret [K, B] = head offsets + fn(actions [T, B, na], start rows [B, ns])."""

    def __init__(self, fn, K=1):
        self.fn, self.K, self.calls = fn, K, []

    def __call__(self, actions, init):
        T, B, na = actions.shape
        S = init.shape[0]
        assert B % S == 0
        rows = init[torch.arange(B) // (B // S)]
        ret = self.fn(actions, rows)
        self.calls.append((actions.clone(), ret.clone()))
        return torch.stack([ret + 0.25 * k for k in range(self.K)])


def quadratic(target):
    """-sum (a - a*)^2 per candidate; target [S, T, na], the candidate's start row carries its state index in column 0"""
    def fn(actions, rows):
        tgt = target[rows[:, 0].long()].permute(1, 0, 2)               # [T, B, na]
        return -((actions - tgt) ** 2).sum(dim=(0, 2))
    return fn


def states_of(S):
    s = torch.zeros(S, NS)
    s[:, 0] = torch.arange(S, dtype=torch.float32)
    return s


def test_one_cem_iteration_is_the_numpy_restatement():
    S, T, na, N, E, alpha = 2, 4, 2, 24, 5, 0.25
    rng = np.random.RandomState(0)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    mean0 = rng.uniform(-0.5, 0.5, size=(S, T, na)).astype(np.float32)
    rec = Recorder(quadratic(target), K=3)
    out = P.plan_cem(None, states_of(S), T, N, E, 1, init_mean=mean0, init_std=0.7, alpha=alpha, min_std=0.05, generator=torch.Generator().manual_seed(11),
                     scorer=rec, na=na)
    # the restatement, from the same generator's draws
    eps = torch.randn(T, S, N, na, generator=torch.Generator().manual_seed(11), dtype=torch.float32).numpy()
    m0 = mean0.transpose(1, 0, 2)[:, :, None, :]                          # [T, S, 1, na]
    a = np.clip(m0 + np.float32(0.7) * eps, np.float32(-1), np.float32(1)).astype(np.float32)
    assert len(rec.calls) == 1 and np.array_equal(rec.calls[0][0].numpy(), a.reshape(T, S * N, na))
    assert (np.abs(a) == 1).any()                                         # the clip acted: the statistics below are of the CLIPPED elites
    scores = rec.calls[0][1].numpy().reshape(S, N) + np.float32(0.25)     # mean over the three heads' offsets 0, 0.25, 0.5
    for s in range(S):
        order = np.argsort(-scores[s], kind='stable')[:E]
        assert scores[s][order[E - 1]] > np.sort(scores[s])[::-1][E]      # no tie at the cut: the elite SET is defined
        el = a[:, s, order, :].astype(np.float64)                         # [T, E, na]
        e_mean = (el.sum(axis=1) / E).astype(np.float32)
        e_std = np.sqrt(((el - el.sum(axis=1, keepdims=True) / E) ** 2).sum(axis=1) / E).astype(np.float32)      # ddof 0
        np.testing.assert_array_equal(e_std, el.std(axis=1).astype(np.float32))
        want_mean = np.float32(alpha) * m0[:, s, 0] + np.float32(1 - alpha) * e_mean
        want_std = np.maximum(np.float32(alpha) * np.float32(0.7) + np.float32(1 - alpha) * e_std, np.float32(0.05))
        np.testing.assert_array_equal(out['actions'][s].numpy(), want_mean)
        np.testing.assert_array_equal(out['std'][s].numpy(), want_std)
        np.testing.assert_allclose(out['history'][0, s].item(), scores[s][order].mean(), rtol=1e-6)
        assert out['best_score'][s].item() == scores[s].max()
        np.testing.assert_array_equal(out['best_actions'][s].numpy(), a[:, s, int(np.argmax(scores[s]))])


def test_best_score_is_the_maximum_over_everything_the_scorer_saw():
    S, T, na, N = 3, 5, 2, 16
    target = torch.as_tensor(np.random.RandomState(1).uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    rec = Recorder(quadratic(target))
    out = P.plan_cem(None, states_of(S), T, N, 4, 5, generator=torch.Generator().manual_seed(3), scorer=rec, na=na)
    assert len(rec.calls) == 5
    seen = torch.stack([r.reshape(S, N) for _, r in rec.calls])           # [iters, S, N]
    assert torch.equal(out['best_score'], seen.amax(dim=(0, 2)))
    for s in range(S):
        it, n = np.unravel_index(int(seen[:, s].argmax()), (5, N))
        assert torch.equal(out['best_actions'][s], rec.calls[it][0].reshape(T, S, N, na)[:, s, n])
    assert out['history'].shape == (5, S) and out['actions'].shape == (S, T, na) and out['std'].shape == (S, T, na)


@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4])
def test_cem_converges_on_a_separable_quadratic(seed):
    S, T, na, N, E, iters = 3, 5, 2, 64, 8, 6
    target = torch.as_tensor(np.random.RandomState(100 + seed).uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    out = P.plan_cem(None, states_of(S), T, N, E, iters, generator=torch.Generator().manual_seed(seed), scorer=Recorder(quadratic(target)), na=na)
    hist = out['history'].numpy()
    assert np.all(np.diff(hist, axis=0) > 0), hist                        # rises at every iteration, for every state
    d0 = torch.linalg.norm(target.reshape(S, -1), dim=1)                  # the start (zeros) to a*
    d1 = torch.linalg.norm((out['actions'] - target).reshape(S, -1), dim=1)
    print("seed %d: final / start distance %s" % (seed, (d1 / d0).numpy()))
    assert torch.all(d1 <= 0.5 * d0)


def test_aggregate_forms():
    ret = torch.tensor([[1.0, 5.0, -2.0], [3.0, 5.0, 0.0], [2.0, 2.0, 2.0]])              # [K = 3, B = 3]
    assert torch.equal(P.aggregate_heads(ret, 'mean'), torch.tensor([2.0, 4.0, 0.0]))
    assert torch.equal(P.aggregate_heads(ret, 'min'), torch.tensor([1.0, 2.0, -2.0]))
    std = ret.numpy().std(axis=0)                                         # ddof 0
    np.testing.assert_allclose(P.aggregate_heads(ret, ('pessimistic', 2.0)).numpy(), np.array([2.0, 4.0, 0.0]) - 2.0 * std, rtol=1e-6)
    assert torch.equal(P.aggregate_heads(ret[:1], ('pessimistic', 3.0)), ret[0])           # one head: no spread
    for bad in ('median', ('pessimistic',), ('optimistic', 1.0), 3):
        with pytest.raises(ValueError, match='aggregate'):
            P.aggregate_heads(ret, bad)
    # through the callers: the worst head of the stand-in is head 0 (offsets 0, 0.25, 0.5)
    S, T, na = 2, 3, 2
    target = torch.zeros(S, T, na)
    acts = torch.as_tensor(np.random.RandomState(2).uniform(-1, 1, size=(S, 4, T, na)), dtype=torch.float32)
    base = -(acts ** 2).sum(dim=(2, 3))
    rec = Recorder(quadratic(target), K=3)
    torch.testing.assert_close(P.score_action_sequences(None, states_of(S), acts, aggregate='min', scorer=rec), base)
    torch.testing.assert_close(P.score_action_sequences(None, states_of(S), acts, aggregate='mean', scorer=rec), base + 0.25)
    one = P.score_action_sequences(None, states_of(S), acts[:, 1], scorer=rec)              # [S, T, na]: one sequence per state
    assert one.shape == (S,)
    torch.testing.assert_close(one, base[:, 1] + 0.25)
    # candidate b = s * N + n starts from state s
    assert torch.equal(rec.calls[0][0].reshape(T, S, 4, na)[:, 1, 2], acts[1, 2])


def test_random_shooting_takes_the_argmax():
    S, T, na, N = 3, 4, 2, 32
    target = torch.as_tensor(np.random.RandomState(5).uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    rec = Recorder(quadratic(target))
    out = P.plan_random_shooting(None, states_of(S), T, N, generator=torch.Generator().manual_seed(0), scorer=rec, na=na)
    shown, ret = rec.calls[0]
    assert shown.min() >= -1 and shown.max() <= 1 and shown.min() < -0.9 and shown.max() > 0.9
    assert torch.equal(out['scores'], ret.reshape(S, N)) and torch.equal(out['score'], out['scores'].max(dim=1).values)
    for s in range(S):
        assert torch.equal(out['actions'][s], shown.reshape(T, S, N, na)[:, s, int(out['scores'][s].argmax())])


def test_controller_shifts_its_warm_start():
    S, T, na = 2, 4, 2
    target = torch.as_tensor(np.random.RandomState(7).uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    init_mean = np.arange(T * na, dtype=np.float32).reshape(T, na) / 10.0 - 0.3
    rec = Recorder(quadratic(target))
    ctl = P.ShootingController(None, T, 32, 6, 3, init_mean=init_mean, init_std=0.5, generator=torch.Generator().manual_seed(1), scorer=rec, na=na)
    a, info = ctl.get_actions(states_of(S).numpy())
    assert info == {} and a.shape == (S, na) and a.dtype == np.float64
    plan = ctl.last_plan['actions']
    np.testing.assert_array_equal(a, plan[:, 0].double().numpy())
    assert torch.equal(ctl._mean[:, :-1], plan[:, 1:])                    # one step on ...
    assert torch.equal(ctl._mean[:, -1], torch.as_tensor(init_mean[-1]).expand(S, na))      # ... the last row from init_mean
    # the next call starts from the shifted mean: with std 0 every candidate IS that mean
    rec.calls.clear()
    ctl.init_std = 0.0
    warm = ctl._mean.clone()
    ctl.get_actions(states_of(S).numpy())
    assert torch.equal(rec.calls[0][0].reshape(T, S, 32, na)[:, :, 5].permute(1, 0, 2), warm)
    ctl.reset([True, False])
    assert torch.equal(ctl._mean[0], torch.as_tensor(init_mean)) and not torch.equal(ctl._mean[1], torch.as_tensor(init_mean))
    ctl.reset()
    assert ctl._mean is None
    a1, _ = ctl.get_action(np.zeros(NS, np.float32))
    assert a1.shape == (na,)


def test_shape_errors():
    rec = Recorder(lambda a, r: a.sum(dim=(0, 2)))
    st = states_of(2)
    with pytest.raises(ValueError, match='an engine or a scorer'):
        P.plan_cem(None, st, 3, 8, 2, 1, na=2)
    with pytest.raises(ValueError, match='na is needed'):
        P.plan_cem(None, st, 3, 8, 2, 1, scorer=rec)
    with pytest.raises(ValueError, match=r'states: expected \[S, 3\]'):
        P.plan_cem(None, torch.zeros(2, 2, NS), 3, 8, 2, 1, scorer=rec, na=2)
    with pytest.raises(ValueError, match='n_elites must be in 1 ... n_candidates = 8'):
        P.plan_cem(None, st, 3, 8, 9, 1, scorer=rec, na=2)
    with pytest.raises(ValueError, match='n_iters must be positive'):
        P.plan_cem(None, st, 3, 8, 2, 0, scorer=rec, na=2)
    with pytest.raises(ValueError, match='horizon and n_candidates must be positive'):
        P.plan_cem(None, st, 0, 8, 2, 1, scorer=rec, na=2)
    with pytest.raises(ValueError, match='alpha must be in'):
        P.plan_cem(None, st, 3, 8, 2, 1, alpha=1.0, scorer=rec, na=2)
    with pytest.raises(ValueError, match=r'init_mean: expected a scalar, \[3, 2\] or \[2, 3, 2\]'):
        P.plan_cem(None, st, 3, 8, 2, 1, init_mean=np.zeros((2, 2)), scorer=rec, na=2)
    with pytest.raises(ValueError, match=r'actions: expected \[2, N, T, 2\] or \[2, T, 2\]'):
        P.score_action_sequences(None, st, torch.zeros(3, 4, 2), scorer=rec)
    with pytest.raises(ValueError, match='horizon and n_candidates must be positive'):
        P.plan_random_shooting(None, st, 3, 0, scorer=rec, na=2)


def test_names_and_abi_without_a_gpu():
    from metrpo_amd import _lib
    for name in ('planning', 'score_action_sequences', 'plan_random_shooting', 'plan_cem', 'ShootingController'):
        assert name in metrpo_amd.__all__ and hasattr(metrpo_amd, name)
    assert metrpo_amd.plan_cem is P.plan_cem and hasattr(metrpo_amd.Engine, 'score_actions') and hasattr(metrpo_amd.Engine, 'last_score_actions_kernel')
    lib = _lib.lib
    assert lib.metrpo_abi_version() == 4
    assert 'metrpo_score_actions' in _lib.SYMBOLS and 'metrpo_last_score_actions_kernel' in _lib.SYMBOLS
    assert lib.metrpo_score_actions(None, C.byref(_lib.ScoreActionsArgs()), None) == -2        # METRPO_ENULL
    assert lib.metrpo_score_actions(None, None, None) == -2
    assert lib.metrpo_last_score_actions_kernel(None) == -2
    # the struct as the header lays it out (LP64): five int32, padding to 8, a double, six pointers
    assert C.sizeof(_lib.ScoreActionsArgs) == 5 * 4 + 4 + 8 + 6 * 8
    assert _lib.ScoreActionsArgs.gamma.offset == 24 and _lib.ScoreActionsArgs.d_init_obs.offset == 32
