"""CPU checks of the first-order part of metrpo_amd.planning with stand-in gradient scorers (no GPU): aggregate_heads_grad, refine_actions,
plan_cem_gd and the controller's new keywords run on whatever device the states live on; the device only scores and differentiates.  The GPU side is
tests/test_gpu_score_grad.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrpo_amd
from metrpo_amd import planning as P

NS = 3


def states_of(S):
    s = torch.zeros(S, NS)
    s[:, 0] = torch.arange(S, dtype=torch.float32)
    return s


class QuadGrad(object):
    """A stand-in gradient scorer on a separable concave quadratic: head k's return of candidate b is c_k - w_k sum (a - a*)^2 with a* the target of
    the candidate's start state (column 0 of its start row); the gradient is taken at the CLIPPED action and gated as the device gates it.  Keeps
    what it was shown."""

    def __init__(self, target, K=1):
        self.target, self.K, self.calls = target, K, []
        self.w = [1.0 + 0.5 * k for k in range(K)]
        self.c = [0.25 * k for k in range(K)]

    def __call__(self, actions, init):
        T, B, na = actions.shape
        S = init.shape[0]
        assert B % S == 0
        rows = init[torch.arange(B) // (B // S)]
        tgt = self.target[rows[:, 0].long()].permute(1, 0, 2)             # [T, B, na]
        u = torch.clamp(actions, -1.0, 1.0)
        gate = ((actions >= -1.0) & (actions <= 1.0)).to(actions.dtype)
        ret = torch.stack([c - w * ((u - tgt) ** 2).sum(dim=(0, 2)) for w, c in zip(self.w, self.c)])
        grad = torch.stack([-2.0 * w * (u - tgt) * gate for w in self.w])
        self.calls.append((actions.clone(), ret.clone(), grad.clone()))
        return ret, grad


@pytest.mark.parametrize('aggregate', ['mean', 'min', ('pessimistic', 0.7)], ids=['mean', 'min', 'pessimistic'])
@pytest.mark.parametrize('K', [1, 4])
def test_aggregate_heads_grad_is_autograd_of_aggregate_heads(aggregate, K):
    T, B, na = 3, 6, 2
    g = torch.Generator().manual_seed(5)
    a = torch.randn(T, B, na, generator=g, dtype=torch.float64, requires_grad=True)
    Wk = torch.randn(K, T, na, generator=g, dtype=torch.float64)
    ret = torch.stack([(torch.sin(a) * Wk[k][:, None, :]).sum(dim=(0, 2)) + (a ** 2).sum(dim=(0, 2)) * 0.1 * k for k in range(K)])     # [K, B]
    grad = torch.stack([torch.autograd.grad(ret[k].sum(), a, retain_graph=True)[0] for k in range(K)])                                # [K, T, B, na]
    got = P.aggregate_heads_grad(ret.detach(), grad, aggregate)
    assert got.shape == (T, B, na)
    if K == 1 and not isinstance(aggregate, str):
        want = grad[0]                                                    # std = 0: the std term is dropped (autograd of sqrt(0) is not finite)
    else:
        want = torch.autograd.grad(P.aggregate_heads(ret, aggregate).sum(), a)[0]
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match='aggregate'):
        P.aggregate_heads_grad(ret.detach(), grad, 'median')


def test_one_sgd_step_and_three_adam_steps_are_the_numpy_restatement():
    S, N, T, na, K = 2, 3, 4, 2, 3
    rng = np.random.RandomState(1)
    target = torch.as_tensor(rng.uniform(-0.9, 0.9, size=(S, T, na)), dtype=torch.float32)
    a0 = (0.9 * rng.randn(S, N, T, na)).astype(np.float32)
    assert (np.abs(a0) > 1).any()                                         # some entries start outside the box: gated, they do not move under SGD
    f = np.float32
    tgt = np.repeat(target.numpy()[:, None], N, axis=1)

    def grad_np(a):                                                       # mean over the heads, in fp32 as torch forms it: stack, then mean over dim 0
        u = np.clip(a, f(-1), f(1))
        gate = ((a >= -1) & (a <= 1)).astype(f)
        per = np.stack([f(-2.0) * f(w) * (u - tgt) * gate for w in (1.0, 1.5, 2.0)])
        return torch.as_tensor(per).mean(dim=0).numpy()

    lr = 0.05
    qs = QuadGrad(target, K)
    out = P.refine_actions(None, states_of(S), a0, 1, lr, optimizer='sgd', grad_scorer=qs)
    want = np.clip(a0 + f(lr) * grad_np(a0), f(-1), f(1))
    assert len(qs.calls) == 2 and np.array_equal(out['last'].numpy(), want)
    assert np.array_equal(out['last'].numpy()[np.abs(a0) > 1], np.clip(a0, -1, 1)[np.abs(a0) > 1])      # gated: only projected
    # three Adam steps, written out
    qs = QuadGrad(target, K)
    b1, b2, eps = 0.9, 0.999, 1e-8
    out = P.refine_actions(None, states_of(S), a0, 3, lr, optimizer='adam', betas=(b1, b2), eps=eps, grad_scorer=qs)
    a, m, v = a0.copy(), None, None
    for it in range(3):
        g = torch.as_tensor(grad_np(a))
        m = (1.0 - b1) * g if m is None else b1 * m + (1.0 - b1) * g
        v = (1.0 - b2) * g * g if v is None else b2 * v + (1.0 - b2) * g * g
        step = lr * (m / (1.0 - b1 ** (it + 1))) / (torch.sqrt(v / (1.0 - b2 ** (it + 1))) + eps)
        a = torch.clamp(torch.as_tensor(a) + step, -1.0, 1.0).numpy()
    assert len(qs.calls) == 4 and np.array_equal(out['last'].numpy(), a)
    # the first Adam step is lr * sign(g) up to eps: the restatement in plain NumPy, to rounding
    g0 = grad_np(a0)
    first = np.clip(a0 + lr * g0 / (np.abs(g0) + eps), -1, 1)
    np.testing.assert_allclose(qs.calls[1][0].numpy(), first.transpose(2, 0, 1, 3).reshape(T, S * N, na), rtol=1e-6, atol=1e-7)
    # [S, T, na]: one candidate per state
    one = P.refine_actions(None, states_of(S), a0[:, 0], 2, lr, grad_scorer=QuadGrad(target, K))
    assert one['actions'].shape == (S, T, na) and one['score'].shape == (S,)


def test_keep_best_never_lowers_a_score():
    S, N, T, na = 2, 5, 3, 2
    rng = np.random.RandomState(2)
    target = torch.as_tensor(rng.uniform(-0.9, 0.9, size=(S, T, na)), dtype=torch.float32)
    a0 = rng.uniform(-1, 1, size=(S, N, T, na)).astype(np.float32)
    for opt, lr in (('sgd', 0.9), ('adam', 0.8)):                         # steps far too long: the iterates overshoot and oscillate
        qs = QuadGrad(target, 2)
        out = P.refine_actions(None, states_of(S), a0, 6, lr, optimizer=opt, grad_scorer=qs, aggregate='min')
        assert torch.all(out['score'] >= out['initial_score'])
        assert (out['last_score'] < out['score']).any()                   # the last iterate is not the best everywhere: keep-best mattered
        # the returned actions score what is reported
        ret, _ = QuadGrad(target, 2)(P._device_major(out['actions']), states_of(S))
        assert torch.equal(P.aggregate_heads(ret, 'min').reshape(S, N), out['score'])
    zero = P.refine_actions(None, states_of(S), a0, 0, 0.1, grad_scorer=QuadGrad(target, 2))
    assert torch.equal(zero['actions'], torch.as_tensor(a0)) and torch.equal(zero['score'], zero['initial_score'])


def test_plan_cem_gd_needs_fewer_scoring_calls_than_plan_cem():
    S, T, na, N, E = 2, 6, 2, 64, 8
    rng = np.random.RandomState(4)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    goal = -0.01                                                         # of a maximum of 0

    def calls_until(plan):
        for n_iters in range(1, 61):
            qs = QuadGrad(target, 1)
            out = plan(n_iters, qs)
            if bool(torch.all(out['best_score'] >= goal)):
                return len(qs.calls)
        return None

    gen = lambda: torch.Generator().manual_seed(3)
    plain = calls_until(lambda n, qs: P.plan_cem(None, states_of(S), T, N, E, n, init_std=0.5, alpha=0.3, generator=gen(), scorer=lambda a, i: qs(a, i)[0], na=na))
    gd = calls_until(lambda n, qs: P.plan_cem_gd(None, states_of(S), T, N, E, n, grad_steps=2, grad_lr=0.4, optimizer='sgd', init_std=0.5, alpha=0.3, generator=gen(),
                                                 grad_scorer=qs, na=na))
    print("calls until every state's best score >= %g: plan_cem %s, plan_cem_gd %s" % (goal, plain, gd))
    assert gd is not None and (plain is None or gd < plain)
    # refine='all' runs and scores through the gradient scorer alone
    qs = QuadGrad(target, 2)
    out = P.plan_cem_gd(None, states_of(S), T, 8, 3, 2, grad_steps=2, grad_lr=0.1, refine='all', generator=gen(), grad_scorer=qs, na=na)
    assert len(qs.calls) == 2 * 3 and out['actions'].shape == (S, T, na) and out['elites'].shape == (S, 3)


def test_grad_steps_zero_is_plan_cem_bit_for_bit():
    S, T, na, N, E = 2, 4, 2, 24, 5
    rng = np.random.RandomState(0)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    mean0 = rng.uniform(-0.5, 0.5, size=(S, T, na)).astype(np.float32)
    kw = dict(init_mean=mean0, init_std=0.7, alpha=0.25, min_std=0.05, aggregate=('pessimistic', 0.5), na=na)
    qs = QuadGrad(target, 3)
    scorer = lambda a, i: qs(a, i)[0]
    want = P.plan_cem(None, states_of(S), T, N, E, 3, generator=torch.Generator().manual_seed(11), scorer=scorer, **kw)
    got = P.plan_cem_gd(None, states_of(S), T, N, E, 3, grad_steps=0, generator=torch.Generator().manual_seed(11), scorer=scorer, **kw)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    got = P.plan_cem_gd(None, states_of(S), T, N, E, 3, grad_steps=0, generator=torch.Generator().manual_seed(11), grad_scorer=qs, **kw)
    for k in want:                                                        # no scorer: the gradient scorer's returns
        assert torch.equal(got[k], want[k]), k


def test_controller_keywords():
    S, T, na = 2, 5, 2
    rng = np.random.RandomState(6)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)
    qs = QuadGrad(target, 2)
    kw = dict(horizon=T, n_candidates=16, n_elites=4, n_iters=2, init_std=0.5, scorer=lambda a, i: qs(a, i)[0], na=na)
    plain = P.ShootingController(None, generator=torch.Generator().manual_seed(1), **kw)
    zero = P.ShootingController(None, generator=torch.Generator().manual_seed(1), grad_steps=0, grad_lr=0.3, grad_scorer=qs, **kw)
    a_plain, _ = plain.get_actions(states_of(S).numpy())
    n_plain = len(qs.calls)
    a_zero, _ = zero.get_actions(states_of(S).numpy())
    assert np.array_equal(a_plain, a_zero) and len(qs.calls) == 2 * n_plain      # grad_steps = 0: today's behaviour, the same number of calls
    gd = P.ShootingController(None, generator=torch.Generator().manual_seed(1), grad_steps=2, grad_lr=0.1, grad_scorer=qs, **kw)
    del qs.calls[:]
    a_gd, info = gd.get_actions(states_of(S).numpy())
    assert a_gd.shape == (S, na) and a_gd.dtype == np.float64 and info == {}
    assert len(qs.calls) == 2 * (1 + 3)                                   # per iteration: one scoring call, then 2 + 1 gradient calls on the elites
    assert torch.all(gd.last_plan['best_score'] >= plain.last_plan['best_score'])        # same draws in iteration 0, refined elites
    assert torch.equal(gd._mean[:, :-1], gd.last_plan['actions'][:, 1:])  # the warm start is kept as before
    with pytest.raises(ValueError, match='n_steps must not be negative'):
        P.ShootingController(None, grad_steps=-1, **kw)
    with pytest.raises(ValueError, match='refine'):
        P.ShootingController(None, grad_steps=1, refine='some', **kw)


def test_argument_errors():
    st = states_of(2)
    qs = QuadGrad(torch.zeros(2, 3, 2))
    a = torch.zeros(2, 4, 3, 2)
    with pytest.raises(ValueError, match='an engine or a grad_scorer'):
        P.refine_actions(None, st, a, 1, 0.1)
    with pytest.raises(ValueError, match='n_steps must not be negative'):
        P.refine_actions(None, st, a, -1, 0.1, grad_scorer=qs)
    with pytest.raises(ValueError, match='lr must be positive'):
        P.refine_actions(None, st, a, 1, 0.0, grad_scorer=qs)
    with pytest.raises(ValueError, match="optimizer: 'rmsprop'"):
        P.refine_actions(None, st, a, 1, 0.1, optimizer='rmsprop', grad_scorer=qs)
    with pytest.raises(ValueError, match=r'actions: expected \[2, N, T, 2\] or \[2, T, 2\]'):
        P.refine_actions(None, st, torch.zeros(3, 4, 3, 2), 1, 0.1, grad_scorer=qs)
    with pytest.raises(ValueError, match=r'states: expected \[S, 3\]'):
        P.refine_actions(None, torch.zeros(2, 2, NS), a, 1, 0.1, grad_scorer=qs)
    with pytest.raises(ValueError, match='an engine or a grad_scorer'):
        P.plan_cem_gd(None, st, 3, 8, 2, 1, grad_steps=1, na=2)
    with pytest.raises(ValueError, match='refine'):
        P.plan_cem_gd(None, st, 3, 8, 2, 1, grad_steps=1, refine='best', grad_scorer=qs, na=2)
    with pytest.raises(ValueError, match='n_elites must be in 1 ... n_candidates = 8'):
        P.plan_cem_gd(None, st, 3, 8, 9, 1, grad_steps=1, grad_scorer=qs, na=2)
    with pytest.raises(ValueError, match='na is needed'):
        P.plan_cem_gd(None, st, 3, 8, 2, 1, grad_steps=1, grad_scorer=qs)


def test_names_and_abi_without_a_gpu():
    from metrpo_amd import _lib
    for name in ('engine_grad_scorer', 'aggregate_heads_grad', 'refine_actions', 'plan_cem_gd'):
        assert name in metrpo_amd.__all__ and hasattr(metrpo_amd, name) and getattr(metrpo_amd, name) is getattr(P, name)
    assert hasattr(metrpo_amd.Engine, 'score_actions_grad') and hasattr(metrpo_amd.Engine, 'last_score_actions_grad_kernel')
    assert metrpo_amd.Engine.SCORE_ACTIONS_GRAD_OUTPUTS == ('grad', 'ret', 'len', 'grad_mean', 'lam0')
    lib = _lib.lib
    assert lib.metrpo_abi_version() == 4
    assert 'metrpo_score_actions_grad' in _lib.SYMBOLS and 'metrpo_last_score_actions_grad_kernel' in _lib.SYMBOLS
    assert lib.metrpo_score_actions_grad(None, C.byref(_lib.ScoreActionsGradArgs()), None) == -2      # METRPO_ENULL
    assert lib.metrpo_score_actions_grad(None, None, None) == -2
    assert lib.metrpo_last_score_actions_grad_kernel(None) == -2
    # the struct as the header lays it out (LP64): six int32, a double, seven pointers
    A = _lib.ScoreActionsGradArgs
    assert C.sizeof(A) == 6 * 4 + 8 + 7 * 8
    assert A.chunk.offset == 20 and A.gamma.offset == 24 and A.d_init_obs.offset == 32 and A.d_grad.offset == 48 and A.d_lam0.offset == 80
