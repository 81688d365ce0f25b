"""CPU checks of the noise-space planner of metrpo_amd.planning (plan_cem_policy, score_noise_sequences, ShootingController(policy_prior=True)) with
stand-in scorers and a stand-in policy (no GPU), and of the host-side declarations of metrpo_score_policy_actions.  The GPU side is
tests/test_gpu_score_policy.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrpo_amd
from metrpo_amd import _lib
from metrpo_amd import planning as P

NS, NA = 3, 2


def states_of(S):
    s = torch.zeros(S, NS)
    s[:, 0] = torch.arange(S, dtype=torch.float32)
    return s


def policy_stand_in(rows):
    """a 'policy mean' that depends on the state: [B, ns] -> [B, na]"""
    return torch.stack([0.3 * torch.cos(rows[:, 0]), -0.2 + 0.1 * rows[:, 0]], dim=1)


class NoiseRecorder(object):
    """A stand-in closed-loop scorer that keeps what it was shown: the candidate's action is policy_stand_in(start row) + noise (the state does not
    move), ret [K, B] = head offsets - sum (action - target)^2."""

    def __init__(self, target, K=1):
        self.target, self.K, self.calls = target, K, []                    # target [S, T, na]

    def __call__(self, noise, init):
        T, B, na = noise.shape
        S = init.shape[0]
        assert B % S == 0
        rows = init[torch.arange(B) // (B // S)]
        act = policy_stand_in(rows).unsqueeze(0) + noise
        tgt = self.target[rows[:, 0].long()].permute(1, 0, 2)
        ret = -((act - tgt) ** 2).sum(dim=(0, 2))
        self.calls.append((noise.clone(), ret.clone()))
        return torch.stack([ret + 0.25 * k for k in range(self.K)])


class EngineStandIn(object):
    """What ShootingController(policy_prior=True) needs of an engine besides the scorer: device, ns, na and policy_actions -> (actions, mean)"""
    device, ns, na = torch.device('cpu'), NS, NA

    def __init__(self):
        self.policy_calls = 0

    def policy_actions(self, obs, eps=None):
        self.policy_calls += 1
        m = policy_stand_in(torch.as_tensor(obs, dtype=torch.float32))
        return m, m


def test_one_iteration_is_the_numpy_restatement_and_delta_zero_rides_along():
    S, T, N, E, alpha, clip = 2, 4, 24, 5, 0.25, 0.9
    rng = np.random.RandomState(0)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, NA)), dtype=torch.float32)
    mean0 = rng.uniform(-0.5, 0.5, size=(S, T, NA)).astype(np.float32)
    rec = NoiseRecorder(target, K=3)
    out = P.plan_cem_policy(None, states_of(S), T, N, E, 1, init_mean=mean0, init_std=0.7, noise_clip=clip, alpha=alpha, min_std=0.05,
                            generator=torch.Generator().manual_seed(11), scorer=rec, na=NA)
    eps = torch.randn(T, S, N, NA, generator=torch.Generator().manual_seed(11), dtype=torch.float32).numpy()
    m0 = mean0.transpose(1, 0, 2)[:, :, None, :]                          # [T, S, 1, na]
    d = np.clip(m0 + np.float32(0.7) * eps, np.float32(-clip), np.float32(clip)).astype(np.float32)
    d[:, :, 0] = 0.0                                                      # include_policy: candidate 0 of every state is the policy itself
    assert len(rec.calls) == 1 and np.array_equal(rec.calls[0][0].numpy(), d.reshape(T, S * N, NA))
    assert (np.abs(d) == np.float32(clip)).any() and np.abs(d).max() <= np.float32(clip)     # noise_clip acted and is honoured
    scores = rec.calls[0][1].numpy().reshape(S, N) + np.float32(0.25)     # mean over the three heads' offsets 0, 0.25, 0.5
    for s in range(S):
        order = np.argsort(-scores[s], kind='stable')[:E]
        assert scores[s][order[E - 1]] > np.sort(scores[s])[::-1][E]      # no tie at the cut: the elite SET is defined
        el = d[:, s, order, :].astype(np.float64)                         # [T, E, na]: the CLAMPED noise, float64
        e_mean = (el.sum(axis=1) / E).astype(np.float32)
        e_std = np.sqrt(((el - el.sum(axis=1, keepdims=True) / E) ** 2).sum(axis=1) / E).astype(np.float32)
        want_mean = np.float32(alpha) * m0[:, s, 0] + np.float32(1 - alpha) * e_mean
        want_std = np.maximum(np.float32(alpha) * np.float32(0.7) + np.float32(1 - alpha) * e_std, np.float32(0.05))
        np.testing.assert_array_equal(out['noise'][s].numpy(), want_mean)
        np.testing.assert_array_equal(out['std'][s].numpy(), want_std)
        assert np.array_equal(out['elites'][s].numpy(), order)
        np.testing.assert_array_equal(out['best_noise'][s].numpy(), d[:, s, order[0], :])
        np.testing.assert_allclose(out['best_score'][s].item(), scores[s][order[0]], rtol=1e-6)
        np.testing.assert_allclose(out['policy_score'][s].item(), scores[s][0], rtol=1e-6)
    assert set(out) == {'noise', 'std', 'best_noise', 'best_score', 'history', 'elites', 'policy_score'}


def test_best_is_never_worse_than_the_policy_and_the_switch_removes_delta_zero():
    S, T, N, E = 3, 3, 8, 2
    # the target IS the policy's output: delta = 0 is the optimum, every drawn candidate is worse
    target = policy_stand_in(states_of(S)).unsqueeze(1).expand(S, T, NA).contiguous()
    rec = NoiseRecorder(target)
    out = P.plan_cem_policy(None, states_of(S), T, N, E, 3, init_std=0.5, generator=torch.Generator().manual_seed(3), scorer=rec, na=NA)
    assert len(rec.calls) == 3
    for noise, _ in rec.calls:
        assert torch.all(noise.reshape(T, S, N, NA)[:, :, 0] == 0) and torch.all(noise.reshape(T, S, N, NA)[:, :, 1:] != 0)
    assert torch.all(out['best_score'] >= out['policy_score']) and torch.equal(out['best_score'], out['policy_score'])
    assert torch.all(out['best_noise'] == 0) and torch.allclose(out['policy_score'], torch.zeros(S), atol=1e-12)
    assert torch.all(out['elites'][:, 0] == 0)
    rec2 = NoiseRecorder(target)
    off = P.plan_cem_policy(None, states_of(S), T, N, E, 2, init_std=0.5, generator=torch.Generator().manual_seed(3), scorer=rec2, na=NA, include_policy=False)
    assert off['policy_score'] is None and torch.all(rec2.calls[0][0] != 0) and torch.all(off['best_score'] < 0)
    # any target: the best candidate seen is at least the policy
    rng = np.random.RandomState(1)
    tgt = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, NA)), dtype=torch.float32)
    any_ = P.plan_cem_policy(None, states_of(S), T, 32, 4, 4, init_std=0.5, generator=torch.Generator().manual_seed(5), scorer=NoiseRecorder(tgt, K=2), na=NA)
    assert torch.all(any_['best_score'] >= any_['policy_score']) and torch.any(any_['best_score'] > any_['policy_score'])


def test_convergence_to_a_known_offset_from_the_policy():
    S, T = 2, 3
    offset = torch.tensor([0.35, -0.45])
    target = (policy_stand_in(states_of(S)) + offset).unsqueeze(1).expand(S, T, NA).contiguous()
    out = P.plan_cem_policy(None, states_of(S), T, 256, 24, 12, init_std=0.5, generator=torch.Generator().manual_seed(0), scorer=NoiseRecorder(target), na=NA)
    assert torch.allclose(out['noise'], offset.expand(S, T, NA), atol=0.02)
    assert torch.all(out['std'] < 0.05) and torch.all(out['history'][-1] > out['history'][0])
    sc = P.score_noise_sequences(None, states_of(S), out['noise'], scorer=NoiseRecorder(target))
    assert sc.shape == (S,) and torch.all(sc > -1e-2)
    many = P.score_noise_sequences(None, states_of(S), torch.zeros(S, 5, T, NA), scorer=NoiseRecorder(target, K=2), aggregate='min')
    assert many.shape == (S, 5) and torch.allclose(many, -(offset ** 2).sum() * T * torch.ones(S, 5))


def test_argument_errors():
    rec = NoiseRecorder(torch.zeros(1, 2, NA))
    with pytest.raises(ValueError, match='noise_clip'):
        P.plan_cem_policy(None, states_of(1), 2, 4, 2, 1, noise_clip=0.0, scorer=rec, na=NA)
    with pytest.raises(ValueError, match='n_elites'):
        P.plan_cem_policy(None, states_of(1), 2, 4, 5, 1, scorer=rec, na=NA)
    with pytest.raises(ValueError, match='an engine or a scorer'):
        P.plan_cem_policy(None, states_of(1), 2, 4, 2, 1, na=NA)
    with pytest.raises(ValueError, match='noise: expected'):
        P.score_noise_sequences(None, states_of(2), torch.zeros(3, 2, NA), scorer=rec)
    with pytest.raises(ValueError, match='grad_steps'):
        P.ShootingController(EngineStandIn(), 3, 8, 2, 1, scorer=rec, policy_prior=True, grad_steps=1)
    with pytest.raises(ValueError, match='needs an engine'):
        P.ShootingController(None, 3, 8, 2, 1, scorer=rec, na=NA, policy_prior=True)


def test_controller_shifts_the_noise_and_returns_the_clipped_policy_action():
    S, T = 2, 4
    offset = torch.tensor([0.9, -0.95])                                   # policy mean + offset leaves [-1, 1] in some entries: the clip acts
    target = (policy_stand_in(states_of(S)) + offset).unsqueeze(1).expand(S, T, NA).contiguous()
    eng = EngineStandIn()
    ctl = P.ShootingController(eng, T, 64, 8, 4, init_std=0.5, generator=torch.Generator().manual_seed(2), scorer=NoiseRecorder(target), policy_prior=True,
                               noise_clip=1.5)
    a, info = ctl.get_actions(states_of(S).numpy())
    assert info == {} and a.dtype == np.float64 and a.shape == (S, NA) and eng.policy_calls == 1
    plan = ctl.last_plan
    want = torch.clamp(policy_stand_in(states_of(S)) + plan['noise'][:, 0], -1.0, 1.0)
    np.testing.assert_array_equal(a, want.double().numpy())
    assert plan['noise'].abs().max() <= 1.5
    assert torch.equal(ctl._mean[:, :-1], plan['noise'][:, 1:]) and torch.all(ctl._mean[:, -1] == 0)      # shifted, the last row reset to 0
    sh = ctl.shifted_noise(torch.arange(S * T * NA, dtype=torch.float32).reshape(S, T, NA) + 1.0)
    assert torch.all(sh[:, -1] == 0) and sh[0, 0, 0] == 1.0 + NA
    rec = NoiseRecorder(target)
    ctl.scorer = rec
    ctl.get_actions(states_of(S).numpy())                                 # the warm start: the first iteration's draws centre on the shifted mean
    first = rec.calls[0][0].reshape(T, S, 64, NA)[:, :, 1:].mean(dim=2).permute(1, 0, 2)
    assert torch.allclose(first[:, :-1], plan['noise'][:, 1:], atol=0.25)
    ctl.reset()
    assert ctl._mean is None


def test_default_controller_plans_exactly_as_before():
    """Without the new keywords the controller is plan_cem with a warm start, bit for bit, for a seeded generator."""
    S, T, na = 2, 4, 2
    rng = np.random.RandomState(4)
    target = torch.as_tensor(rng.uniform(-0.8, 0.8, size=(S, T, na)), dtype=torch.float32)

    def scorer(actions, init):
        B = actions.shape[1]
        rows = init[torch.arange(B) // (B // init.shape[0])]
        return -((actions - target[rows[:, 0].long()].permute(1, 0, 2)) ** 2).sum(dim=(0, 2)).unsqueeze(0)

    ctl = P.ShootingController(None, T, 32, 4, 3, init_std=0.8, generator=torch.Generator().manual_seed(9), scorer=scorer, na=na)
    assert ctl.policy_prior is False
    a1, _ = ctl.get_actions(states_of(S).numpy())
    a2, _ = ctl.get_actions(states_of(S).numpy())
    gen = torch.Generator().manual_seed(9)
    p1 = P.plan_cem(None, states_of(S), T, 32, 4, 3, init_std=0.8, generator=gen, scorer=scorer, na=na)
    p2 = P.plan_cem(None, states_of(S), T, 32, 4, 3, init_mean=torch.cat([p1['actions'][:, 1:], torch.zeros(S, 1, na)], dim=1), init_std=0.8, generator=gen,
                    scorer=scorer, na=na)
    np.testing.assert_array_equal(a1, p1['actions'][:, 0].double().numpy())
    np.testing.assert_array_equal(a2, p2['actions'][:, 0].double().numpy())
    for k in p2:
        assert torch.equal(ctl.last_plan[k], p2[k]), k


def test_declarations():
    for name in ('engine_policy_scorer', 'score_noise_sequences', 'plan_cem_policy'):
        assert name in metrpo_amd.__all__ and getattr(metrpo_amd, name) is getattr(P, name)
    assert C.sizeof(_lib.ScorePolicyActionsArgs) == 6 * 4 + 8 + 7 * 8
    assert _lib.lib.metrpo_abi_version() == 4
    assert 'metrpo_score_policy_actions' in _lib.SYMBOLS and 'metrpo_last_score_policy_actions_kernel' in _lib.SYMBOLS
    assert _lib.lib.metrpo_last_score_policy_actions_kernel(None) == -2                 # METRPO_ENULL: the symbol is exported and bound
    assert metrpo_amd.Engine.SCORE_POLICY_ACTIONS_OUTPUTS == ('ret', 'len', 'ret_mean', 'ret_std', 'act_out')
    sc = P.engine_policy_scorer(None, gamma=0.9, stop_at_done=False, noise_in_std=True, force_generic=True)
    assert callable(sc)
