"""CPU checks of the gradient side of the noise-space planner of metrpo_amd.planning (refine_noise, plan_cem_policy_gd,
ShootingController(policy_prior=True, noise_grad_steps=n)) with stand-in scorers and a stand-in policy (no GPU), and of the host-side declarations of
metrpo_score_policy_actions_grad.  The GPU side is tests/test_gpu_score_policy_grad.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrpo_amd
from metrpo_amd import _lib
from metrpo_amd import planning as P
from test_planning_policy_host import NS, NA, states_of, policy_stand_in, NoiseRecorder, EngineStandIn


class NoiseGrad(object):
    """NoiseRecorder with its gradient: ret [K, B] = head offsets - sum (policy + noise - target)^2, grad [K, T, B, na] = -2 (policy + noise - target)"""

    def __init__(self, target, K=1):
        self.target, self.K, self.calls = target, K, []

    def __call__(self, noise, init):
        T, B, na = noise.shape
        S = init.shape[0]
        rows = init[torch.arange(B) // (B // S)]
        diff = policy_stand_in(rows).unsqueeze(0) + noise - self.target[rows[:, 0].long()].permute(1, 0, 2)
        ret = -(diff ** 2).sum(dim=(0, 2))
        self.calls.append(noise.clone())
        return torch.stack([ret + 0.25 * k for k in range(self.K)]), torch.stack([-2.0 * diff] * self.K)


def target_of(S, T, seed=0, lo=-0.8, hi=0.8):
    return torch.as_tensor(np.random.RandomState(seed).uniform(lo, hi, size=(S, T, NA)), dtype=torch.float32)


def test_refine_noise_is_projected_ascent_that_keeps_the_best_iterate():
    S, N, T, clip, lr = 2, 3, 4, 0.6, 0.1
    target = target_of(S, T, 1, -1.5, 1.5)                                # some optima lie beyond noise_clip of the policy: the projection acts
    gs = NoiseGrad(target, K=2)
    nz = torch.as_tensor(np.random.RandomState(2).uniform(-0.5, 0.5, size=(S, N, T, NA)), dtype=torch.float32)
    out = P.refine_noise(None, states_of(S), nz, 1, lr, noise_clip=clip, optimizer='sgd', grad_scorer=gs)
    assert len(gs.calls) == 2 and torch.equal(gs.calls[0], P._device_major(nz))
    ret, grad = NoiseGrad(target, K=2)(P._device_major(nz), states_of(S))
    want = torch.clamp(P._device_major(nz) + lr * grad.mean(dim=0), -clip, clip)
    assert torch.equal(P._device_major(out['last']), want) and torch.equal(gs.calls[1], want)
    assert torch.equal(out['initial_score'].reshape(-1), ret.mean(dim=0))
    assert set(out) == {'noise', 'score', 'last', 'last_score', 'initial_score'}
    many = P.refine_noise(None, states_of(S), nz, 40, lr, noise_clip=clip, optimizer='sgd', grad_scorer=NoiseGrad(target))
    assert many['last'].abs().max() <= clip and bool((many['last'].abs() == clip).any())            # projected onto +-noise_clip, and it acted
    assert torch.all(many['score'] >= many['initial_score']) and torch.all(many['score'] >= many['last_score'])
    # keep-best: a step far too long makes every later iterate worse; the input comes back
    bad = P.refine_noise(None, states_of(S), nz, 3, 50.0, noise_clip=5.0, optimizer='sgd', grad_scorer=NoiseGrad(target))
    assert torch.equal(bad['noise'], nz) and torch.equal(bad['score'], bad['initial_score']) and torch.all(bad['last_score'] < bad['score'])
    # Adam, one candidate per state, n_steps = 0
    one = P.refine_noise(None, states_of(S), nz[:, 0], 5, 0.05, grad_scorer=NoiseGrad(target))
    assert one['noise'].shape == (S, T, NA) and one['score'].shape == (S,) and torch.all(one['score'] > one['initial_score'])
    zero = P.refine_noise(None, states_of(S), nz, 0, 0.05, grad_scorer=NoiseGrad(target))
    assert torch.equal(zero['noise'], nz) and torch.equal(zero['last'], nz)


def test_refine_actions_still_projects_onto_the_unit_box():
    """_refine's projection became a parameter: refine_actions' default is clamp(-1, 1), as before"""
    S, N, T = 1, 2, 3
    gs = NoiseGrad(target_of(S, T, 3, 2.0, 3.0))                          # pulls every entry beyond +1 (the stand-in's signature fits grad_scorer=)
    out = P.refine_actions(None, states_of(S), torch.zeros(S, N, T, NA), 60, 0.2, optimizer='sgd', grad_scorer=gs)
    assert out['last'].max() == 1.0 and out['last'].abs().max() <= 1.0


@pytest.mark.parametrize('include_policy', [True, False])
def test_plan_cem_policy_gd_without_steps_is_plan_cem_policy_bit_for_bit(include_policy):
    S, T, N, E = 2, 4, 24, 5
    target = target_of(S, T, 4)
    kw = dict(init_std=0.7, noise_clip=0.9, alpha=0.25, min_std=0.05, na=NA, include_policy=include_policy)
    a = P.plan_cem_policy(None, states_of(S), T, N, E, 3, generator=torch.Generator().manual_seed(11), scorer=NoiseRecorder(target, K=3), **kw)
    for refine in ('elites', 'all'):
        b = P.plan_cem_policy_gd(None, states_of(S), T, N, E, 3, 0, refine=refine, generator=torch.Generator().manual_seed(11),
                                 scorer=NoiseRecorder(target, K=3), **kw)
        assert set(a) == set(b)
        for k in a:
            assert (a[k] is None and b[k] is None) if a[k] is None else torch.equal(a[k], b[k]), k
    # ... and with the gradient scorer alone (no scorer, no engine) its returns are the scores
    c = P.plan_cem_policy_gd(None, states_of(S), T, N, E, 3, 0, generator=torch.Generator().manual_seed(11), grad_scorer=NoiseGrad(target, K=3), **kw)
    for k in a:
        assert (a[k] is None and c[k] is None) if a[k] is None else torch.equal(a[k], c[k]), k


@pytest.mark.parametrize('refine', ['elites', 'all'])
def test_plan_cem_policy_gd_refines_before_the_refit_and_never_falls_below_the_policy(refine):
    S, T, N, E = 2, 3, 16, 4
    target = target_of(S, T, 5)
    gs, rec = NoiseGrad(target), NoiseRecorder(target)
    kw = dict(init_std=0.5, na=NA, generator=torch.Generator().manual_seed(7))
    out = P.plan_cem_policy_gd(None, states_of(S), T, N, E, 2, 3, grad_lr=0.1, refine=refine, optimizer='sgd', scorer=rec, grad_scorer=gs, **kw)
    plain = P.plan_cem_policy(None, states_of(S), T, N, E, 2, scorer=NoiseRecorder(target), init_std=0.5, na=NA, generator=torch.Generator().manual_seed(7))
    if refine == 'elites':                                                 # per iteration: one scoring call of S N candidates, 3 + 1 gradient calls of S E
        assert len(rec.calls) == 2 and len(gs.calls) == 8 and all(c.shape[1] == S * E for c in gs.calls)
        assert torch.all(rec.calls[0][0].reshape(T, S, N, NA)[:, :, 0] == 0)                        # delta = 0 is planted
    else:
        assert len(rec.calls) == 0 and len(gs.calls) == 8 and all(c.shape[1] == S * N for c in gs.calls)
        assert torch.all(gs.calls[0].reshape(T, S, N, NA)[:, :, 0] == 0)
    assert torch.equal(out['policy_score'], plain['policy_score'])          # the score of delta = 0 itself
    assert torch.all(out['best_score'] >= out['policy_score'])
    assert torch.all(out['history'][0] > plain['history'][0])               # the refined elites of the first iteration beat the drawn ones
    assert torch.all(out['best_score'] > plain['best_score'])


def test_argument_errors():
    rec, gs = NoiseRecorder(torch.zeros(1, 2, NA)), NoiseGrad(torch.zeros(1, 2, NA))
    nz = torch.zeros(1, 2, 2, NA)
    with pytest.raises(ValueError, match='noise_clip'):
        P.refine_noise(None, states_of(1), nz, 1, 0.1, noise_clip=0.0, grad_scorer=gs)
    with pytest.raises(ValueError, match='n_steps'):
        P.refine_noise(None, states_of(1), nz, -1, 0.1, grad_scorer=gs)
    with pytest.raises(ValueError, match='lr'):
        P.refine_noise(None, states_of(1), nz, 1, 0.0, grad_scorer=gs)
    with pytest.raises(ValueError, match='optimizer'):
        P.refine_noise(None, states_of(1), nz, 1, 0.1, optimizer='lbfgs', grad_scorer=gs)
    with pytest.raises(ValueError, match='an engine or a grad_scorer'):
        P.refine_noise(None, states_of(1), nz, 1, 0.1)
    with pytest.raises(ValueError, match='noise: expected'):
        P.refine_noise(None, states_of(2), torch.zeros(3, 2, NA), 1, 0.1, grad_scorer=gs)
    with pytest.raises(ValueError, match='refine'):
        P.plan_cem_policy_gd(None, states_of(1), 2, 4, 2, 1, 1, refine='some', scorer=rec, grad_scorer=gs, na=NA)
    with pytest.raises(ValueError, match='n_elites'):
        P.plan_cem_policy_gd(None, states_of(1), 2, 4, 5, 1, 1, scorer=rec, grad_scorer=gs, na=NA)
    with pytest.raises(ValueError, match='noise_clip'):
        P.plan_cem_policy_gd(None, states_of(1), 2, 4, 2, 1, 1, noise_clip=float('inf'), scorer=rec, grad_scorer=gs, na=NA)
    with pytest.raises(ValueError, match='n_steps'):
        P.plan_cem_policy_gd(None, states_of(1), 2, 4, 2, 1, -1, scorer=rec, grad_scorer=gs, na=NA)
    with pytest.raises(ValueError, match='an engine or a grad_scorer'):
        P.plan_cem_policy_gd(None, states_of(1), 2, 4, 2, 1, 1, scorer=rec, na=NA)


def test_controller_keyword_and_the_old_refusal():
    S, T = 2, 4
    target = (policy_stand_in(states_of(S)) + torch.tensor([0.4, -0.3])).unsqueeze(1).expand(S, T, NA).contiguous()
    # the old refusal stands exactly as it was: gradients with respect to open-loop actions do not combine with the policy prior
    with pytest.raises(ValueError, match='grad_steps > 0 .gradients with respect to open-loop actions. cannot be combined with it'):
        P.ShootingController(EngineStandIn(), T, 8, 2, 1, scorer=NoiseRecorder(target), policy_prior=True, grad_steps=1)
    with pytest.raises(ValueError, match='noise_grad_steps > 0 .* needs policy_prior=True'):
        P.ShootingController(None, T, 8, 2, 1, scorer=NoiseRecorder(target), na=NA, noise_grad_steps=1)
    with pytest.raises(ValueError, match='n_steps'):
        P.ShootingController(EngineStandIn(), T, 8, 2, 1, scorer=NoiseRecorder(target), policy_prior=True, noise_grad_steps=-1)
    eng, gs = EngineStandIn(), NoiseGrad(target)
    ctl = P.ShootingController(eng, T, 32, 4, 2, init_std=0.5, generator=torch.Generator().manual_seed(2), scorer=NoiseRecorder(target), policy_prior=True,
                               noise_clip=1.5, noise_grad_steps=2, noise_grad_lr=0.1, noise_grad_scorer=gs)
    assert ctl.noise_grad_steps == 2 and ctl.grad_steps == 0
    a, info = ctl.get_actions(states_of(S).numpy())
    assert info == {} and a.shape == (S, NA) and a.dtype == np.float64 and eng.policy_calls == 1
    assert len(gs.calls) == 2 * 3                                           # plan_cem_policy_gd ran: per iteration 2 + 1 gradient calls on the elites
    gen = torch.Generator().manual_seed(2)
    want = P.plan_cem_policy_gd(None, states_of(S), T, 32, 4, 2, 2, grad_lr=0.1, init_std=0.5, noise_clip=1.5, generator=gen, scorer=NoiseRecorder(target),
                                grad_scorer=NoiseGrad(target), na=NA)
    for k in want:
        assert torch.equal(ctl.last_plan[k], want[k]), k
    np.testing.assert_array_equal(a, torch.clamp(policy_stand_in(states_of(S)) + want['noise'][:, 0], -1.0, 1.0).double().numpy())
    assert torch.equal(ctl._mean[:, :-1], want['noise'][:, 1:]) and torch.all(ctl._mean[:, -1] == 0)
    # the default (noise_grad_steps = 0) plans with plan_cem_policy as before
    ctl0 = P.ShootingController(EngineStandIn(), T, 32, 4, 2, init_std=0.5, generator=torch.Generator().manual_seed(2), scorer=NoiseRecorder(target),
                                policy_prior=True, noise_clip=1.5)
    ctl0.get_actions(states_of(S).numpy())
    plain = P.plan_cem_policy(None, states_of(S), T, 32, 4, 2, init_std=0.5, noise_clip=1.5, generator=torch.Generator().manual_seed(2),
                              scorer=NoiseRecorder(target), na=NA)
    for k in plain:
        assert torch.equal(ctl0.last_plan[k], plain[k]), k


def test_declarations():
    for name in ('engine_policy_grad_scorer', 'refine_noise', 'plan_cem_policy_gd'):
        assert name in metrpo_amd.__all__ and getattr(metrpo_amd, name) is getattr(P, name)
    assert C.sizeof(_lib.ScorePolicyActionsGradArgs) == 7 * 4 + 4 + 8 + 8 * 8         # seven int32, padding, gamma, eight pointers
    assert _lib.lib.metrpo_abi_version() == 4
    assert 'metrpo_score_policy_actions_grad' in _lib.SYMBOLS and 'metrpo_last_score_policy_actions_grad_kernel' in _lib.SYMBOLS
    assert _lib.lib.metrpo_last_score_policy_actions_grad_kernel(None) == -2             # METRPO_ENULL: the symbol is exported and bound
    assert _lib.lib.metrpo_score_policy_actions_grad(None, None, None) == -2
    assert metrpo_amd.Engine.SCORE_POLICY_ACTIONS_GRAD_OUTPUTS == ('grad', 'ret', 'len', 'grad_mean', 'lam0', 'act_out')
    assert callable(P.engine_policy_grad_scorer(None, gamma=0.9, stop_at_done=False, noise_in_std=True, force_generic=True))
