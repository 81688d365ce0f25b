"""PPO's KL penalty on the GPU (metrpo_ppo_kl_loss_grad / metrpo_ppo_kl_update: the OP_PPOKL instantiations of the update kernels in
csrc/policy_update.hip, policy_mfma.hip, policy_fused3.hip and policy_gemm.hip behind the OP_LOSSKL launch that leaves the mean KL on the device)
against the float64 restatement tests/ppo_kl_ref.py, on every update family of test_gpu_vpg.FAMILIES at their N; the data are test_gpu_ppo.case()'s
(near-bound samples removed, CAP = 1 %).  Tolerances: tests/tolerances.py.

The penalty's gate is discontinuous in the mean KL.  Every case keeps the float64 mean KL a factor 2 (gradient cases) or at least 10 % (epoch
cases) away from step_size -- far above the fp32 error of the device's KL -- so both sides take the same branch; the builders assert it on the CPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import tolerances as TOL
import ppo_ref as R
import ppo_kl_ref as K
import test_gpu_ppo as T
from test_gpu_ppo import cpu, rel_l2, engine_for, _adam_state, _state, BAND, CAP
from test_gpu_vpg import FAMILIES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CASES = {}


def _args(cs):
    return cs['pdims'], cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls']


def kl_case(family):
    """test_gpu_ppo.case(family) (theta moved off theta_old) plus the reference's mean KL there and a kl_penalty under which the KL part of the
    reference gradient has at least the norm of the surrogate part, so that a missing KL seed cannot hide.  Computed once per family."""
    if family not in _CASES:
        cs = T.case(family)
        _, _, info = K.loss_grad(cs['theta'], *_args(cs), cs['clip'], 0.0, 1.0, 0.0, cs['valid'])
        assert info['open'] and info['mean_kl'] > 1e-4, info['mean_kl']
        n_ppo, n_kl = np.linalg.norm(info['g_ppo']), np.linalg.norm(info['g_kl'])
        beta = float(np.float32(max(1.0, 2.0 * n_ppo / n_kl)))       # (a float32: the kernels take it as one)
        assert beta * n_kl >= n_ppo, (family, beta, n_kl, n_ppo)
        cs.update(mean_kl=info['mean_kl'], beta=beta, kl_share=beta * n_kl / n_ppo)
        _CASES[family] = cs
    return _CASES[family]


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_ppo_kl_loss_grad_matches_reference_gate_open_and_closed(family):
    """1: step_size = 0.5 x and 2 x the reference's mean KL.  Open: loss and gradient against the restatement.  Closed: ppo_loss_grad's bits."""
    cs = kl_case(family)
    eng, b = engine_for(cs)
    for ent in (0.0, 0.02):
        plain = cpu(eng.ppo_loss_grad(b, cs['clip'], ent))
        for step, want_open in ((0.5 * cs['mean_kl'], True), (2.0 * cs['mean_kl'], False)):
            loss, g, info = K.loss_grad(cs['theta'], *_args(cs), cs['clip'], ent, cs['beta'], step, cs['valid'])
            assert info['open'] is want_open
            out = cpu(eng.ppo_kl_loss_grad(b, cs['clip'], ent, cs['beta'], step))
            assert eng.last_update_launch()['op'] == 6           # OP_PPOKL, on the family the case names (engine_for asserts update_path)
            print('ppo_kl parity %s ent=%g open=%d: beta %.3g (|beta g_kl| / |g_ppo| = %.2f) mean_kl %.4g loss err %.3g grad rel_l2 %.3g' % (
                family, ent, want_open, cs['beta'], cs['kl_share'], cs['mean_kl'], abs(out[0] - loss) / max(1.0, abs(loss)), rel_l2(out[1:], g)))
            assert abs(out[0] - loss) <= TOL.LOSS_RTOL * max(1.0, abs(loss)), (out[0], loss)
            assert rel_l2(out[1:], g) <= TOL.GRAD_REL_L2, rel_l2(out[1:], g)
            if want_open:
                assert rel_l2(out[1:], plain[1:]) > 0.5           # the seed is there (kl_case: the KL part is at least the surrogate part)
            else:
                assert np.array_equal(out, plain)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_clamped_log_std_slot_has_exactly_zero_gradient_with_the_gate_open(family):
    """2: one log_std below log(1e-6), entropy coefficient and penalty on, step_size = 0 (any positive mean KL opens the gate): that slot's
    gradient is exactly 0.0 -- no surrogate, entropy or KL share.  (Nothing else is asserted: ratios are meaningless at std = 1e-6.)"""
    cs = dict(T.case(family, moved=False))
    na = cs['pdims'][-1]
    cs['theta'] = cs['theta'].copy(); cs['theta'][-na] = -20.0
    eng, b = engine_for(cs)
    lk = cpu(eng.loss_kl(b))
    assert lk[1] > 0.0                                          # the gate IS open
    out = cpu(eng.ppo_kl_loss_grad(b, 0.2, 0.05, 3.0, 0.0))
    assert out[-na] == 0.0
    assert np.all(out[-na + 1:] != 0.0) if na > 1 else True


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_mean_kl_none_is_the_devices_own_loss_kl(family):
    """3: mean_kl=None computes what loss_kl returns: the same bits as passing loss_kl(batch)[1:2]."""
    cs = kl_case(family)
    eng, b = engine_for(cs)
    for step in (0.5 * cs['mean_kl'], 2.0 * cs['mean_kl']):
        lk = eng.loss_kl(b)
        given = cpu(eng.ppo_kl_loss_grad(b, cs['clip'], 0.02, cs['beta'], step, mean_kl=lk[1:2]))
        own = cpu(eng.ppo_kl_loss_grad(b, cs['clip'], 0.02, cs['beta'], step))
        assert np.array_equal(given, own)
    # ... and the gate follows the value that is passed, not the batch: a mean KL of 0 closes it, a huge one opens it
    plain = cpu(eng.ppo_loss_grad(b, cs['clip'], 0.02))
    zero = torch.zeros(1, dtype=torch.float64, device=eng.device)
    assert np.array_equal(cpu(eng.ppo_kl_loss_grad(b, cs['clip'], 0.02, cs['beta'], 0.5 * cs['mean_kl'], mean_kl=zero)), plain)
    assert not np.array_equal(cpu(eng.ppo_kl_loss_grad(b, cs['clip'], 0.02, cs['beta'], 2.0 * cs['mean_kl'], mean_kl=zero + 1e3)), plain)
    tie = torch.full((1,), 0.25, dtype=torch.float64, device=eng.device)       # MaximumGrad: a tie goes to the constant
    assert np.array_equal(cpu(eng.ppo_kl_loss_grad(b, cs['clip'], 0.02, cs['beta'], 0.25, mean_kl=tie)), plain)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_fused_epochs_are_bitwise_the_call_by_call_form(family):
    """4: ppo_kl_update(n_epochs=n) is n x (loss_kl, ppo_kl_loss_grad with that mean KL, policy_adam_step(clip_val=None)) bit for bit in theta, m, v,
    t, the losses and the mean KLs, n = 1 and 4, with the gate open at entry."""
    cs = kl_case(family)
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 1)
    ent, step = 0.02, 0.5 * cs['mean_kl']
    for n in (1, 4):
        eng.set_policy(cs['theta']); eng.set_policy_adam(m0, v0, t0)
        by_losses, by_kls = [], []
        for _ in range(n):
            lk = eng.loss_kl(b)
            lg = eng.ppo_kl_loss_grad(b, cs['clip'], ent, cs['beta'], step, mean_kl=lk[1:2])
            by_losses.append(cpu(lg)[0]); by_kls.append(cpu(lk)[1])
            eng.policy_adam_step(lg[1:], 1e-2, clip_val=None)
        by = _state(eng)
        eng.set_policy(cs['theta']); eng.set_policy_adam(m0, v0, t0)
        losses, kls = eng.ppo_kl_update(b, n_epochs=n, clip_lr=cs['clip'], entropy_bonus_coeff=ent, kl_penalty=cs['beta'], step_size=step, lr=1e-2,
                                        want_mean_kls=True)
        one = _state(eng)
        assert one[3] == by[3] == t0 + n
        for a, c in zip(one[:3], by[:3]):
            assert np.array_equal(a, c)
        assert losses.shape == kls.shape == (n,)
        assert np.array_equal(cpu(losses), np.array(by_losses)) and np.array_equal(cpu(kls), np.array(by_kls))
        assert by_kls[0] > step and not np.array_equal(one[0], cs['theta'])
    assert eng.ppo_kl_update(b, n_epochs=0, want_losses=True).shape == (0,) and _state(eng)[3] == t0 + 4


def epoch_case(family, lr=1e-2, ent=0.02):
    """Four epochs from theta = theta_old (mean KL 0: the gate is closed at epoch 0), on the CPU alone: step_size is put between the mean KLs of two
    successive epochs of the unpenalised reference run, kl_penalty makes the KL part the size of the surrogate part where the gate first opens.
    Asserted on the penalised reference run: closed at epoch 0, open at a later epoch, every epoch's mean KL at least 10 % away from step_size."""
    key = ('epochs', family)
    if key not in _CASES:
        cs = dict(T.case(family, moved=False))
        m0, v0, t0 = _adam_state(len(cs['theta']), 2)
        free = K.adam_epochs(cs['theta'], m0.astype(np.float64), v0.astype(np.float64), t0, *_args(cs), cs['clip'], ent, 0.0, 0.0, cs['valid'],
                             n_epochs=3, lr=lr)
        k1, k2 = free[5][1], free[5][2]
        assert free[5][0] < 1e-9 and k2 > 1.5 * k1 > 0.0, free[5]        # (old_mean is theta_old's mean rounded to float32: not exactly 0)
        step = float(np.sqrt(k1 * k2))
        th, m, v, t = cs['theta'], m0.astype(np.float64), v0.astype(np.float64), t0
        for _ in range(2):
            th, m, v, t = K.adam_epochs(th, m, v, t, *_args(cs), cs['clip'], ent, 0.0, step, cs['valid'], n_epochs=1, lr=lr)[:4]
        info = K.loss_grad(th, *_args(cs), cs['clip'], ent, 1.0, step, cs['valid'])[2]
        beta = float(np.float32(max(1.0, np.linalg.norm(info['g_ppo']) / np.linalg.norm(info['g_kl']))))
        kls = K.adam_epochs(cs['theta'], m0.astype(np.float64), v0.astype(np.float64), t0, *_args(cs), cs['clip'], ent, beta, step, cs['valid'],
                            n_epochs=4, lr=lr)[5]
        opened = kls - step > 0.0
        assert not opened[0] and opened[1:].any(), (kls, step)
        assert np.all(np.abs(kls - step) >= 0.1 * step), (kls, step)
        cs.update(step=step, beta=beta, lr=lr, ent=ent, ref_kls=kls)
        _CASES[key] = cs
    return _CASES[key]


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_four_epochs_track_the_reference_across_the_gate(family):
    """5: four epochs from theta_old against ppo_kl_ref.adam_epochs in the form of test_gpu_ppo.test_four_epochs_track_the_reference: every epoch's
    reference step starts from the DEVICE's own state, single-epoch calls (the near-bound samples are taken out at each epoch's theta), its bounds
    (loss within LOSS_RTOL, moments rel-L2 <= 1e-4, theta step rel-L2 <= 1e-3), and the mean KL entering the epoch within LOSS_RTOL.  The gate is
    closed at epoch 0 and open at a later one (epoch_case, and asserted again on the states the device went through).
    Observed on an MI355X, worst of the four epochs (loss error / max(1, |loss|), mean KL error / max(1, |mean KL|), rel-L2 of m, of v and of the
    theta step; bounds LOSS_RTOL, LOSS_RTOL, 1e-4, 1e-4, 1e-3): fused3 loss 3.33e-07, kl 2.35e-07, m 9.37e-07, v 2.44e-06, theta step 5.53e-06 (gates
    closed, closed, open, open); gemm loss 1.61e-08, kl 4.48e-08, m 4.14e-07, v 3.98e-07, theta step 8.75e-06 (closed, closed, open, open); generic loss
    1.14e-07, kl 4.36e-08, m 5.75e-07, v 9.91e-07, theta step 9.12e-06 (closed, closed, open, closed); mfma loss 1.19e-07, kl 4.43e-08, m 5.17e-07,
    v 1.01e-06, theta step 9.11e-06 (closed, closed, open, closed)."""
    cs = epoch_case(family)
    ent, lr, step, beta = cs['ent'], cs['lr'], cs['step'], cs['beta']
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 2)
    eng.set_policy_adam(m0, v0, t0)
    base = np.ones(cs['N'], np.uint8); base[::7] = 0; base[5] = 0
    worst, gates = np.zeros(5), []
    for k in range(4):
        prev = _state(eng)
        ratio = R.ratios(prev[0], cs['pdims'], cs['obs'], cs['act'], cs['old_mean'], cs['old_ls'])[0]
        valid = base.copy()
        valid[T.near_bound(ratio, cs['clip'])] = 0
        assert base.sum() - valid.sum() <= CAP * cs['N']
        bk = eng.make_batch(cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls'][0], valid=valid)
        loss, kl = eng.ppo_kl_update(bk, n_epochs=1, clip_lr=cs['clip'], entropy_bonus_coeff=ent, kl_penalty=beta, step_size=step, lr=lr, want_mean_kls=True)
        loss, kl = cpu(loss), cpu(kl)
        cur = _state(eng)
        th_r, m_r, v_r, t_r, l_r, k_r = K.adam_epochs(prev[0], prev[1], prev[2], prev[3], *_args(cs), cs['clip'], ent, beta, step, valid, n_epochs=1, lr=lr)
        assert abs(k_r[0] - step) >= 0.1 * step, (k, k_r[0], step)          # both sides take the same branch
        gates.append(k_r[0] - step > 0.0)
        figs = np.array([abs(loss[0] - l_r[0]) / max(1.0, abs(l_r[0])), abs(kl[0] - k_r[0]) / max(1.0, abs(k_r[0])), rel_l2(cur[1], m_r), rel_l2(cur[2], v_r),
                         rel_l2(cur[0] - prev[0], th_r - prev[0])])
        worst = np.maximum(worst, figs)
        print('ppo_kl epoch %d %s: gate %d mean_kl %.4g step_size %.4g beta %.3g  loss %.3g  kl %.3g  m %.3g  v %.3g  theta step %.3g' % (
            (k, family, gates[-1], k_r[0], step, beta) + tuple(figs)))
        assert cur[3] == t_r == t0 + k + 1
        assert figs[0] <= TOL.LOSS_RTOL and figs[1] <= TOL.LOSS_RTOL, figs
        assert figs[2] <= 1e-4 and figs[3] <= 1e-4, figs
        assert figs[4] <= 1e-3, figs
    assert not gates[0] and any(gates[1:]), gates
    print('ppo_kl 4 epochs %s worst: loss %.3g  kl %.3g  m %.3g  v %.3g  theta step %.3g  gates %s' % ((family,) + tuple(worst) + (gates,)))


def test_no_host_wait_between_the_epochs():
    """6: the call only enqueues (the method of test_gpu_ppo.test_no_host_wait_between_the_epochs): a spin kernel keeps the stream busy in front of
    it; metrpo_ppo_kl_update with four epochs returns while the event recorded behind the spin kernel has not fired."""
    cs = kl_case('mfma')
    eng, b = engine_for(cs)
    dev = eng.device
    kw = dict(clip_lr=cs['clip'], kl_penalty=cs['beta'], step_size=0.5 * cs['mean_kl'])
    eng.ppo_kl_update(b, n_epochs=4, **kw)                        # workspaces, the Adam state and the four mean-KL pairs exist
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); torch.cuda._sleep(20000000); e1.record(); torch.cuda.synchronize()
    cycles = int(20000000 * 400.0 / max(e0.elapsed_time(e1), 1e-3))
    side = torch.cuda.Stream(device=dev)
    front = torch.cuda.Event()
    t_before = eng.get_policy_adam()[2]
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        front.record(side)
        losses, kls = eng.ppo_kl_update(b, n_epochs=4, entropy_bonus_coeff=0.01, want_mean_kls=True, **kw)
        still_busy = not front.query()
    torch.cuda.synchronize()
    assert still_busy, "ppo_kl_update waited for the device: the event in front of it had fired when it returned"
    assert eng.get_policy_adam()[2] == t_before + 4 and np.all(np.isfinite(cpu(losses))) and np.all(cpu(kls) > 0.0)


def test_bad_arguments():
    """7: the stated codes."""
    from metrpo_amd import _lib
    lib = _lib.lib
    cs = kl_case('mfma')
    eng, b = engine_for(cs)
    out = torch.empty(eng.P + 1, dtype=torch.float64, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    par, kp = _lib.PpoParams(0.3, 0.0, 1e-3, 0.9, 0.999, 1e-8), _lib.PpoKlParams(1.0, 0.01)
    st = eng._stream()
    assert lib.metrpo_ppo_kl_loss_grad(eng._ctx, C.byref(b), C.byref(par), C.byref(kp), None, None, st) == -2          # METRPO_ENULL
    assert lib.metrpo_ppo_kl_loss_grad(eng._ctx, C.byref(b), None, C.byref(kp), None, p(out), st) == -2
    assert lib.metrpo_ppo_kl_loss_grad(eng._ctx, C.byref(b), C.byref(par), None, None, p(out), st) == -2
    assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(b), C.byref(par), None, 1, None, None, st) == -2
    nb = eng.make_batch(cs['obs'], cs['act'], cs['adv'], None, None)                                                   # no old distribution
    assert lib.metrpo_ppo_kl_loss_grad(eng._ctx, C.byref(nb), C.byref(par), C.byref(kp), None, p(out), st) == -1        # METRPO_EINVAL
    assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(nb), C.byref(par), C.byref(kp), 1, None, None, st) == -1
    for bad in ((-0.5, 0.01), (float('nan'), 0.01), (float('inf'), 0.01), (1.0, float('nan')), (1.0, float('inf'))):
        assert lib.metrpo_ppo_kl_loss_grad(eng._ctx, C.byref(b), C.byref(par), C.byref(_lib.PpoKlParams(*bad)), None, p(out), st) == -1, bad
        assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(b), C.byref(par), C.byref(_lib.PpoKlParams(*bad)), 1, None, None, st) == -1, bad
    assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(b), C.byref(_lib.PpoParams(0.3, 0.0, -1e-3, 0.9, 0.999, 1e-8)), C.byref(kp), 1, None, None, st) == -1
    assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(b), C.byref(par), C.byref(kp), -1, None, None, st) == -1
    assert eng.get_policy_adam()[2] == 0                                                                               # nothing was stepped
    # an open TRPO update: METRPO_ESTATE
    assert eng.trpo_update(b, spec_trials=1) is None
    assert lib.metrpo_ppo_kl_update(eng._ctx, C.byref(b), C.byref(par), C.byref(kp), 1, None, None, st) == -5
    eng.trpo_update_end()
    torch.cuda.synchronize()


def _ppo_kl_setup(reset=True, seed=3):
    import metrpo_amd
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    p['algo'] = 'ppo'
    p['n_models'] = 2
    p['dynamics_model']['hidden_layers'] = [64, 64]
    po = p['policy_opt_params']
    po.update(T=10, log_every=1, max_iters=3, num_iters_threshold=2)
    po['ppo'] = dict(batch_size=1000, init_std=0.7, reset=reset, n_epochs=3, clip_lr=0.2, entropy_bonus_coeff=0.01, use_kl_penalty=True,
                     initial_kl_penalty=4.0, step_size=1e-5)
    s = metrpo_amd.from_params(p, seed=seed)
    assert isinstance(s.algo, metrpo_amd.PPO) and s.algo.use_kl_penalty and (s.algo.kl_penalty, s.algo.step_size) == (4.0, 1e-5)
    dm, _, _, pool = O.make_problem('swimmer', K=2, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=4)
    s.engine.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    return s, pool[:50].astype(np.float32)


def test_early_stop_loop_runs_the_penalised_ppo_and_restores_theta_and_adam_state():
    """9: early_stop.optimize_policy with PPO(use_kl_penalty=True) (C0-sized): a never-improving run restores theta AND (m, v, t); a normal run
    advances t by n_epochs per iteration; optimize_policy's LossAfter carries the penalty (the gate is open after three epochs at step_size 1e-5)."""
    from metrpo_amd import early_stop
    s, val = _ppo_kl_setup(reset=False)
    eng = s.engine
    m0, v0, t0 = _adam_state(eng.P, 3)
    eng.set_policy_adam(m0, v0, t0)
    entry = _state(eng)
    kw = dict(s.optimize_policy_kwargs, stop_fn=lambda old, new, mode='scalar': True)       # every candidate is "worse"
    out = early_stop.optimize_policy(s.algo, val, **kw)
    assert out['best_index'] == 0 and out['last_index'] == 2
    end = _state(eng)
    assert end[3] == entry[3] == t0
    assert all(np.array_equal(a, c) for a, c in zip(end[:3], entry[:3]))
    kw = dict(s.optimize_policy_kwargs, mode='no_early', max_iters=2)
    early_stop.optimize_policy(s.algo, val, **kw)
    assert _state(eng)[3] == t0 + 2 * 3 and not np.array_equal(_state(eng)[0], entry[0])
    s.algo.start_worker()
    sd = s.algo.process_samples(1, s.algo.obtain_samples(1))
    d = s.algo.optimize_policy(1, sd)
    assert sorted(d) == ['LossAfter', 'LossBefore', 'MeanKL', 'MeanKLBefore', 'UnclippedSurrLoss']
    vals = {k: float(cpu(x)[0]) for k, x in d.items()}
    assert all(np.isfinite(x) for x in vals.values()) and abs(vals['MeanKLBefore']) <= 1e-6 and vals['MeanKL'] > 1.1e-5, vals
    # LossAfter = the unpenalised loss at the same theta + kl_penalty * (MeanKL - step_size)
    agent = sd["agent_infos"]
    b = eng.make_batch(sd["observations"], sd["actions"], sd["advantages"], agent["mean"], agent["log_std"], valid=sd.get("valids"))
    plain = float(cpu(eng.ppo_loss_grad(b, 0.2, 0.01))[0])
    want = plain + 4.0 * (vals['MeanKL'] - 1e-5)
    assert abs(vals['LossAfter'] - want) <= TOL.LOSS_RTOL * max(1.0, abs(want)), (vals, plain)


def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    """8: 2 processes on cuda:0 with the one-shot exchange, three fused epochs of metrpo_ppo_kl_update on half the batch each: the mean-KL reduction
    carries the exchange like the gradient reduction.  step_size lies between every rank's own share of the mean KL and the global mean at entry
    (asserted by the helper on the device's numbers and here on the reference's): the gate is open only because the shares are summed first.
    theta is bit-identical on both ranks (the helper) and within MULTI_RANK_THETA of the one-rank result."""
    cs = dict(T.case('mfma', epochs=3, ent=0.02, lr=1e-3))
    N, n = cs['N'], int(cs['valid'].sum())
    whole = K.mean_kl(cs['theta'], cs['pdims'], cs['obs'], cs['old_mean'], cs['old_ls'], cs['valid'])
    shares = [K.mean_kl(cs['theta'], cs['pdims'], cs['obs'][lo:hi], cs['old_mean'][lo:hi], cs['old_ls'][lo:hi], cs['valid'][lo:hi], n_global=n)
              for lo, hi in ((0, N // 2), (N // 2, N))]
    step, beta = 0.75 * whole, 8.0
    assert max(shares) < 0.9 * step and step < 0.9 * whole, (shares, step, whole)
    out_file = str(tmp_path / 'ppo_kl_ranks.npz')
    world, port = 2, 29641
    cmd = ['timeout', '-k', '10', '600', sys.executable, os.path.join(HERE, '_two_rank_ppo_kl.py'), out_file, repr(step), repr(beta)]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=660)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    assert all(pr.returncode == 0 for pr in procs), '\n'.join(l[-3000:] for l in logs)
    many = np.load(out_file)
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 2)
    eng.set_policy_adam(m0, v0, t0)
    plain_theta = None
    losses, kls = eng.ppo_kl_update(b, n_epochs=3, clip_lr=cs['clip'], entropy_bonus_coeff=0.02, kl_penalty=beta, step_size=step, lr=1e-3, want_mean_kls=True)
    losses, kls = cpu(losses), cpu(kls)
    one = _state(eng)
    assert int(many['t']) == one[3] == t0 + 3
    stepv = np.abs(one[0] - cs['theta']).max()
    np.testing.assert_allclose(many['theta'], one[0], rtol=0, atol=TOL.MULTI_RANK_THETA * stepv + 1e-7)
    assert rel_l2(many['m'], one[1]) <= 1e-4 and rel_l2(many['v'], one[2]) <= 1e-4
    np.testing.assert_allclose(many['loss'], losses, rtol=TOL.LOSS_RTOL, atol=TOL.LOSS_RTOL)
    np.testing.assert_allclose(many['kl'], kls, rtol=TOL.LOSS_RTOL, atol=TOL.LOSS_RTOL)
    # the penalty acted: without it the same three epochs end somewhere else
    eng.set_policy(cs['theta']); eng.set_policy_adam(m0, v0, t0)
    eng.ppo_update(b, n_epochs=3, clip_lr=cs['clip'], entropy_bonus_coeff=0.02, lr=1e-3)
    plain_theta = _state(eng)[0]
    assert np.abs(plain_theta - one[0]).max() > 10 * (TOL.MULTI_RANK_THETA * stepv + 1e-7)
