"""'ppo' policy update on the GPU (metrpo_ppo_loss_grad / metrpo_ppo_update: the OP_PPO instantiations of the update kernels in
csrc/policy_update.hip, policy_mfma.hip, policy_fused3.hip and policy_gemm.hip, the entropy term and the Adam tail of k_finalize) against the
float64 restatement tests/ppo_ref.py, on every update family of test_gpu_vpg.FAMILIES; the fused epochs against their two-call form; no host
wait between the epochs; the 'ppo' branch of early_stop.optimize_policy; two ranks on one GPU with the one-shot exchange.
Tolerances: tests/tolerances.py.

The gate of the clipped surrogate is discontinuous in the likelihood ratio, and fp32 cannot be held to a sample whose float64 ratio lies within
BAND = 1e-4 of 1 +- c (about 10x the fp32 error of a ratio of O(1)): the reference marks those samples invalid for BOTH sides (case()), at most
CAP = 1 % of N, and the cases are chosen so that the reference alone stays under the cap and puts 10 % .. 90 % of the valid samples on the
clipped, zero-gradient side."""
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
from test_gpu_vpg import FAMILIES

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAND, CAP = 1e-4, 0.01
# family -> (clip_lr, scale of the move off theta_old): per case, so that the reference's clipped share lies in [0.1, 0.9] (asserted in case())
CLIP = {'generic': (0.05, 0.02), 'gemm': (0.08, 0.02), 'mfma': (0.05, 0.02), 'fused3': (0.1, 0.004)}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def rel_l2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def near_bound(ratio, clip):
    """Samples whose float64 likelihood ratio lies within BAND of a clip bound 1 +- clip: marked invalid for both sides."""
    return (np.abs(ratio - (1 - clip)) < BAND) | (np.abs(ratio - (1 + clip)) < BAND)


def case(family, seed=41, moved=True, epochs=0, ent=0.0, lr=1e-2):
    """The data of one case, on the CPU alone (no engine): theta_old, theta (moved off it by a fixed random direction), the batch with the old
    distribution of theta_old, and `valid` with the reference's near-bound samples removed -- at theta for the gradient cases, at the theta of
    every reference epoch for the multi-epoch ones (iterated until the set is stable).  log_std stays away from the clamp."""
    env, ph, path, N, expect = FAMILIES[family]
    clip, scale = CLIP[family]
    _, theta0, pdims, _ = O.make_problem(env, K=2, dyn_hidden=(64, 64), pol_hidden=ph, seed=seed, n_pool=8)
    rng = np.random.RandomState(seed)
    na = pdims[-1]
    th_old = theta0 + rng.randn(theta0.size) * 0.05
    th_old[-na:] = rng.randn(na) * 0.2 - 0.3
    th_old = f32(th_old)
    obs = f32(rng.randn(N, pdims[0]) * 0.5)
    old_mean = f32(O.policy_mean(th_old, pdims, obs))
    old_ls = np.broadcast_to(th_old[-na:], old_mean.shape).copy()
    act = f32(old_mean + np.exp(old_ls) * rng.randn(N, na))
    adv = f32(O.center_advantages(rng.randn(N)))
    theta = f32(th_old + scale * rng.randn(th_old.size)) if moved else th_old.copy()
    valid = np.ones(N, np.uint8); valid[::7] = 0; valid[5] = 0
    base = valid.copy()

    def near(th):
        return near_bound(R.ratios(th, pdims, obs, act, old_mean, old_ls)[0], clip)
    if epochs == 0:
        valid[near(theta)] = 0
    else:
        m0, v0 = _adam_state(len(theta), 2)[:2]
        for _ in range(20):
            th, m, v, t, drop = theta, m0.astype(np.float64), v0.astype(np.float64), 5, np.zeros(N, bool)
            for _e in range(epochs):
                drop |= near(th)
                th, m, v, t, _l = R.adam_epochs(th, m, v, t, pdims, obs, act, adv, old_mean, old_ls, clip, ent, valid, n_epochs=1, lr=lr)
            if not (drop & valid.astype(bool)).any():
                break
            valid[drop] = 0
        else:
            raise AssertionError("the near-bound set of the reference did not settle")
    removed = int(base.sum() - valid.sum())
    assert removed <= CAP * N, (family, removed, N)
    _, _, ratio, gate = R.loss_grad(theta, pdims, obs, act, adv, old_mean, old_ls, clip, 0.0, valid)
    clipped = 1.0 - gate[valid.astype(bool)].mean()
    if moved:
        assert 0.1 <= clipped <= 0.9, (family, clipped)
    return dict(family=family, pdims=pdims, th_old=th_old, theta=theta, obs=obs, act=act, adv=adv, old_mean=old_mean, old_ls=old_ls,
                valid=valid, clip=clip, removed=removed, clipped=clipped, N=N)


def _adam_state(P, seed):
    rng = np.random.RandomState(seed)
    m = (rng.randn(P) * 1e-3).astype(np.float32)
    v = (rng.rand(P) * 1e-5 + 1e-6).astype(np.float32)
    return m, v, 5


def engine_for(cs):
    import metrpo_amd
    env, ph, path, N, expect = FAMILIES[cs['family']]
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    eng.set_policy(cs['theta'])
    assert eng.set_update_path(path) == path
    assert eng.update_path(N) == expect
    b = eng.make_batch(cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls'][0], valid=cs['valid'])
    return eng, b


def _state(eng):
    m, v, t = eng.get_policy_adam()
    return cpu(eng.get_policy()), cpu(m), cpu(v), t


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_ppo_loss_grad_matches_reference(family):
    """1: gradient parity with the gate in both states (case() asserts the clipped share and the removal cap)."""
    cs = case(family)
    eng, b = engine_for(cs)
    for ent in (0.0, 0.02):
        loss, g, _, _ = R.loss_grad(cs['theta'], cs['pdims'], cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls'], cs['clip'], ent, cs['valid'])
        out = cpu(eng.ppo_loss_grad(b, cs['clip'], ent))
        print('ppo parity %s ent=%g: clipped %.3f removed %d/%d loss err %.3g grad rel_l2 %.3g' % (
            family, ent, cs['clipped'], cs['removed'], cs['N'], abs(out[0] - loss) / max(1.0, abs(loss)), rel_l2(out[1:], g)))
        assert abs(out[0] - loss) <= TOL.LOSS_RTOL * max(1.0, abs(loss)), (out[0], loss)
        assert rel_l2(out[1:], g) <= TOL.GRAD_REL_L2, rel_l2(out[1:], g)


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_clamped_log_std_slot_has_exactly_zero_gradient(family):
    """1 (separate case): theta = theta_old with one log_std below log(1e-6) and ent_coeff > 0: that slot's gradient is exactly 0.0 -- no
    surrogate share, no entropy share.  (Nothing else is asserted: ratios are meaningless at std = 1e-6, test_gpu_vpg.py:62-63.)"""
    cs = case(family, moved=False)
    na = cs['pdims'][-1]
    cs['theta'] = cs['theta'].copy(); cs['theta'][-na] = -20.0
    eng, b = engine_for(cs)
    out = cpu(eng.ppo_loss_grad(b, 0.2, 0.05))
    assert out[-na] == 0.0
    assert np.all(out[-na + 1:] != 0.0) if na > 1 else True


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_at_theta_old_and_with_a_huge_clip_it_is_the_trpo_surrogate(family):
    """2: at theta_old every ratio is 1, nothing is gated (the tie goes to the unclipped branch); with clip_lr huge nothing is gated anywhere."""
    cs = case(family, moved=False)
    eng, b = engine_for(cs)
    a, g = cpu(eng.ppo_loss_grad(b, cs['clip'], 0.0)), cpu(eng.loss_grad(b))
    assert rel_l2(a[1:], g[1:]) <= TOL.GRAD_REL_L2 and abs(a[0] - g[0]) <= TOL.LOSS_RTOL * max(1.0, abs(g[0]))
    cm = case(family)
    eng, b = engine_for(cm)
    a, g = cpu(eng.ppo_loss_grad(b, 1e9, 0.0)), cpu(eng.loss_grad(b))
    assert rel_l2(a[1:], g[1:]) <= TOL.GRAD_REL_L2 and abs(a[0] - g[0]) <= TOL.LOSS_RTOL * max(1.0, abs(g[0]))
    c = cpu(eng.ppo_loss_grad(b, cm['clip'], 0.0))
    assert rel_l2(c[1:], g[1:]) > 0.05                          # ... and the gate of the real clip is not a no-op there


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_fused_epochs_are_bitwise_the_two_call_form(family):
    """3 and 5: ppo_update(n_epochs=1) is ppo_loss_grad + policy_adam_step(clip_val=None) bit for bit in theta, m, v and t; n_epochs=4 is four
    such pairs; d_losses has one entry per epoch and entry e is the ppo_loss_grad loss at the theta entering epoch e."""
    cs = case(family)
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 1)
    ent = 0.02
    for n in (1, 4):
        eng.set_policy(cs['theta']); eng.set_policy_adam(m0, v0, t0)
        two_losses = []
        for _ in range(n):
            lg = eng.ppo_loss_grad(b, cs['clip'], ent)
            two_losses.append(cpu(lg)[0])
            eng.policy_adam_step(lg[1:], 1e-2, clip_val=None)
        two = _state(eng)
        eng.set_policy(cs['theta']); eng.set_policy_adam(m0, v0, t0)
        losses = eng.ppo_update(b, n_epochs=n, clip_lr=cs['clip'], entropy_bonus_coeff=ent, lr=1e-2)
        one = _state(eng)
        assert one[3] == two[3] == t0 + n
        for a, c in zip(one[:3], two[:3]):
            assert np.array_equal(a, c)
        assert losses.shape == (n,) and np.array_equal(cpu(losses), np.array(two_losses))
        assert not np.array_equal(one[0], cs['theta'])
    assert eng.ppo_update(b, n_epochs=0, want_losses=True).shape == (0,) and _state(eng)[3] == t0 + 4


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_four_epochs_track_the_reference(family):
    """4: four epochs against ppo_ref.adam_epochs, in the form of test_gpu_vpg's multi-step test: each epoch's reference step starts from the
    DEVICE's own state (theta, m, v, t), with the bounds of that test (loss within LOSS_RTOL, Adam moments rel-L2 <= 1e-4, theta step rel-L2
    <= 1e-3).  The epochs are single-epoch calls here because the near-bound samples have to be taken out at each epoch's theta (a fused run
    cannot be masked in between, and masking the union of a reference trajectory's bands moves that trajectory by more than the band: it does
    not settle); that the fused four-epoch call is these four calls bit for bit is test_fused_epochs_are_bitwise_the_two_call_form.
    Observed on an MI355X, worst of the four epochs (loss error / max(1, |loss|), rel-L2 of m, of v and of the theta step; bounds LOSS_RTOL, 1e-4, 1e-4,
    1e-3): fused3 loss 5.05e-08, m 3.03e-07, v 2.83e-07, theta step 5.38e-06; gemm loss 6.56e-09, m 2.87e-07, v 1.66e-06, theta step 5.07e-06; generic loss
    8.01e-09, m 2.37e-07, v 1.13e-06, theta step 4.53e-06; mfma loss 7.85e-09, m 2.36e-07, v 1.13e-06, theta step 4.53e-06."""
    ent, lr = 0.02, 1e-2
    cs = case(family)
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 2)
    eng.set_policy_adam(m0, v0, t0)
    base = np.ones(cs['N'], np.uint8); base[::7] = 0; base[5] = 0
    worst = np.zeros(4)
    for k in range(4):
        prev = _state(eng)
        ratio = R.ratios(prev[0], cs['pdims'], cs['obs'], cs['act'], cs['old_mean'], cs['old_ls'])[0]
        valid = base.copy()
        valid[(np.abs(ratio - (1 - cs['clip'])) < BAND) | (np.abs(ratio - (1 + cs['clip'])) < BAND)] = 0
        assert base.sum() - valid.sum() <= CAP * cs['N']
        bk = eng.make_batch(cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls'][0], valid=valid)
        loss = cpu(eng.ppo_update(bk, n_epochs=1, clip_lr=cs['clip'], entropy_bonus_coeff=ent, lr=lr))
        cur = _state(eng)
        th_r, m_r, v_r, t_r, l_r = R.adam_epochs(prev[0], prev[1], prev[2], prev[3], cs['pdims'], cs['obs'], cs['act'], cs['adv'], cs['old_mean'],
                                                  cs['old_ls'], cs['clip'], ent, valid, n_epochs=1, lr=lr)
        gate = R.loss_grad(prev[0], cs['pdims'], cs['obs'], cs['act'], cs['adv'], cs['old_mean'], cs['old_ls'], cs['clip'], ent, valid)[3]
        figs = np.array([abs(loss[0] - l_r[0]) / max(1.0, abs(l_r[0])), rel_l2(cur[1], m_r), rel_l2(cur[2], v_r), rel_l2(cur[0] - prev[0], th_r - prev[0])])
        worst = np.maximum(worst, figs)
        print('ppo epoch %d %s: clipped %.3f removed %d  loss %.3g  m %.3g  v %.3g  theta step %.3g' % (
            (k, family, 1.0 - gate[valid.astype(bool)].mean(), base.sum() - valid.sum()) + tuple(figs)))
        assert cur[3] == t_r == t0 + k + 1
        assert figs[0] <= TOL.LOSS_RTOL, figs
        assert figs[1] <= 1e-4 and figs[2] <= 1e-4, figs
        assert figs[3] <= 1e-3, figs
    print('ppo 4 epochs %s worst: loss %.3g  m %.3g  v %.3g  theta step %.3g' % ((family,) + tuple(worst)))


def test_no_host_wait_between_the_epochs():
    """6: the call only enqueues.  A spin kernel keeps the stream busy for ~0.4 s in front of it; metrpo_ppo_update with four epochs returns
    while the event recorded behind the spin kernel has not fired (a host read between epochs would have to wait for it)."""
    cs = case('mfma')
    eng, b = engine_for(cs)
    dev = eng.device
    eng.ppo_update(b, n_epochs=1, clip_lr=cs['clip'])             # workspaces and the Adam state exist
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
        losses = eng.ppo_update(b, n_epochs=4, clip_lr=cs['clip'], entropy_bonus_coeff=0.01)
        still_busy = not front.query()
    torch.cuda.synchronize()
    assert still_busy, "ppo_update waited for the device: the event in front of it had fired when it returned"
    assert eng.get_policy_adam()[2] == t_before + 4 and np.all(np.isfinite(cpu(losses)))


def test_bad_arguments():
    from metrpo_amd import _lib
    lib = _lib.lib
    cs = case('mfma')
    eng, b = engine_for(cs)
    out = torch.empty(eng.P + 1, dtype=torch.float64, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    par = _lib.PpoParams(0.3, 0.0, 1e-3, 0.9, 0.999, 1e-8)
    assert lib.metrpo_ppo_loss_grad(eng._ctx, C.byref(b), C.byref(par), None, eng._stream()) == -2          # METRPO_ENULL
    assert lib.metrpo_ppo_loss_grad(eng._ctx, C.byref(b), None, p(out), eng._stream()) == -2
    assert lib.metrpo_ppo_update(eng._ctx, C.byref(b), None, 1, None, eng._stream()) == -2
    nb = eng.make_batch(cs['obs'], cs['act'], cs['adv'], None, None)                                        # no old distribution
    assert lib.metrpo_ppo_loss_grad(eng._ctx, C.byref(nb), C.byref(par), p(out), eng._stream()) == -1        # METRPO_EINVAL, naming PPO
    assert b'PPO' in lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_ppo_update(eng._ctx, C.byref(nb), C.byref(par), 1, None, eng._stream()) == -1
    for bad in ((-0.1, 0.0, 1e-3, 0.9, 0.999, 1e-8), (0.3, float('nan'), 1e-3, 0.9, 0.999, 1e-8), (0.3, 0.0, -1e-3, 0.9, 0.999, 1e-8),
                (0.3, 0.0, 1e-3, 1.0, 0.999, 1e-8)):
        assert lib.metrpo_ppo_update(eng._ctx, C.byref(b), C.byref(_lib.PpoParams(*bad)), 1, None, eng._stream()) == -1
    assert lib.metrpo_ppo_update(eng._ctx, C.byref(b), C.byref(par), -1, None, eng._stream()) == -1
    assert eng.get_policy_adam()[2] == 0                                                                    # nothing was stepped
    torch.cuda.synchronize()


def _ppo_setup(reset=True, seed=3):
    import metrpo_amd
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    p['algo'] = 'ppo'
    p['n_models'] = 2
    p['dynamics_model']['hidden_layers'] = [64, 64]
    po = p['policy_opt_params']
    po.update(T=10, log_every=1, max_iters=3, num_iters_threshold=2)
    po['ppo'] = dict(batch_size=1000, init_std=0.7, reset=reset, n_epochs=3, clip_lr=0.2, entropy_bonus_coeff=0.01)
    s = metrpo_amd.from_params(p, seed=seed)
    assert isinstance(s.algo, metrpo_amd.PPO) and s.shapes['batch_size'] == 1000 and s.algo.optimizer.n_epochs == 3
    dm, _, _, pool = O.make_problem('swimmer', K=2, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=4)
    s.engine.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    return s, pool[:50].astype(np.float32)


def test_early_stop_loop_restores_theta_and_adam_state_and_carries_them_over():
    """7: the 'ppo' branch of early_stop.optimize_policy (C0-sized): a never-improving run restores theta AND (m, v, t); a normal run leaves t
    advanced by n_epochs per iteration, not reset at entry; optimize_policy returns the five diagnostics."""
    from metrpo_amd import early_stop
    s, val = _ppo_setup(reset=False)
    eng = s.engine
    m0, v0, t0 = _adam_state(eng.P, 3)
    eng.set_policy_adam(m0, v0, t0)
    entry = _state(eng)
    kw = dict(s.optimize_policy_kwargs, stop_fn=lambda old, new, mode='scalar': True)       # every candidate is "worse"
    assert kw['reset_log_std'] is False
    out = early_stop.optimize_policy(s.algo, val, **kw)
    assert out['best_index'] == 0 and out['last_index'] == 2
    end = _state(eng)
    assert end[3] == entry[3] == t0
    assert all(np.array_equal(a, c) for a, c in zip(end[:3], entry[:3]))
    kw = dict(s.optimize_policy_kwargs, mode='no_early', max_iters=2)
    early_stop.optimize_policy(s.algo, val, **kw)
    assert _state(eng)[3] == t0 + 2 * 3 and not np.array_equal(_state(eng)[0], entry[0])
    early_stop.optimize_policy(s.algo, val, **kw)
    assert _state(eng)[3] == t0 + 4 * 3                                                       # not reset between calls
    s.algo.start_worker()
    sd = s.algo.process_samples(1, s.algo.obtain_samples(1))
    d = s.algo.optimize_policy(1, sd)
    assert sorted(d) == ['LossAfter', 'LossBefore', 'MeanKL', 'MeanKLBefore', 'UnclippedSurrLoss']
    vals = {k: float(cpu(x)[0]) for k, x in d.items()}
    assert all(np.isfinite(x) for x in vals.values()) and abs(vals['MeanKLBefore']) <= 1e-6 and vals['MeanKL'] > 0.0, vals


def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    """8: 2 processes on cuda:0 (3 with this one) with the one-shot exchange: each epoch's reduction carries the exchange, the entropy term and
    the step in its tail.  theta is bit-identical on both ranks (asserted by the helper) and within MULTI_RANK_THETA of the one-rank result."""
    out_file = str(tmp_path / 'ppo_ranks.npz')
    world, port = 2, 29631
    cmd = ['timeout', '-k', '10', '600', sys.executable, os.path.join(HERE, '_two_rank_ppo.py'), out_file]
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
    cs = case('mfma', epochs=3, ent=0.02, lr=1e-3)
    eng, b = engine_for(cs)
    m0, v0, t0 = _adam_state(eng.P, 2)
    eng.set_policy_adam(m0, v0, t0)
    losses = cpu(eng.ppo_update(b, n_epochs=3, clip_lr=cs['clip'], entropy_bonus_coeff=0.02, lr=1e-3))
    one = _state(eng)
    assert int(many['t']) == one[3] == t0 + 3
    step = np.abs(one[0] - cs['theta']).max()
    np.testing.assert_allclose(many['theta'], one[0], rtol=0, atol=TOL.MULTI_RANK_THETA * step + 1e-7)
    assert rel_l2(many['m'], one[1]) <= 1e-4 and rel_l2(many['v'], one[2]) <= 1e-4
    np.testing.assert_allclose(many['loss'], losses, rtol=TOL.LOSS_RTOL, atol=TOL.LOSS_RTOL)
