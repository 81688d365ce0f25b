"""'vpg' policy update on the GPU (metrpo_vpg_loss_grad / metrpo_vpg_update: the UPD_VPG instantiations of the update kernels in
csrc/policy_update.hip, policy_mfma.hip, policy_fused3.hip and policy_gemm.hip, and k_finalize's Adam tail) against the float64
restatement tests/vpg_ref.py, on every update family; the fused step against its two-call form; the 'vpg' branch of
early_stop.optimize_policy; two ranks on one GPU with the one-shot exchange.  Tolerances: tests/tolerances.py."""
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
import vpg_ref as R
from test_gpu_engine import _update_problem, rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# family -> (env, policy hidden layers, set_update_path argument, N, expected update_path(N))
FAMILIES = {
    'generic': ('swimmer', (32, 32), False, 5000, 'generic'),
    'gemm': ('swimmer', (32, 32), 'gemm', 9000, 'gemm'),
    'mfma': ('swimmer', (32, 32), True, 5000, 'mfma'),                 # the 2 x 32 MFMA kernels (C1's policy)
    'fused3': ('humanoid', (100, 50, 25), True, 20011, 'mfma'),       # the fused 100-50-25 kernels (params-humanoid.json)
}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _problem(family, seed=31):
    env, ph, path, N, expect = FAMILIES[family]
    eng, th, pdims, obs, act, adv, om, ols = _update_problem(env, N, seed=seed, pol_hidden=ph)
    assert eng.set_update_path(path) == path
    assert eng.update_path(N) == expect
    na = pdims[-1]
    # one log_std below log(1e-6) (clamped: zero gradient), the others away from the clamp
    th = th.copy()
    th[-na] = -20.0
    eng.set_policy(th)
    valid = np.ones(N, np.uint8); valid[::7] = 0; valid[5] = 0
    return eng, th, pdims, obs, act, adv, om, ols, valid


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_vpg_loss_grad_matches_reference(family):
    eng, th, pdims, obs, act, adv, om, ols, valid = _problem(family)
    keep = valid.astype(bool)
    loss, g = R.loss_grad(th, pdims, obs, act, adv, valid=valid)
    assert g[-pdims[-1]] == 0.0
    for b in (eng.make_batch(obs, act, adv, None, None, valid=valid),              # VPG reads no old distribution
              eng.make_batch(obs, act, adv, om, ols[0], valid=valid)):              # ... and ignores one that is there (broadcast log_std)
        out = cpu(eng.vpg_loss_grad(b))
        assert abs(out[0] - loss) <= TOL.LOSS_RTOL * max(1.0, abs(loss)), (out[0], loss)
        assert rel_l2(out[1:], g) <= TOL.GRAD_REL_L2, rel_l2(out[1:], g)
        assert out[-pdims[-1]] == 0.0
    # at theta_old the likelihood ratio is 1: the VPG gradient is the TRPO surrogate's gradient.  (Not with a clamped log_std: there std = 1e-6
    # turns the fp32 rounding of the stored mean into ratios of exp(1e12 x rounding) in the TRPO kernels -- the reference's graph alike.)
    th = th.copy(); th[-pdims[-1]] = -0.3
    eng.set_policy(th)
    mean = O.policy_mean(th, pdims, obs).astype(np.float32).astype(np.float64)
    lso = np.broadcast_to(O.policy_log_std(th, pdims), mean.shape).copy()
    at_old = eng.make_batch(obs, act, adv, mean, lso, valid=valid)
    g_trpo = cpu(eng.loss_grad(at_old))[1:]
    g_vpg = cpu(eng.vpg_loss_grad(at_old))[1:]
    assert rel_l2(g_vpg, g_trpo) <= TOL.GRAD_REL_L2, rel_l2(g_vpg, g_trpo)
    assert keep.sum() < len(keep)


def _adam_state(eng, seed):
    rng = np.random.RandomState(seed)
    m = (rng.randn(eng.P) * 1e-3).astype(np.float32)
    v = (rng.rand(eng.P) * 1e-5 + 1e-6).astype(np.float32)
    return m, v, 5


def _state(eng):
    m, v, t = eng.get_policy_adam()
    return cpu(eng.get_policy()), cpu(m), cpu(v), t


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_fused_step_is_bitwise_the_two_call_form(family):
    """vpg_update == vpg_loss_grad + policy_adam_step(clip_val=0), bit for bit in theta, m, v and t; the loss is the gradient pass's."""
    eng, th, pdims, obs, act, adv, om, ols, valid = _problem(family)
    b = eng.make_batch(obs, act, adv, None, None, valid=valid)
    m0, v0, t0 = _adam_state(eng, 1)
    eng.set_policy_adam(m0, v0, t0)
    lg = eng.vpg_loss_grad(b)
    eng.policy_adam_step(lg[1:], 1e-3, clip_val=None)
    two = _state(eng)
    eng.set_policy(th); eng.set_policy_adam(m0, v0, t0)
    loss = eng.vpg_update(b, lr=1e-3)
    one = _state(eng)
    assert one[3] == two[3] == t0 + 1
    for a, c in zip(one[:3], two[:3]):
        assert np.array_equal(a, c)
    assert cpu(loss)[0] == cpu(lg)[0]
    assert not np.array_equal(one[0], th)


@pytest.mark.parametrize('family', ['generic', 'mfma', 'fused3'])
def test_three_updates_track_tf_adam_and_repeat_bitwise(family):
    eng, th, pdims, obs, act, adv, om, ols, valid = _problem(family)
    b = eng.make_batch(obs, act, adv, None, None, valid=valid)
    m0, v0, t0 = _adam_state(eng, 2)
    runs = []
    for _ in range(2):
        eng.set_policy(th); eng.set_policy_adam(m0, v0, t0)
        states = []
        for k in range(3):
            prev = _state(eng)
            loss = eng.vpg_update(b, lr=1e-2)
            cur = _state(eng)
            states.append(cur)
            # the reference step from the device's own state: gradient at the device theta, TF-Adam in float64
            l_ref, g_ref = R.loss_grad(prev[0], pdims, obs, act, adv, valid=valid)
            th_r, m_r, v_r, t_r = R.adam_step(prev[0], prev[1], prev[2], prev[3], g_ref, lr=1e-2)
            assert cur[3] == t_r == t0 + k + 1
            assert abs(cpu(loss)[0] - l_ref) <= TOL.LOSS_RTOL * max(1.0, abs(l_ref))
            assert rel_l2(cur[1], m_r) <= 1e-4 and rel_l2(cur[2], v_r) <= 1e-4
            assert rel_l2(cur[0] - prev[0], th_r - prev[0]) <= 1e-3, rel_l2(cur[0] - prev[0], th_r - prev[0])
        runs.append(states)
    for s1, s2 in zip(*runs):
        assert all(np.array_equal(a, c) for a, c in zip(s1[:3], s2[:3]))


def test_bad_arguments():
    from metrpo_amd import _lib
    lib = _lib.lib
    eng, th, pdims, obs, act, adv, om, ols, valid = _problem('mfma')
    b = eng.make_batch(obs, act, adv, None, None)
    out = torch.empty(eng.P + 1, dtype=torch.float64, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    par = _lib.VpgParams(1e-3, 0.9, 0.999, 1e-8)
    assert lib.metrpo_vpg_loss_grad(eng._ctx, C.byref(b), None, eng._stream()) == -2              # METRPO_ENULL
    assert lib.metrpo_vpg_update(eng._ctx, C.byref(b), None, None, eng._stream()) == -2
    for bad in ((-1e-3, 0.9, 0.999, 1e-8), (1e-3, 1.0, 0.999, 1e-8), (1e-3, 0.9, -0.1, 1e-8), (1e-3, 0.9, 0.999, float('nan'))):
        assert lib.metrpo_vpg_update(eng._ctx, C.byref(b), C.byref(_lib.VpgParams(*bad)), None, eng._stream()) == -1   # METRPO_EINVAL
    nb = eng.make_batch(obs, act, adv, None, None); nb.N = 0
    assert lib.metrpo_vpg_loss_grad(eng._ctx, C.byref(nb), p(out), eng._stream()) == -1
    nb = eng.make_batch(obs, act, adv, None, None); nb.d_adv = None
    assert lib.metrpo_vpg_loss_grad(eng._ctx, C.byref(nb), p(out), eng._stream()) == -2
    assert lib.metrpo_vpg_update(eng._ctx, C.byref(nb), C.byref(par), None, eng._stream()) == -2
    assert lib.metrpo_loss_grad(eng._ctx, C.byref(b), p(out), eng._stream()) == -2                  # TRPO still needs the old distribution
    assert eng.get_policy_adam()[2] == 0                                                            # nothing was stepped
    torch.cuda.synchronize()


def _vpg_setup(reset=True, seed=3):
    import metrpo_amd
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    p['algo'] = 'vpg'
    p['n_models'] = 2
    p['dynamics_model']['hidden_layers'] = [64, 64]
    po = p['policy_opt_params']
    po.update(T=10, log_every=1, max_iters=3, num_iters_threshold=2)
    po['vpg'].update(batch_size=1000, init_std=0.7, reset=reset)
    s = metrpo_amd.from_params(p, seed=seed)
    assert isinstance(s.algo, metrpo_amd.VPG) and s.shapes['batch_size'] == 1000
    dm, _, _, pool = O.make_problem('swimmer', K=2, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=4)
    s.engine.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    return s, pool[:50].astype(np.float32)


def test_loop_never_improving_restores_theta_and_adam_state():
    from metrpo_amd import early_stop
    s, val = _vpg_setup(reset=False)
    eng = s.engine
    m0, v0, t0 = _adam_state(eng, 3)
    eng.set_policy_adam(m0, v0, t0)
    entry = _state(eng)
    kw = dict(s.optimize_policy_kwargs, stop_fn=lambda old, new, mode='scalar': True)       # every candidate is "worse"
    out = early_stop.optimize_policy(s.algo, val, **kw)
    assert out['best_index'] == 0 and out['last_index'] == 2
    end = _state(eng)
    assert end[3] == entry[3] == t0
    assert all(np.array_equal(a, c) for a, c in zip(end[:3], entry[:3]))


def test_loop_adam_state_carries_over_and_log_std_reset():
    from metrpo_amd import early_stop
    s, val = _vpg_setup(reset=True)
    eng = s.engine
    th = cpu(eng.get_policy()); th[-eng.na:] = -1.5
    eng.set_policy(th)
    kw = dict(s.optimize_policy_kwargs, mode='no_early', max_iters=2)
    assert kw['reset_log_std'] is True
    early_stop.optimize_policy(s.algo, val, **kw)
    th1, m1, v1, t1 = _state(eng)
    assert t1 == 2 and np.abs(m1).max() > 0
    # log_std was reset to log(vpg.init_std), then moved by two Adam steps of at most ~lr each
    np.testing.assert_allclose(th1[-eng.na:], np.log(0.7), atol=3e-3)
    early_stop.optimize_policy(s.algo, val, **kw)
    assert _state(eng)[3] == 4                                   # not reset between calls (policy_adam_init is empty for vpg)
    # a never-improving run right after a reset restores the reset log_std exactly
    th = cpu(eng.get_policy()); th[-eng.na:] = -1.5
    eng.set_policy(th)
    early_stop.optimize_policy(s.algo, val, **dict(s.optimize_policy_kwargs, stop_fn=lambda old, new, mode='scalar': True))
    assert np.array_equal(cpu(eng.get_policy())[-eng.na:], np.full(eng.na, np.float32(np.log(0.7)), np.float64))
    assert np.all(np.isfinite(cpu(eng.get_policy())))


@pytest.mark.parametrize('path', ['mfma', 'gemm'])
def test_two_ranks_on_one_gpu_equal_one_rank(path, tmp_path):
    """2 processes on cuda:0 (3 with this one) with the one-shot exchange: the MFMA path carries the exchange and the step in k_finalize's
    tail, the GEMM path all-reduces between its reduction and the stand-alone step."""
    out_file = str(tmp_path / 'vpg_ranks.npz')
    world, port = 2, 29611 + (path == 'gemm')
    cmd = [sys.executable, os.path.join(HERE, '_two_rank_vpg.py'), out_file, path]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT,
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=600)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    assert all(pr.returncode == 0 for pr in procs), '\n'.join(l[-3000:] for l in logs)
    many = np.load(out_file)
    eng, th, pdims, obs, act, adv, om, ols = _update_problem(N=6000, seed=29)
    eng.set_update_path({'mfma': True, 'gemm': 'gemm'}[path])
    m0, v0, t0 = _adam_state(eng, 4)
    eng.set_policy_adam(m0, v0, t0)
    b = eng.make_batch(obs, act, adv, None, None)
    for _ in range(2):
        eng.vpg_update(b, lr=1e-2)
    one = _state(eng)
    assert int(many['t']) == one[3] == t0 + 2
    step = np.abs(one[0] - th).max()
    np.testing.assert_allclose(many['theta'], one[0], rtol=0, atol=TOL.MULTI_RANK_THETA * step + 1e-7)
    assert rel_l2(many['m'], one[1]) <= 1e-4 and rel_l2(many['v'], one[2]) <= 1e-4
