"""'bptt-stochastic' policy update on the GPU (metrpo_bptt_grad_stochastic: csrc/bptt.hip, bptt_mfma.hip, det_gemm.hip) against the float64
restatement of tests/bptt_stochastic_ref.py, on every BPTT sweep family; the production Philox draws against their NumPy restatement; the
BPTT(stochastic=True) training loop and a 'bptt-stochastic' params file through from_params and the early-stopping driver."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
import bptt_stochastic_ref as R
import helpers as Hh
import tolerances as TOL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def cpu(t):
    return t.detach().cpu().numpy()


def rel_l2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def setup(env, K, dh, ph, seed, scale=0.25):
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, ph, seed=seed)
    rng = np.random.RandomState(seed + 7)
    na = dm.na
    theta = theta + scale * rng.randn(theta.size)                # some actions saturate the clip
    theta[-na:] = rng.uniform(-1.2, 0.3, size=na)                  # log_std: exp() of the raw parameter, no min_std clamp
    eng.set_policy(theta)
    return eng, dm, pdims, pool, rng


def x0_for(env, pool, B):
    x0 = (pool[:B] * (3.0 if env in ('hopper', 'half_cheetah') else 1.0)).astype(np.float32)
    if env == 'ant':
        x0[:B // 4, 2] = 0.15                                      # done from the first step on
    return x0


def select(eng, path):
    """path 0: the generic sweeps (requested explicitly: small nets may also qualify for the GEMM path); 1 MFMA sweeps; 2 GEMM path."""
    assert eng.set_det_path(path != 0) == path


def check_parity(eng, dm, pdims, env, x0, T, gamma, eps):
    costs, grad, nsat = eng.bptt_grad_stochastic(x0, T, gamma, noise=eps.astype(np.float32), n_saturates=True)
    th = cpu(eng.get_policy()).astype(np.float64)
    rc, rg, rn = R.stochastic_costs_and_grad(dm.astype(np.float32).astype(np.float64), th, pdims, env, x0.astype(np.float64), T, gamma, f32(eps))
    np.testing.assert_allclose(cpu(costs), rc, **TOL.BPTT_COST)
    g = cpu(grad)
    assert rel_l2(g, rg) < TOL.BPTT_GRAD_REL_L2, rel_l2(g, rg)
    na = dm.na
    assert rel_l2(g[-na:], rg[-na:]) < TOL.BPTT_GRAD_REL_L2, (g[-na:], rg[-na:])
    assert np.abs(cpu(nsat) - rn).sum() <= 1                       # |u| == 1 counts; one rounding-level tie allowed
    assert rn.sum() > 0                                            # the case has saturating actions
    return g


# (env, K, dyn hidden, pol hidden, B, T, gamma, sweep family (select), policy perturbation)
FAMILIES = [
    ('swimmer', 3, (24, 16), (8, 8), 100, 12, 0.97, 0, 0.25),
    ('swimmer', 5, (64, 64), (32, 32), 200, 15, 1.0, 1, 0.25),
    ('ant', 3, (64, 64), (32, 32), 130, 12, 0.95, 1, 0.25),                # running `dones`
    ('swimmer', 4, (48, 20), (32, 32), 77, 10, 0.98, 1, 0.25),             # zero-padded narrow net on the MFMA sweeps
    ('swimmer', 3, (128, 128), (32, 32), 150, 8, 0.97, 2, 0.25),          # k_dg_pre_mfma
    ('humanoid', 2, (128, 128), (20, 10, 5), 40, 5, 1.0, 2, 0.25),        # k_dg_pre (thread per row)
    ('humanoid', 2, (128, 128), (100, 50, 25), 40, 5, 1.0, 2, 0.05),      # k_dg_pre_mfma3
]


@pytest.mark.parametrize('env,K,dh,ph,B,T,gamma,path,scale', FAMILIES)
def test_parity_mode_matches_restatement(env, K, dh, ph, B, T, gamma, path, scale):
    eng, dm, pdims, pool, rng = setup(env, K, dh, ph, seed=111, scale=scale)
    select(eng, path)
    x0 = x0_for(env, pool, B)
    eps = rng.randn(K, T, B, dm.na)
    check_parity(eng, dm, pdims, env, x0, T, gamma, eps)


@pytest.mark.parametrize('dh,path', [((64, 64), 1), ((24, 16), 0), ((128, 128), 2)])
def test_noise_exactly_on_the_clip_bound_passes_the_gradient(dh, path):
    """u_pre == 1.0 exactly: action dim 0's mean is its bias 0.5 (zero weight column), std = exp(0) = 1, eps = 0.5."""
    ph = (32, 32) if path else (8, 8)
    eng, dm, pdims, pool, rng = setup('swimmer', 3, dh, ph, seed=112)
    th = cpu(eng.get_policy()).astype(np.float64)
    Ws, bs, ls = O.policy_unflatten(th, pdims)
    Ws[-1][:, 0] = 0.0; bs[-1][0] = 0.5; ls[0] = 0.0
    eng.set_policy(O.policy_flatten(Ws, bs, ls))
    select(eng, path)
    B, T = 90, 8
    eps = rng.randn(3, T, B, dm.na)
    on = rng.rand(3, T, B) < 0.4
    eps[..., 0][on] = 0.5
    g = check_parity(eng, dm, pdims, 'swimmer', x0_for('swimmer', pool, B), T, 1.0, eps)
    # the bias of dim 0 collects the bound samples' adjoint: a gate that dropped them would change it
    th2 = cpu(eng.get_policy()).astype(np.float64)
    _, rg, _ = R.stochastic_costs_and_grad(dm.astype(np.float32).astype(np.float64), th2, pdims, 'swimmer',
                                           x0_for('swimmer', pool, B).astype(np.float64), T, 1.0, f32(eps))
    b0 = th2.size - 2 * dm.na                                      # index of b_out[0] (layout W0 b0 ... W_out b_out log_std)
    np.testing.assert_allclose(g[b0], rg[b0], rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize('env,K,dh,ph,path', [('swimmer', 3, (64, 64), (32, 32), 1), ('swimmer', 3, (24, 16), (8, 8), 0),
                                              ('swimmer', 3, (128, 128), (32, 32), 2), ('humanoid', 2, (128, 128), (20, 10, 5), 2),
                                              ('humanoid', 2, (128, 128), (100, 50, 25), 2)])
def test_zero_noise_is_the_deterministic_gradient(env, K, dh, ph, path):
    """fmaf(0, std, mean) == mean and the log_std sum is of exact zeros: bitwise the 'bptt' gradient."""
    eng, dm, pdims, pool, rng = setup(env, K, dh, ph, seed=113, scale=0.05)
    select(eng, path)
    B, T = (100, 10) if env == 'swimmer' else (40, 5)
    x0 = x0_for(env, pool, B)
    c0, g0 = eng.bptt_grad(x0, T, 0.99)
    c1, g1 = eng.bptt_grad_stochastic(x0, T, 0.99, noise=np.zeros((K, T, B, dm.na), np.float32))
    assert torch.equal(c0, c1)
    assert torch.equal(g0[:-dm.na], g1[:-dm.na])
    assert torch.all(g1[-dm.na:] == 0)


def test_production_draws_reproducible_family_independent_and_restated():
    eng, dm, pdims, pool, rng = setup('swimmer', 5, (64, 64), (32, 32), seed=114)
    B, T, gamma = 150, 12, 0.99
    x0 = x0_for('swimmer', pool, B)
    assert eng.set_det_path(True) == 1
    c1, g1, n1 = eng.bptt_grad_stochastic(x0, T, gamma, seed=77, n_saturates=True)
    c2, g2, n2 = eng.bptt_grad_stochastic(x0, T, gamma, seed=77, n_saturates=True)
    assert torch.equal(c1, c2) and torch.equal(g1, g2) and torch.equal(n1, n2)
    c3, g3 = eng.bptt_grad_stochastic(x0, T, gamma, seed=78)
    assert not torch.equal(c1, c3) and not torch.equal(g1, g3)
    # the same draws on the generic sweeps
    assert eng.set_det_path(False) == 0
    cg, gg = eng.bptt_grad_stochastic(x0, T, gamma, seed=77)
    eng.set_det_path(True)
    np.testing.assert_allclose(cpu(cg), cpu(c1), rtol=1e-5, atol=1e-6)
    assert rel_l2(cpu(gg), cpu(g1)) < TOL.BPTT_GRAD_REL_L2
    # the documented counter mapping, restated in NumPy, fed back through parity mode
    eps = R.bptt_noise(77, 5, T, B, dm.na)
    cp, gp = eng.bptt_grad_stochastic(x0, T, gamma, noise=eps.astype(np.float32))
    np.testing.assert_allclose(cpu(cp), cpu(c1), rtol=1e-5, atol=1e-6)
    assert rel_l2(cpu(gp), cpu(g1)) < 1e-5


def test_production_draws_agree_between_gemm_path_and_generic():
    eng, dm, pdims, pool, rng = setup('swimmer', 2, (128, 128), (32, 32), seed=115)
    B, T = 70, 6
    x0 = x0_for('swimmer', pool, B)
    assert eng.set_det_path(True) == 2
    c1, g1 = eng.bptt_grad_stochastic(x0, T, 1.0, seed=5)
    assert eng.set_det_path(False) == 0
    c2, g2 = eng.bptt_grad_stochastic(x0, T, 1.0, seed=5)
    eng.set_det_path(True)
    np.testing.assert_allclose(cpu(c1), cpu(c2), rtol=1e-5, atol=1e-6)
    assert rel_l2(cpu(g1), cpu(g2)) < TOL.BPTT_GRAD_REL_L2
    eps = R.bptt_noise(5, 2, T, B, dm.na)
    cp, gp = eng.bptt_grad_stochastic(x0, T, 1.0, noise=eps.astype(np.float32))
    np.testing.assert_allclose(cpu(cp), cpu(c1), rtol=1e-5, atol=1e-6)


def test_production_draws_on_the_mfma3_pre_step_match_the_restatement():
    """na = 21: six Philox chunks per (i, t, b), drawn by lanes (cb, q) as chunk 4 cb + q in k_dg_pre_mfma3."""
    eng, dm, pdims, pool, rng = setup('humanoid', 2, (128, 128), (100, 50, 25), seed=117, scale=0.05)
    B, T = 40, 4
    x0 = x0_for('humanoid', pool, B)
    select(eng, 2)
    c1, g1, n1 = eng.bptt_grad_stochastic(x0, T, 1.0, seed=11, n_saturates=True)
    eps = R.bptt_noise(11, 2, T, B, dm.na)
    cp, gp, np_ = eng.bptt_grad_stochastic(x0, T, 1.0, noise=eps.astype(np.float32), n_saturates=True)
    np.testing.assert_allclose(cpu(cp), cpu(c1), rtol=1e-5, atol=1e-6)
    assert rel_l2(cpu(gp), cpu(g1)) < 1e-5
    assert np.abs(cpu(n1) - cpu(np_)).sum() <= 1
    check_parity(eng, dm, pdims, 'humanoid', x0, T, 1.0, eps)


def test_stochastic_training_loop_follows_the_restatement_and_trains_log_std():
    import metrpo_amd
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 3, (32, 32), (16, 16), seed=116)
    T, gamma, lr, clip, B, seed = 12, 1.0, 2e-2, 1.0, 96, 9
    opt = metrpo_amd.BPTT(eng, T=T, gamma=gamma, learning_rate=lr, grad_norm_clipping=clip, batch_size=B, stochastic=True, seed=seed)
    th = cpu(eng.get_policy()).astype(np.float64)
    ls0 = th[-dm.na:].copy()
    adam = Bp.PolicyAdam(th.size)
    dm32 = dm.astype(np.float32).astype(np.float64)
    for it in range(5):
        xb = pool[it * 16:it * 16 + B].astype(np.float32)
        cost = float(opt.step(xb))
        eps = f32(R.bptt_noise(seed * 1000003 + it, 3, T, B, dm.na))       # the running per-object key
        rc, rg, _ = R.stochastic_costs_and_grad(dm32, th, pdims, 'swimmer', xb.astype(np.float64), T, gamma, eps)
        assert abs(cost - rc.mean()) < 2e-4 * max(1.0, abs(rc.mean()))
        th = adam.step(th, rg, pdims, lr=lr, clip_val=clip)
    got = cpu(eng.get_policy())
    np.testing.assert_allclose(got, th, rtol=2e-3, atol=2e-4)
    assert np.all(np.abs(got[-dm.na:] - ls0) > 1e-3)                # log_std is trained
    assert opt.n_saturates is not None and tuple(opt.n_saturates.shape) == (B, dm.na)


def test_bptt_stochastic_params_file_runs_the_early_stopping_driver():
    import metrpo_amd
    from metrpo_amd import early_stop
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    p['algo'] = 'bptt-stochastic'
    p['n_models'] = 2
    p['dynamics_model']['hidden_layers'] = [64, 64]
    po = p['policy_opt_params']
    po.update(T=10, batch_size=64, log_every=2, max_iters=6, num_iters_threshold=4)
    po['trpo']['batch_size'] = 1000
    s = metrpo_amd.from_params(p, seed=3)
    assert s.bptt is not None and s.bptt.stochastic and s.bptt_optimize_policy_kwargs is not None
    assert 'reset_log_std' not in s.bptt_optimize_policy_kwargs
    dm, _, _, pool = O.make_problem('swimmer', K=2, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=4)
    s.engine.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    out = early_stop.optimize_policy(s.bptt, pool[:50].astype(np.float32), **s.bptt_optimize_policy_kwargs)
    assert out['last_index'] >= 2 and len(out['training_costs']) == out['last_index']
    assert np.all(np.isfinite(out['training_costs'])) and np.all(np.isfinite(out['min_validation_costs']['estimated']))
    assert np.all(np.isfinite(cpu(s.engine.get_policy())))


def test_error_statuses():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    eng = metrpo_amd.Engine('swimmer', 2, (16, 16), (8, 8))
    x0 = torch.zeros((4, 10), dtype=torch.float32, device=eng.device)
    g = torch.empty(eng.P, dtype=torch.float64, device=eng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda init, T: lib.metrpo_bptt_grad_stochastic(eng._ctx, init, 4, T, 1.0, None, 1, None, p(g), None, eng._stream())
    assert call(p(x0), 5) == -5                                      # METRPO_ESTATE: no dynamics yet
    dm, theta, _, _ = O.make_problem('swimmer', K=2, dyn_hidden=(16, 16), pol_hidden=(8, 8), seed=1)
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    assert call(p(x0), 5) == -5                                      # no policy yet
    eng.set_policy(theta)
    assert call(None, 5) == -2                                       # METRPO_ENULL
    assert call(p(x0), 0) == -1 and call(p(x0), -3) == -1            # METRPO_EINVAL
    assert call(p(x0), 5) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.bptt_grad_stochastic(x0, 5, 1.0)                         # neither draws nor seed
