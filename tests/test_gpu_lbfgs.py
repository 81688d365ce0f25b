"""The 'l-bfgs' policy update on the GPU (csrc/lbfgs.hip): the reverse-communication core against the NumPy restatement tests/lbfgs_ref.py
(itself pinned against scipy in tests/test_lbfgs_ref.py), the BPTT-driven minimisation against a host-driven loop, against the oracle, and
inside early_stop.optimize_policy.  All calls go through the C ABI."""
import numpy as np
import pytest
import torch

import helpers as Hh
import lbfgs_ref as L
import tolerances as TOL
from oracle import bptt_oracle as Bp

pytestmark = pytest.mark.gpu


def cpu(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def core_engine():
    import metrpo_amd
    return metrpo_amd.Engine('swimmer', 2, (16, 16), (8, 8))


def device_run(eng, fg, x0, **o):
    """the device core driven like scipy's wrapper; fg(x: device float64 tensor) -> (f, g) device float64 tensors."""
    opts = dict(L.DEFAULTS); opts.update(o)
    x = eng.lbfgs_begin(torch.as_tensor(x0, dtype=torch.float64, device='cuda'), eng.lbfgs_opts(**opts))
    xs, last, f, g = [], None, None, None
    while True:
        xh = x.clone()
        if last is None or not torch.equal(xh, last):
            f, g = fg(xh)
            last = xh
            xs.append(cpu(xh))
        x, task = eng.lbfgs_iterate(f, g)
        if tuple(cpu(task).tolist()) != L.FG:
            break
    r = eng.lbfgs_result()
    r['xs'], r['x'] = xs, cpu(x)
    return r


def ref_run(fg, x0, **o):
    def fgn(x):
        f, g = fg(torch.as_tensor(x, device='cuda'))
        return float(f.item()), cpu(g)
    return L.minimize(fgn, x0, **o)


def rosen(x):
    f = torch.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)
    g = torch.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f.reshape(1), g


def spd_quadratic(n, seed=0):
    rng = np.random.RandomState(seed)
    if n <= 64:
        A = rng.randn(n, n); A = A @ A.T / n + np.eye(n)
        A = torch.as_tensor(A, device='cuda')
        mv = lambda x: A @ x
    else:                                                     # diagonal-plus-low-rank at large n
        dg = torch.as_tensor(1.0 + 9.0 * rng.rand(n), device='cuda')
        U = torch.as_tensor(rng.randn(n, 4) / np.sqrt(n), device='cuda')
        mv = lambda x: dg * x + U @ (U.T @ x)
    b = torch.as_tensor(rng.randn(n), device='cuda')

    def fg(x):
        Ax = mv(x)
        return (0.5 * torch.dot(x, Ax) - torch.dot(b, x)).reshape(1), Ax - b
    return fg


def check_same_run(d, r, k=25, tol=1e-10, counts=True):
    for a, b in zip(d['xs'][:k], r.xs[:k]):
        assert rel(a, b) < tol, rel(a, b)
    if counts:
        assert (d['nit'], d['nfev'], d['task'], d['status']) == (r.nit, r.nfev, r.task, r.status)


def test_rosenbrock_100_first_evaluations_match_the_restatement():
    eng = core_engine()
    x0 = np.tile([-1.2, 1.0], 50)
    d, r = device_run(eng, rosen, x0, maxiter=40), ref_run(rosen, x0, maxiter=40)
    assert len(d['xs']) >= 25
    check_same_run(d, r, counts=False)


@pytest.mark.parametrize('n', [3, 12500])
def test_spd_quadratic_matches_the_restatement(n):
    eng = core_engine()
    fg = spd_quadratic(n)
    x0 = np.zeros(n)
    d, r = device_run(eng, fg, x0), ref_run(fg, x0)
    assert r.task[0] == 4
    check_same_run(d, r)


def biased(fg, k, bias):
    """a stateful objective whose gradient gets a constant bias from evaluation k on (forces a line-search failure at col > 0)."""
    calls = [0]

    def f(x):
        calls[0] += 1
        fv, g = fg(x)
        return fv, (g + bias) if calls[0] > k else g
    return f


@pytest.mark.parametrize('case', ['stationary', 'rel_reduction', 'maxiter', 'maxfun', 'maxfun_in_search', 'maxls1', 'restart',
                                  'abnormal'])
def test_every_stopping_path_gives_the_restatement_task(case):
    eng = core_engine()
    x10 = np.tile([-1.2, 1.0], 5)
    quad = spd_quadratic(30, seed=0)
    if case == 'stationary':
        fg, x0, o = (lambda x: (torch.dot(x, x).reshape(1) * 0.5, x)), np.zeros(7), {}
    elif case == 'rel_reduction':
        fg, x0, o = quad, np.ones(30), {}
    elif case == 'maxiter':
        fg, x0, o = rosen, x10, dict(maxiter=7)
    elif case == 'maxfun':
        fg, x0, o = rosen, x10, dict(maxfun=9)
    elif case == 'maxfun_in_search':
        fg, x0, o = rosen, x10, dict(maxfun=4)
    elif case == 'maxls1':
        fg, x0, o = rosen, x10, dict(maxls=1)
    elif case == 'restart':
        fg, x0, o = None, x10, {}
    else:
        fg, x0, o = (lambda x: (torch.dot(x, x).reshape(1), -2.0 * x)), np.ones(5), dict(maxls=2)
    if case == 'restart':
        bias = torch.full((10,), 50.0, dtype=torch.float64, device='cuda')
        d, r = device_run(eng, biased(rosen, 6, bias), x0, **o), ref_run(biased(rosen, 6, bias), x0, **o)
    else:
        d, r = device_run(eng, fg, x0, **o), ref_run(fg, x0, **o)
    expect = dict(stationary=L.CONV_PG, rel_reduction=L.CONV_F, maxiter=L.STOP_ITER, maxfun=L.STOP_FUN, maxfun_in_search=L.STOP_FUN,
                  abnormal=L.ABNORMAL).get(case)
    if expect is not None:
        assert r.task == expect
    if case == 'maxfun_in_search':
        assert r.nfev > 4                                   # the limit passed inside a line search, noticed at the new iterate
    check_same_run(d, r)
    np.testing.assert_allclose(d['x'], r.x, rtol=1e-10, atol=1e-12)


# ---- the policy driver
SHAPES = [('swimmer', 3, (24, 16), (8, 8), 40, 6, 0.97, False),         # generic sweeps
          ('swimmer', 5, (64, 64), (32, 32), 60, 8, 1.0, True),         # MFMA 2x64
          ('half_cheetah', 2, (32, 32), (32, 32), 40, 6, 0.99, True),   # MFMA 2x32
          ('swimmer', 3, (128, 128), (32, 32), 50, 5, 1.0, True)]       # GEMM path


def policy_setup(env, K, dh, ph, B, generic, seed=7):
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, ph, seed=seed)
    rng = np.random.RandomState(3)
    theta = theta + 0.1 * rng.randn(theta.size)
    theta[-dm.na:] = -0.3                                        # log_std: in var_list, gradient 0
    eng.set_policy(theta)
    eng.set_det_path(not generic)
    x0 = pool[:B].astype(np.float32)
    return eng, dm, pdims, x0


def host_fg(eng, x0, T, gamma):
    """TF's float32 loss and gradient at theta = float32(x), cast to float64 (ScipyOptimizerInterface)."""
    def fg(x):
        eng.set_policy(np.asarray(x).astype(np.float32))
        costs, grad = eng.bptt_grad(x0, T, gamma)
        c = cpu(costs)
        f = 0.0
        for v in c.tolist():
            f += v
        return float(np.float32(f / len(c))), cpu(grad).astype(np.float32).astype(np.float64)
    return fg


@pytest.mark.parametrize('env,K,dh,ph,B,T,gamma,fast', SHAPES)
def test_policy_driver_matches_the_host_driven_loop(env, K, dh, ph, B, T, gamma, fast):
    eng, dm, pdims, x0 = policy_setup(env, K, dh, ph, B, not fast)
    th0 = cpu(eng.get_policy())
    adam0 = [cpu(a) if torch.is_tensor(a) else a for a in eng.get_policy_adam()]
    # the host-driven restatement, evaluating through engine.bptt_grad
    r = L.minimize(host_fg(eng, x0, T, gamma), th0.astype(np.float64), maxiter=12)
    # the device core, driven step by step from the host on the same evaluations
    eng.set_policy(th0)
    fg = host_fg(eng, x0, T, gamma)
    dev = device_run(eng, lambda x: tuple(torch.as_tensor(v, dtype=torch.float64, device='cuda').reshape(-1) for v in fg(cpu(x))), th0.astype(np.float64),
                     maxiter=12)
    for a, b in zip(dev['xs'][:10], r.xs[:10]):
        assert np.array_equal(a.astype(np.float32), b.astype(np.float32))
        assert rel(a, b) < 1e-12
    assert (dev['nit'], dev['nfev'], dev['task']) == (r.nit, r.nfev, r.task)
    # the driver: one call, the task words read from the device
    eng.set_policy(th0)
    out = eng.lbfgs_policy(x0, T, gamma, eng.lbfgs_opts(maxiter=12))
    assert (out['nit'], out['nfev'], out['task'], out['status']) == (r.nit, r.nfev, r.task, r.status)
    th = cpu(eng.get_policy())
    assert np.array_equal(th, r.x.astype(np.float32))
    assert out['fun'] == r.fun
    assert np.array_equal(th[-dm.na:], th0[-dm.na:])
    adam1 = [cpu(a) if torch.is_tensor(a) else a for a in eng.get_policy_adam()]
    for a, b in zip(adam0, adam1):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # against the oracle: the cost went down, and fun is the float64 cost at the final theta
    oc0, _ = Bp.policy_costs_and_grad(dm.astype(np.float32).astype(np.float64), th0.astype(np.float64), pdims, env, x0.astype(np.float64), T, gamma)
    oc, _ = Bp.policy_costs_and_grad(dm.astype(np.float32).astype(np.float64), th.astype(np.float64), pdims, env, x0.astype(np.float64), T, gamma)
    assert out['fun'] <= float(np.mean(oc0)) * (1 + 1e-6) + 1e-7
    np.testing.assert_allclose(out['fun'], np.mean(oc), **TOL.BPTT_COST)


def test_lookahead_does_not_change_the_result():
    env, K, dh, ph, B, T, gamma, fast = SHAPES[1]
    eng, dm, pdims, x0 = policy_setup(env, K, dh, ph, B, not fast)
    th0 = cpu(eng.get_policy())
    outs, ths = [], []
    for la in (1, 4):
        eng.set_policy(th0)
        outs.append(eng.lbfgs_policy(x0, T, gamma, eng.lbfgs_opts(maxiter=15, lookahead=la)))
        ths.append(cpu(eng.get_policy()))
    assert outs[0] == outs[1]
    assert np.array_equal(ths[0], ths[1])


class Pool(object):
    def __init__(self, states):
        self.states = states

    def sample(self, n):
        return self.states[:n]


@pytest.mark.parametrize('restore', [False, True])
def test_early_stop_runs_one_minimisation_and_one_validation_round(restore):
    import metrpo_amd
    from metrpo_amd import early_stop as E
    env, K, dh, ph, B, T, gamma, fast = SHAPES[1]
    eng, dm, pdims, x0 = policy_setup(env, K, dh, ph, B, not fast)
    th0 = cpu(eng.get_policy())
    val = x0[:20] * 1.1
    lb = metrpo_amd.LBFGS(eng, T, gamma, batch_size=B, maxiter=6)
    est0 = cpu(eng.validation_cost(val, T, gamma))
    stop_fn = (lambda old, new, mode='vector': True) if restore else E.stop_critereon(0.10, 1e-5, 0.30)
    out = E.optimize_policy(lb, val, T, gamma, mode='estimated', stop_fn=stop_fn, init_pool=Pool(x0), max_iters=50, log_every=5)
    assert out['last_index'] == 1 and len(out['training_costs']) == 1 and len(out['history']) == 1
    assert lb.result['nit'] <= 6
    # the decision: is_done on the logged costs, replayed
    eng.set_policy(th0)
    lb2 = metrpo_amd.LBFGS(eng, T, gamma, batch_size=B, maxiter=6)
    lb2.minimize(x0)
    th1 = cpu(eng.get_policy())
    est1 = cpu(eng.validation_cost(val, T, gamma))
    done = E.is_done('estimated', stop_fn, {'real': 0.0, 'trpo_mean': np.inf, 'estimated': est0},
                     {'trpo_mean': 0.0, 'estimated': est1, 'real': 0.0})
    assert done == restore
    eng.set_policy(th0)
    out = E.optimize_policy(lb, val, T, gamma, mode='estimated', stop_fn=stop_fn, init_pool=Pool(x0))
    th = cpu(eng.get_policy())
    assert np.array_equal(th, th0 if done else th1)
    assert out['best_index'] == (0 if done else 1)
