"""The NumPy restatement of L-BFGS-B (tests/lbfgs_ref.py) against the local scipy's minimize(method='L-BFGS-B', jac=True): the wrapper
of the same L-BFGS-B 3.0 that the reference's scipy 0.19 wraps.  Evaluation points agree to 1e-12 relative while the two runs are in
step; on long Rosenbrock runs the last-bit differences of the direction (the two-loop recursion here, L-BFGS-B's compact form there) grow
along the curved valley, so those runs are pinned on a prefix and on their outcome."""
import numpy as np
import pytest

import lbfgs_ref as L

so = pytest.importorskip('scipy.optimize')


def scipy_run(fg, x0, **o):
    xs = []

    def f(x):
        xs.append(np.array(x, dtype=np.float64))
        return fg(x)
    opts = dict(maxcor=o.get('m', 10), maxls=o.get('maxls', 20), maxiter=o.get('maxiter', 15000), maxfun=o.get('maxfun', 15000),
                ftol=o.get('ftol', L.DEFAULTS['ftol']), gtol=o.get('gtol', 1e-5))
    return so.minimize(f, x0, jac=True, method='L-BFGS-B', options=opts), xs


def rosen(x):
    return so.rosen(x), so.rosen_der(x)


def quadratic(n, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)); A = A @ A.T / n + np.eye(n)
    b = rng.standard_normal(n)
    return lambda x: (0.5 * x @ A @ x - b @ x, A @ x - b), A, b


def compare(fg, x0, prefix=None, outcome=True, **o):
    r, xs = scipy_run(fg, x0, **o)
    q = L.minimize(fg, x0, **o)
    k = len(xs) if prefix is None else prefix
    assert len(q.xs) >= min(k, len(xs))
    for a, b in zip(xs[:k], q.xs[:k]):
        assert np.max(np.abs(a - b)) <= 1e-12 * max(np.max(np.abs(a)), 1e-300)
    if outcome:
        assert (q.nit, q.nfev, q.status, q.message) == (r.nit, r.nfev, r.status, r.message)
    return r, q


@pytest.mark.parametrize('n,prefix', [(2, 14), (10, 30), (100, 12)])
def test_rosenbrock(n, prefix):
    x0 = np.tile([-1.2, 1.0], n // 2)
    r, q = compare(rosen, x0, prefix=prefix, outcome=(n < 100))
    assert q.status == 0 and r.status == 0 and q.message == r.message
    np.testing.assert_allclose(q.x, np.ones(n), atol=1e-4)


def test_spd_quadratic_1000():
    fg, A, b = quadratic(1000)
    r, q = compare(fg, np.zeros(1000), prefix=14)
    assert q.task == L.CONV_F
    assert len(q.xs) == r.nfev


def test_stationary_start():
    fg, A, b = quadratic(50, seed=2)
    r, q = compare(fg, np.linalg.solve(A, b))
    assert q.task == L.CONV_PG and q.nit == 0 and q.nfev == 1


@pytest.mark.parametrize('opts,task', [(dict(maxiter=7), L.STOP_ITER), (dict(maxfun=9), L.STOP_FUN), (dict(maxfun=4), L.STOP_FUN),
                                       (dict(maxls=1), None)])
def test_limits(opts, task):
    r, q = compare(rosen, np.tile([-1.2, 1.0], 5), **opts)
    if task is not None:
        assert q.task == task and q.status == 1
    if opts.get('maxfun') == 4:
        assert q.nfev > 4                       # passed inside a line search, noticed at the next iterate


def test_every_maxfun_limit_agrees():
    for mf in range(1, 30):
        compare(rosen, np.tile([-1.2, 1.0], 5), maxfun=mf)


def test_restart_at_col_gt_0_then_abnormal_at_col_0():
    """a constant gradient bias from evaluation k on: the search fails with stored pairs (restart), then with none (ABNORMAL)."""
    def make():
        calls = [0]

        def fg(x):
            calls[0] += 1
            f, g = rosen(x)
            return f, (g + 50.0) if calls[0] > 6 else g
        return fg
    x0 = np.tile([-1.2, 1.0], 5)
    r, xs = scipy_run(make(), x0)
    q = L.minimize(make(), x0)
    assert (q.nit, q.nfev, q.status, q.message) == (r.nit, r.nfev, r.status, r.message)
    for a, b in zip(xs, q.xs):
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(a))


def test_abnormal_with_no_stored_pair():
    fg = lambda x: (float(x @ x), -2.0 * x)       # the gradient points uphill: every search fails
    r, q = compare(fg, np.ones(5))
    assert q.task == L.ABNORMAL and q.status == 2 and q.message == 'ABNORMAL: '


def test_bptt_oracle_objective_in_float32_as_tf_hands_it():
    """the reference's setting: f and g the float32 loss and gradient, x fed to the float32 variables."""
    from oracle import bptt_oracle as Bp
    from oracle import metrpo_oracle as O
    env = 'swimmer'
    dm, theta, pdims, pool = O.make_problem(env, K=2, dyn_hidden=(8, 8), pol_hidden=(4, 4), seed=0, n_pool=16)
    x0 = pool[:6].astype(np.float32).astype(np.float64)

    def fg(x):
        th = np.asarray(x).astype(np.float32).astype(np.float64)
        c, g = Bp.policy_costs_and_grad(dm, th, pdims, env, x0, 3, 1.0)
        return float(np.float32(np.mean(c))), g.astype(np.float32).astype(np.float64)
    r, q = compare(fg, np.asarray(theta, dtype=np.float64), maxiter=15)
    assert q.fun <= fg(theta)[0]
