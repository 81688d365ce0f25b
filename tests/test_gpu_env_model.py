"""The environments' reward model (csrc/env_model.h) on its own, through the diagnostics hook Engine.debug_env_model: env_cost, env_done, the adjoint
d(w cost)/dx_next of every dimension and d(w cost)/du, for all six environments at their ENV_SPECS shapes, once with the environment passed at run time (the
generic kernels' form) and once through the instantiation compiled for it (the five 2 x 64 environments), against oracle.metrpo_oracle.cost_np_vec, is_done
and oracle.bptt_oracle._cost_grads in float64.

N = 64 rows of float32 values per environment stand on every branch: Hopper x0 on both sides of 0.45, x1 beyond +-0.2 and inside, every one of dims 2.. at
+-50 and +-150 (dim 5, which also carries the reward, among them) and rows with all of them exactly +-100 (the bound itself: no penalty); half-cheetah with
the clipped quantity below, inside and above [-10, 10] and exactly -10 and 10 (the gate is inclusive); Ant's z below, inside, exactly on (1.0) and above its
range, one row with a NaN (in the reward's own dimension: its cost is NaN, the row counts for `done` only) and one with an inf elsewhere at z = 0.6; uniform
rows for the other three.  Every row is 1e-3 or more off a kink unless the bound is a float32 number (10, 1.0, 100), so float32 and float64 take the same
branch, which build() asserts on the oracle's own float32 evaluation.

done equals the oracle exactly.  Cost and adjoints: |got - ref| <= 4 e32 + ulp32(|ref|) per cell, e32 the largest error over the array of the oracle
evaluated in float32 against itself in float64 on the same rows: the device's fmaf chain and summation order differ from NumPy's by a few roundings.  On these
rows e32 is 2.3e-5 for Hopper's cost (values up to 355: the bound is 9.0e-5 + ulp = 1.2e-4 there), 1.3e-6 for the humanoid's cost (values up to 11.4: bound
6.3e-6) and at most 4.8e-7 for every other array (bound 1.9e-6 + ulp); the kernels use up to a quarter of it.  The row form
of the state adjoint (env_cost_dx_row into zeros) equals the per-dimension form bit for bit.  pytest -s prints the figures."""
import numpy as np
import pytest
import torch
import helpers as Hh
from oracle import metrpo_oracle as O
from oracle import bptt_oracle as BO

pytestmark = pytest.mark.gpu

N = 64
COMPILED = ('swimmer', 'half_cheetah', 'ant', 'hopper', 'snake')
CASES = [(env, False) for env in sorted(O.ENV_SPECS)] + [(env, True) for env in COMPILED]


def rows(env):
    """-> x_next [N][ns], u [N][na], w [N], float32"""
    ns, na, _ = O.ENV_SPECS[env]
    rng = np.random.RandomState(sorted(O.ENV_SPECS).index(env))
    x = rng.uniform(-2.0, 2.0, (N, ns)).astype(np.float32)
    u = rng.uniform(-1.0, 1.0, (N, na)).astype(np.float32)
    w = (rng.uniform(0.1, 1.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    r = np.arange(N)
    if env == 'hopper':
        x[:, 0] = np.float32([0.25, 0.65])[r & 1]
        x[:, 1] = np.float32([0.1, -0.1, 0.5, -0.5])[(r >> 1) & 3]
        for j in range(2, ns):
            x[:, j] = np.float32([50.0, -50.0, 150.0, -150.0])[(r // 8 + j) & 3]
        x[60:, 2:] = np.float32([100.0, -100.0])[(r[60:, None] + np.arange(2, ns)[None]) & 1]
        assert set(np.abs(x[:60, 5])) == {50.0, 150.0}
    elif env == 'half_cheetah':
        x[:, 9] = np.float32([-12.0, 0.0, 12.0])[r % 3]
        u[62:] = 0.0
        x[62:, 9] = np.float32([10.0, -10.0])
    elif env == 'ant':
        x[:, 2] = np.float32([0.1, 0.6, 1.0, 1.2])[r & 3]
        x[61, 15] = np.nan                  # z = 0.6 on rows 61 and 57
        x[57, 20] = np.inf
    return x, u, w


def oracle(env, x, u, w):
    gu, gx = BO._cost_grads(env, u, x, w)
    with np.errstate(invalid='ignore'):
        return dict(cost=O.cost_np_vec(env, x, u, x), done=np.asarray(O.is_done(env, x, x), bool), gx=gx, gu=gu)


def build(env):
    x, u, w = rows(env)
    r64 = oracle(env, x.astype(np.float64), u.astype(np.float64), w.astype(np.float64))
    r32 = oracle(env, x, u, w)
    assert all(r32[k].dtype == np.float32 for k in ('cost', 'gx', 'gu'))
    assert np.array_equal(r32['done'], r64['done'])
    fin = np.isfinite(r64['cost'])
    # same branch in both precisions: a gate or bound term present in one is present in the other
    assert np.array_equal(r32['gx'][fin] == 0, r64['gx'][fin] == 0) and np.array_equal(r32['gu'][fin] == 0, r64['gu'][fin] == 0)
    return x, u, w, r32, r64, fin


REF = {}


def ref(env):
    if env not in REF:
        REF[env] = build(env)
    return REF[env]


@pytest.fixture(scope='module')
def eng():
    return Hh.make_engine('swimmer', 3, (64, 64), (32, 32), seed=3)[0]


def test_rows_stand_on_every_branch():
    x, u, w, r32, r64, fin = ref('hopper')
    assert (0.45 - x[:, 0] > 0).any() and (0.45 - x[:, 0] < 0).any() and (np.abs(x[:, 1]) > 0.2).any() and (np.abs(x[:, 1]) < 0.2).any()
    assert (x[:, 2:] > 100).any(0).all() and (x[:, 2:] < -100).any(0).all() and (np.abs(x[:, 2:]) < 100).any(0).all() and (np.abs(x[60:, 2:]) == 100).all()
    x, u, w, r32, r64, fin = ref('half_cheetah')
    inner = x[:, 9].astype(np.float64) - 0.05 * np.sum(np.square(u.astype(np.float64)), axis=1)
    assert (inner < -10).any() and (inner > 10).any() and (np.abs(inner) < 10).any() and set(inner[62:]) == {10.0, -10.0}
    assert np.all(r64['gx'][62:, 9] == -w[62:])
    x, u, w, r32, r64, fin = ref('ant')
    assert set(x[:, 2]) == set(np.float32([0.1, 0.6, 1.0, 1.2])) and x[57, 2] == x[61, 2] == np.float32(0.6)
    assert not fin[61] and fin.sum() == N - 1 and r64['done'][57] and r64['done'][61] and not r64['done'][1]
    assert r64['done'].sum() == 32 + 2 and not r64['done'][2]            # z = 1.0 is inside


@pytest.mark.parametrize('env,compiled', CASES, ids=['%s-%s' % (e, 'compiled' if c else 'runtime') for e, c in CASES])
def test_env_model(eng, env, compiled):
    x, u, w, r32, r64, fin = ref(env)
    out = eng.debug_env_model(env, *(torch.from_numpy(a).to(eng.device) for a in (x, u, w)), compile_time=compiled)
    torch.cuda.synchronize()
    got = dict((k, v.cpu().numpy()) for k, v in out.items())
    assert np.array_equal(got['done'] != 0, r64['done'])
    assert np.array_equal(got['gx_row'], got['gx'])
    for k in ('cost', 'gx', 'gu'):
        e32 = np.max(np.abs(r32[k][fin].astype(np.float64) - r64[k][fin]))
        bound = 4.0 * e32 + np.spacing(np.abs(r64[k][fin]).astype(np.float32)).astype(np.float64)
        err = np.abs(got[k][fin].astype(np.float64) - r64[k][fin])
        print('%s %s %s: e32 %.3g  worst error %.3g  worst share of the bound %.3g' % (env, 'compiled' if compiled else 'runtime', k, e32, err.max(), (err / bound).max()))
        assert np.all(err <= bound), (env, k, err.max())


def test_compiled_form_is_refused_for_the_humanoid(eng):
    from metrpo_amd._lib import MetrpoError
    x, u, w = (torch.from_numpy(a).to(eng.device) for a in rows('humanoid'))
    with pytest.raises(MetrpoError, match='debug_env_model'):
        eng.debug_env_model('humanoid', x, u, w, compile_time=True)
