"""Case table, recorded-rollout generator, kink guard and bound arithmetic of the 'svg' tests (tests/test_svg_cases.py on the CPU,
tests/test_gpu_svg.py on the device).  TEST INFRASTRUCTURE ONLY.

A case is (env, ensemble and policy shape, n rollouts padded to T with ragged lengths, gamma, head, Jacobian path, chunk).  Its rollouts are
"recorded": states from the init pool pushed through head `model` under the policy mean plus noise (actions unclipped, some beyond +-1; the
output bias of action 0 is raised so that its mean sits beyond the clip bound, where a wrongly applied clip gate shows), plus observation noise,
rounded to float32 -- the device's storage type -- so the bounds cover arithmetic only.

Kink guard: a rollout enters a case only if the float32 and the float64 restatement take the same branch at every relu of the head and at every
cost kink, with the float64 argument at least KINK_FACTOR x their difference away from the kink.  A rollout that fails is redrawn; at most
MAX_REPLACED of a case's rollouts may be (so none, at n <= 5: the seeds below need no redraw, which tests/test_svg_cases.py checks)."""
import functools
from collections import namedtuple

import numpy as np
from oracle import metrpo_oracle as O
import svg_ref as R
import tolerances as TOL
from helpers import problem_data

KINK_FACTOR = 16.0
MAX_REPLACED = 0.05

Case = namedtuple('Case', 'id env K dh ph act n T gamma model path chunk seed')
# path: what the call asks for ('auto', 'generic', 'gemm'); want: what metrpo_last_svg_path must report


def gemm_applicable(c):
    ns = O.ENV_SPECS[c.env][0]
    return c.act == 'relu' and len(c.dh) >= 1 and min(c.dh) >= 16 and ns <= 64


def want_path(c):
    return c.path if c.path != 'auto' else ('gemm' if gemm_applicable(c) else 'generic')


def lengths_of(n, T):
    """(T, T-1, 1, T, T-1, 1, ...) clamped into [1, T]"""
    return np.array([max(1, (T, T - 1, 1)[r % 3]) for r in range(n)], dtype=np.int32)


def _mk():
    cases = []

    def add(env, K, dh, ph, n, T, gamma=1.0, model=0, paths=('generic', 'gemm'), chunk=0, act='relu', seed=7):
        for p in paths:
            cid = '%s-%s-%s-%s-n%dT%d-g%g-m%d-%s-c%d' % (env, 'x'.join(map(str, dh)), 'x'.join(map(str, ph)), act, n, T, gamma, model, p, chunk)
            cases.append(Case(cid, env, K, tuple(dh), tuple(ph), act, n, T, gamma, model, p, chunk, seed))
    # n x T x gamma x head on the 2 x 64 class, both paths
    add('swimmer', 3, (64, 64), (32, 32), 1, 1)
    add('swimmer', 3, (64, 64), (32, 32), 3, 2, 0.97, 2)
    add('swimmer', 3, (64, 64), (32, 32), 5, 11, 0.97, 0)
    add('swimmer', 3, (64, 64), (32, 32), 3, 11, 1.0, 2)
    add('swimmer', 3, (64, 64), (32, 32), 1, 11, 0.97, 2)
    add('swimmer', 3, (64, 64), (32, 32), 5, 1, 1.0, 0)
    # both paths forced on the other widths; every env but Ant
    add('half_cheetah', 2, (128, 128), (32, 32), 3, 11, 0.97, 1)
    add('hopper', 2, (24, 16), (32, 32), 3, 11, 0.97, 1)
    add('snake', 2, (48, 48, 32), (32, 32), 5, 2, 1.0, 0)
    add('humanoid', 2, (64, 64), (100, 50, 25), 3, 2, 0.97, 1)
    add('snake', 2, (32,), (16,), 3, 2, 1.0, 1)                  # one hidden layer: the seed feeds the input layer's product directly
    # generic by auto: a hidden layer below 16 units, tanh layers, humanoid's 100-50-25 policy on a narrow head
    add('swimmer', 2, (8, 8), (32, 32), 3, 11, 0.97, 1, paths=('auto',))
    add('hopper', 2, (32, 32), (32, 32), 3, 11, 0.97, 0, paths=('auto',), act='tanh')
    add('humanoid', 2, (8, 8), (100, 50, 25), 3, 2, 0.97, 0, paths=('auto',))
    # GEMM by auto
    add('half_cheetah', 2, (64, 64), (32, 32), 3, 2, 1.0, 1, paths=('auto',))
    # N = n T at the GEMM row-tile edges 63, 64, 65, 129
    add('swimmer', 2, (64, 64), (32, 32), 1, 63, 0.97, 0)
    add('swimmer', 2, (64, 64), (32, 32), 1, 64, 0.97, 1)
    add('swimmer', 2, (64, 64), (32, 32), 5, 13, 0.97, 0)
    add('swimmer', 2, (64, 64), (32, 32), 3, 43, 0.97, 1)
    # chunk against N = 33: N = chunk - 1, chunk, chunk + 1, and chunk = 16 (rollout 1 = samples 11 .. 21 straddles the boundary)
    for ch in (34, 33, 32, 16):
        add('swimmer', 2, (64, 64), (32, 32), 3, 11, 0.97, 1, chunk=ch)
    return cases


CASES = _mk()
BY_ID = {c.id: c for c in CASES}


@functools.lru_cache(maxsize=None)
def problem(env, K, dh, ph, act, seed):
    dm, theta, pdims, pool = problem_data(env, K, dh, ph, seed=seed, dyn_act=act)
    Ws, bs, ls = O.policy_unflatten(theta.copy(), pdims)
    bs[-1][0] += 1.3                                             # action 0's mean beyond the clip bound (svg applies NO clip)
    theta = O.policy_flatten(Ws, bs, ls).astype(np.float32).astype(np.float64)
    dm = dm.astype(np.float32).astype(np.float64)
    return dm, theta, pdims, pool


def kink_sites(env, s, a, dtype):
    """arguments of the cost's kinks at (x_next = s, u = a): zero = on the kink"""
    s, a = s.astype(dtype), a.astype(dtype)
    if env == 'half_cheetah':
        inner = s[:, 9] - dtype(1e-1) * dtype(0.5) * np.sum(np.square(a), axis=1)
        return np.stack([inner + 10, 10 - inner], axis=1)
    if env == 'hopper':
        return np.concatenate([(dtype(0.45) - s[:, 0])[:, None], (np.abs(s[:, 1]) - dtype(0.2))[:, None], np.abs(s[:, 2:]) - 100], axis=1)
    return np.ones((s.shape[0], 1), dtype=dtype)


def rollout_margin(dm, env, model, s, a):
    """min over the kink sites of |z64| / |z32 - z64| (inf where the two agree exactly); 0 if a branch differs"""
    sites = []
    if 'relu' in dm.acts:                                         # the pre-activations of the relu layers (tanh and identity have no kink)
        _, z64 = R.dyn_jacobian(dm, model, s, a, np.float64)
        _, z32 = R.dyn_jacobian(dm, model, s, a, np.float32)
        sites += [(p.ravel(), q.ravel().astype(np.float64)) for x, p, q in zip(dm.acts, z64, z32) if x == 'relu']
    sites.append((kink_sites(env, s, a, np.float64).ravel(), kink_sites(env, s, a, np.float32).ravel().astype(np.float64)))
    m = np.inf
    for z64, z32 in sites:
        if np.any((z64 > 0) != (z32 > 0)):
            return 0.0
        d = np.abs(z32 - z64)
        with np.errstate(divide='ignore'):
            m = min(m, float(np.min(np.where(d > 0, np.abs(z64) / np.where(d > 0, d, 1.0), np.inf))))
    return m


def draw_rollout(dm, theta, pdims, pool, model, T, rng):
    """One recorded trajectory: Os [T+1, ns], As [T, na], float32-representable"""
    ns, na = dm.ns, dm.na
    Os, As = np.zeros((T + 1, ns)), np.zeros((T, na))
    s = pool[rng.randint(len(pool))].astype(np.float32).astype(np.float64)
    for t in range(T):
        a = (O.policy_mean(theta, pdims, s[None])[0] + 0.3 * rng.randn(na)).astype(np.float32).astype(np.float64)
        Os[t], As[t] = s, a
        nxt = O.dynamics_forward(dm, model, s[None], np.clip(a, -1, 1)[None])[0] + 0.01 * rng.randn(ns)
        s = nxt.astype(np.float32).astype(np.float64)
    Os[T] = s
    return Os, As


@functools.lru_cache(maxsize=None)
def _case_data(cid):
    c = BY_ID[cid]
    dm, theta, pdims, pool = problem(c.env, c.K, c.dh, c.ph, c.act, c.seed)
    lens = lengths_of(c.n, c.T)
    obs = np.zeros((c.n, c.T + 1, dm.ns)); act = np.zeros((c.n, c.T, dm.na))
    replaced, margin = 0, np.inf
    for r in range(c.n):
        for attempt in range(8):
            rng = np.random.RandomState(c.seed * 100003 + r * 101 + attempt)
            Os, As = draw_rollout(dm, theta, pdims, pool, c.model, c.T, rng)
            m = rollout_margin(dm, c.env, c.model, Os[:lens[r]], As[:lens[r]])
            if m >= KINK_FACTOR:
                break
            replaced += 1
        else:
            raise AssertionError('%s: no rollout clear of the kinks in 8 draws' % cid)
        obs[r], act[r], margin = Os, As, min(margin, m)
    return dict(case=c, dm=dm, theta=theta, pdims=pdims, obs=obs[:, :-1].copy(), obs_next=obs[:, 1:].copy(), Os=obs, act=act, lengths=lens,
                replaced=replaced, margin=margin)


def case_data(case):
    return _case_data(case.id)


@functools.lru_cache(maxsize=None)
def _reference(cid, dtype_name, wrong):
    d = _case_data(cid)
    c = d['case']
    return R.svg_gradient(d['dm'], d['theta'], d['pdims'], c.env, d['obs'], d['act'], d['lengths'], model=c.model, gamma=c.gamma,
                          dtype=np.dtype(dtype_name).type, wrong=wrong, obs_next=d['obs_next'])


def reference(case, dtype=np.float64, wrong=None):
    """the restatement of the case (computed once per (case, dtype, wrong), shared, never written to)"""
    return _reference(case.id, np.dtype(dtype).name, wrong)


def blocks(pdims):
    """(name, slice) of every variable W_l, b_l of the flat policy vector, then log_std"""
    out, o = [], 0
    for l in range(len(pdims) - 1):
        nW = pdims[l] * pdims[l + 1]
        out.append(('W%d' % l, slice(o, o + nW))); o += nW
        out.append(('b%d' % l, slice(o, o + pdims[l + 1]))); o += pdims[l + 1]
    out.append(('log_std', slice(o, o + pdims[-1])))
    return out


def vector_use(g, ref, pdims):
    """(share of GRAD_REL_L2 the whole vector uses, worst share of block_bound over the variables W_l / b_l, its name)"""
    whole = float(np.linalg.norm(g - ref) / np.linalg.norm(ref)) / TOL.GRAD_REL_L2
    worst, where = 0.0, None
    for name, sl in blocks(pdims)[:-1]:
        share = float(np.linalg.norm(g[sl] - ref[sl])) / TOL.block_bound(TOL.GRAD_REL_L2, ref[sl], ref)
        if share > worst:
            worst, where = share, name
    return whole, worst, where


def state_use(g, ref):
    return float(np.linalg.norm(g - ref) / np.linalg.norm(ref)) / TOL.GRAD_REL_L2


JAC_REL_FRO = 1e-5


def jac_use(J, ref, lengths):
    """worst over the live samples of ||J - ref||_F / ||ref||_F, as a share of JAC_REL_FRO; J, ref [n, T, rows, cols]"""
    worst = 0.0
    for r in range(J.shape[0]):
        for t in range(int(lengths[r])):
            worst = max(worst, float(np.linalg.norm(J[r, t] - ref[r, t]) / np.linalg.norm(ref[r, t])))
    return worst / JAC_REL_FRO
