"""The case table of tests/test_gpu_score_grad.py and its float64 side, on the CPU alone (tests/test_score_grad_ref.py checks the table and the kink
guard without the library).

A case is (path, env, K, dynamics widths, activation, B, T, S, gamma, stop_at_done, variant).  path 'fused' is metrpo_score_actions_grad's fused shape
class (score_actions_grad.hip: 16-candidate wave tiles, four of one head per workgroup in the reverse sweep, so B = 63 / 64 / 65 are the workgroup's
edges and 15 / 16 / 17 the tile's); 'generic' is every other shape, or the fused shapes with force_generic.

The gradient of a return is piecewise smooth in the actions: a relu pre-activation, |a| = 1, half-cheetah's reward clip, hopper's max terms and Ant's
z bounds are kinks at which fp32 and float64 may take different branches.  guard() walks a case in float64 and in float32 beside it
(score_grad_ref.walk keeps the signed distance of every such argument from its kink) and a candidate whose float64 argument lies within KINK_FACTOR x
the float32 - float64 difference of a kink, or on the other side, has its action sequence drawn afresh; at most MAX_REPLACED of a case's candidates.
The draws are 0.8 N(0, 1): every case has actions beyond the clip at some steps, so the gate is exercised.
variant 'ant_plant': the start states' z (dim 2) is dealt out over [0.25, 0.95] so that candidates end at assorted steps of the horizon."""
from collections import namedtuple

import numpy as np

import helpers as Hh
import score_grad_ref as R

KINK_FACTOR = 16.0                   # bptt_cases' factor
MAX_REPLACED = 0.25                  # of a case's candidates
FUSED_ENVS = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant')
SIZES_B = (1, 15, 16, 17, 33, 63, 64, 65)

Case = namedtuple('Case', 'id path env K dh act B T S gamma stop variant seed')

# seeds are 7000 + the case's index, except where that draw cannot meet the kink guard's conditions (found on the reference alone)
SEEDS = {}


def _build():
    cases = []

    def add(path, env, B, T, K=5, dh=(64, 64), act='relu', S=1, gamma=0.99, stop=True, variant='plain'):
        cid = '%s-%s-%s-%s-K%d-B%d-T%d-S%d-g%s-%s-%s' % (path, env, 'x'.join(map(str, dh)), act, K, B, T, S, gamma, 'stop' if stop else 'nostop', variant)
        cases.append(Case(cid, path, env, K, tuple(dh), act, B, T, S, gamma, stop, variant, SEEDS.get(cid, 7000 + len(cases))))

    for path in ('fused', 'generic'):
        for B in SIZES_B:                                            # every tile and workgroup edge
            add(path, 'swimmer', B, 2)
        for env in FUSED_ENVS:                                       # every env at the long horizon, a tile straddling start states
            add(path, env, 33, 11, S=3)
        for K in (1, 8, 9):
            add(path, 'swimmer', 17, 2, K=K)
        add(path, 'swimmer', 65, 2, dh=(48, 48))                     # the zero-padded layout
        add(path, 'ant', 17, 2, dh=(48, 20))
        add(path, 'half_cheetah', 17, 1)
        add(path, 'hopper', 16, 2, S=16)                             # S = B
        add(path, 'snake', 64, 2, S=64, gamma=1.0)
        add(path, 'swimmer', 33, 11, S=3, gamma=1.0, stop=False)
        add(path, 'ant', 33, 11, S=3, stop=False)
        add(path, 'ant', 65, 11, S=65, variant='ant_plant')
        add(path, 'ant', 17, 2, S=17, gamma=1.0, variant='ant_plant')
    # shapes only the generic path has
    add('generic', 'swimmer', 33, 3, dh=(128, 128), S=3)
    add('generic', 'humanoid', 17, 3, K=2, dh=(32, 32))
    add('generic', 'humanoid', 33, 2, K=2, dh=(48, 48, 32), S=3)
    add('generic', 'half_cheetah', 33, 3, K=2, dh=(32, 32), act='tanh', S=3)
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def shape_key(case):
    return (case.env, case.K, case.dh, case.act)


_PROBLEMS, _DATA = {}, {}


def problem(case):
    """The ensemble of the case's shape (one per (env, K, widths, activation): the GPU test keeps one engine per shape), rounded to fp32."""
    key = shape_key(case)
    if key not in _PROBLEMS:
        seed = 500 + (FUSED_ENVS.index(case.env) if case.env in FUSED_ENVS else 6)
        dm, theta, pdims, pool = Hh.problem_data(case.env, case.K, case.dh, (32, 32), seed=seed, dyn_act=case.act)
        _PROBLEMS[key] = (dm.astype(np.float32).astype(np.float64), f32(theta), pdims, f32(pool))
    return _PROBLEMS[key]


def guard(dm, case, init, actions):
    """-> (ok [B]: the same branch at every kink site in float32 and float64 and the float64 argument at least KINK_FACTOR x their difference away
    from the kink; margin [B]: the smallest |argument| / difference of the candidate)."""
    a64 = R.walk(dm, case.env, init, actions, case.gamma, case.stop, np.float64, grad=False)['sites']
    a32 = R.walk(dm, case.env, init, actions, case.gamma, case.stop, np.float32, grad=False)['sites']
    B = actions.shape[1]
    ok, margin = np.ones(B, bool), np.full(B, np.inf)
    for n in a64:
        diff = np.abs(a32[n] - a64[n])
        ok &= np.all((np.sign(a32[n]) == np.sign(a64[n])) & (a64[n] != 0) & (np.abs(a64[n]) >= KINK_FACTOR * diff), axis=1)
        margin = np.minimum(margin, np.min(np.abs(a64[n]) / np.maximum(diff, 1e-300), axis=1))
    return ok, margin


def case_data(case):
    """-> dict(case, dm, init [S, ns], actions [T, B, na] (fp32 values), replaced, accepted, margin); cached."""
    if case.id in _DATA:
        return _DATA[case.id]
    dm, _, _, pool = problem(case)
    rng = np.random.RandomState(case.seed)
    B, T, S, na = case.B, case.T, case.S, dm.na
    init = pool[rng.permutation(len(pool))[:S]].copy()
    if case.variant == 'ant_plant':
        init[:, 2] = f32(0.25 + 0.7 * ((np.arange(S) * 7) % 11) / 10.0)
        init[5::13, 2] = f32(1.15)                                  # outside 0.2 <= z <= 1.0; the model moves z by ~0.1 a step: done at the first step
    draw = lambda n: f32(0.8 * rng.randn(T, n, na))
    actions = draw(B)
    ok, margin = guard(dm, case, init, actions)
    replaced = 0
    while not ok.all():
        bad = np.flatnonzero(~ok)
        replaced += len(bad)
        if replaced > MAX_REPLACED * B:
            break                                                   # (asserted by tests/test_score_grad_ref.py, from these figures)
        actions[:, bad] = draw(len(bad))
        ok, margin = guard(dm, case, init, actions)                 # the whole batch again: candidate b's start row depends on b
    d = dict(case=case, dm=dm, init=init, actions=actions, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _DATA[case.id] = d
    return d


def reference(d):
    """The float64 reference of a case (score_grad_ref.score_actions_grad's dict); cached in d."""
    if 'ref' not in d:
        c = d['case']
        d['ref'] = R.score_actions_grad(d['dm'], c.env, d['init'], d['actions'], c.gamma, c.stop)
    return d['ref']


def grad_use(got, ref, row):
    """Shares of its bounds a [T, B, n] gradient of one head uses: -> (whole rel-L2 / row, worst per-step share, worst per-candidate share); <= 1
    passes.  The per-step and per-candidate blocks are held by tolerances.block_bound, so one wrong step or row cannot hide in the whole."""
    import tolerances as TOL
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.all(np.isfinite(got)):
        return float('inf'), float('inf'), float('inf')
    whole = float(np.linalg.norm(got - ref) / max(row * np.linalg.norm(ref), 1e-300))
    step = max(float(np.linalg.norm(got[t] - ref[t]) / max(TOL.block_bound(row, ref[t], ref), 1e-300)) for t in range(ref.shape[0]))
    cand = max(float(np.linalg.norm(got[:, b] - ref[:, b]) / max(TOL.block_bound(row, ref[:, b], ref), 1e-300)) for b in range(ref.shape[1]))
    return whole, step, cand


def lam_use(got, ref, row):
    """The same for lam0 [B, ns] of one head: (whole, worst per-candidate share)."""
    w, _, c = grad_use(np.asarray(got)[None], np.asarray(ref)[None], row)
    return w, c


def reward_row(t):
    """tests/tolerances.py: REWARD for step t <= 10, LONG_RUN beyond (tests/test_gpu_score_actions.py's rule)."""
    import tolerances as TOL
    return TOL.REWARD if t <= 10 else TOL.LONG_RUN


def shares(got, ref, case, row=None, ret_row=reward_row):
    """Worst share over the heads of every bound tests/test_gpu_score_grad.py holds: np.array([grad whole, grad per step, grad per candidate,
    lam0 whole, lam0 per candidate, ret]); <= 1 passes.  grad / lam0: rel-L2 `row` (BPTT_GRAD_REL_L2) per head and by block_bound per step and per
    candidate; ret: sum_t gamma^t (atol + rtol |r_t|) (score_actions_ref.bound).  got may lack lam0 / ret (their shares are then 0)."""
    import tolerances as TOL
    import score_actions_ref as SA
    row = TOL.BPTT_GRAD_REL_L2 if row is None else row
    out = np.zeros(6)
    for k in range(ref['grad'].shape[0]):
        out[:3] = np.maximum(out[:3], grad_use(got['grad'][k], ref['grad'][k], row))
        if got.get('lam0') is not None:
            out[3:5] = np.maximum(out[3:5], lam_use(got['lam0'][k], ref['lam0'][k], row))
    if got.get('ret') is not None:
        bnd = SA.bound(ref['rew'], case.gamma, ret_row)
        out[5] = float((np.abs(np.asarray(got['ret'], np.float64) - ref['ret']) / bnd).max())
    return out
