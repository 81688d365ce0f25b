"""The case table of tests/test_gpu_terminal_value.py and its float64 side, on the CPU alone (tests/test_terminal_value_ref.py checks the table, the
kink guard and the bounds without the library).  After tests/score_grad_cases.py: its ensembles and policies (one engine per shape), its kink guard
(KINK_FACTOR, MAX_REPLACED) with one more site, the terminal value's clip |s_T,d| = 10.

A case is score_grad_cases' (path, env, K, dynamics widths, activation, B, T, S, gamma, stop_at_done, variant, seed) with
    nb      biases of the terminal value: 1, or S (candidate b uses bias[b // (B // S)])
    calls   'all': the two scoring calls and the two gradient calls; 'grad': the gradient calls alone (the reverse sweep's workgroup edges)
    in_std  closed loop: the noise is in units of the policy's std
    noise   closed loop: False = d_noise NULL (then B = S)
and is walked twice, open loop (supplied actions) and closed loop (noise around the policy).

Draws: actions / noise 0.8 N(0, 1) in action units (score_policy_grad_cases' rule where the noise is in std units); w1 ~ 0.5 N(0, 1), w2 ~ 0.1 N(0, 1),
bias ~ N(0, 1), so that V weighs like a few steps' reward.  variant 'ant_plant': score_grad_cases' (candidates end at assorted steps: at the first,
in the middle, at the last, never); 'tv_far': dims 0 and 3 of the odd start states are +12 and -12, beyond the value's clip, so the clip and its gate
are exercised.

Bounds (tests/tolerances.py, none new): grad / lam0 by BPTT_GRAD_REL_L2 per head, and by block_bound per step and per candidate
(score_grad_cases.grad_use); ret by score_actions_ref.bound extended by one term,
    sum_t gamma^t (row(t).atol + row(t).rtol |r_t|) + gamma^T (row(T).atol + row(T).rtol (|bias| + sum_d |w1 o| + |w2 o^2|)),
row(t) = REWARD for t <= 10, LONG_RUN beyond."""
from collections import namedtuple

import numpy as np

from oracle import metrpo_oracle as O
import score_actions_ref as SA
import score_grad_cases as GC
import terminal_value_ref as R

KINK_FACTOR = 16.0
MAX_REPLACED = 0.25                  # of a case's candidates
FUSED_ENVS = GC.FUSED_ENVS
LOOPS = ('open', 'closed')

Case = namedtuple('Case', GC.Case._fields + ('nb', 'calls', 'in_std', 'noise'))

# seeds are 26000 + the case's index, except where that draw cannot meet the kink guard's conditions (found on the reference alone)
SEEDS = {}


def _build():
    cases = []

    def add(path, env, B, T, K=5, dh=(64, 64), act='relu', S=1, gamma=0.99, stop=True, variant='plain', nb=1, calls='all', in_std=None, noise=True):
        in_std = bool(len(cases) % 2) if in_std is None else in_std
        cid = '%s-%s-%s-%s-K%d-B%d-T%d-S%d-g%s-%s-%s-nb%d-%s%s' % (path, env, 'x'.join(map(str, dh)), act, K, B, T, S, gamma, 'stop' if stop else 'nostop',
                                                               variant, nb, 'std' if in_std else 'act', '' if noise else '-nonoise')
        cases.append(Case(cid, path, env, K, tuple(dh), act, B, T, S, gamma, stop, variant, SEEDS.get(cid, 26000 + len(cases)), nb, calls, in_std, noise))

    for path in ('fused', 'generic'):
        for B in (1, 15, 16, 17, 33):                                # the tile's edges, all four calls
            add(path, 'swimmer', B, 2)
        for B in (63, 64, 65):                                       # the reverse sweep's workgroup edges
            add(path, 'swimmer', B, 2, calls='grad')
        add(path, 'swimmer', 17, 1)                                  # the seed meets the very first step
        add(path, 'half_cheetah', 17, 1, in_std=True)
        for env in FUSED_ENVS:                                       # every fused env, a bias per start state, a tile straddling start states
            add(path, env, 33, 11, S=3, nb=3)
        add(path, 'ant', 65, 11, S=65, nb=65, variant='ant_plant')   # done at the first step, in the middle, at the last, never
        add(path, 'ant', 65, 11, S=65, nb=1, variant='ant_plant', gamma=1.0, in_std=True)
        for K in (1, 9):
            add(path, 'swimmer', 17, 2, K=K)
        add(path, 'swimmer', 33, 2, dh=(48, 48), S=3, nb=3)          # the zero-padded layout
        add(path, 'swimmer', 33, 11, S=3, nb=3, gamma=1.0, stop=False)
        add(path, 'ant', 33, 11, S=3, stop=False)
        add(path, 'snake', 16, 2, S=16, nb=16, gamma=1.0)            # S = B
        add(path, 'swimmer', 33, 2, S=3, nb=3, variant='tv_far', in_std=False)
        add(path, 'hopper', 33, 3, S=3, nb=1, variant='tv_far', in_std=True)
        add(path, 'swimmer', 17, 2, S=17, nb=17, in_std=False, noise=False)      # closed loop: d_noise NULL
        add(path, 'swimmer', 17, 2, S=17, nb=1, in_std=True, noise=False)
    # shapes only the generic path has
    add('generic', 'humanoid', 17, 3, K=2, dh=(32, 32))
    add('generic', 'swimmer', 33, 3, dh=(128, 128), S=3, nb=3)
    add('generic', 'half_cheetah', 33, 3, K=2, dh=(32, 32), act='tanh', S=3, nb=3)
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}
RUNS = [(c, loop) for c in CASES for loop in LOOPS]
RUN_IDS = ['%s-%s' % (c.id, loop) for c, loop in RUNS]

f32 = GC.f32
shape_key = GC.shape_key
problem = GC.problem                 # (dm, theta, pdims, pool) of the case's shape, rounded to fp32

_DATA = {}


def walk_kw(case, loop, theta, pdims):
    kw = dict(gamma=case.gamma, stop_at_done=case.stop)
    if loop == 'closed':
        kw.update(policy=(theta, pdims), noise_in_std=case.in_std, T=case.T)
    return kw


def guard(d, seq, tv):
    """score_grad_cases.guard on this walk, the terminal value's clip included: -> (ok [B], margin [B])"""
    case = d['case']
    kw = dict(walk_kw(case, d['loop'], d['theta'], d['pdims']), grad=False)
    a64 = R.walk(d['dm'], case.env, d['init'], seq, tv, dtype=np.float64, **kw)['sites']
    a32 = R.walk(d['dm'], case.env, d['init'], seq, tv, dtype=np.float32, **kw)['sites']
    B = case.B
    ok, margin = np.ones(B, bool), np.full(B, np.inf)
    for n in a64:
        diff = np.abs(a32[n] - a64[n])
        ok &= np.all((np.sign(a32[n]) == np.sign(a64[n])) & (a64[n] != 0) & (np.abs(a64[n]) >= KINK_FACTOR * diff), axis=1)
        margin = np.minimum(margin, np.min(np.abs(a64[n]) / np.maximum(diff, 1e-300), axis=1))
    return ok, margin


def case_data(case, loop):
    """-> dict(case, loop, dm, theta, pdims, init [S, ns], seq [T, B, na] (actions or noise, fp32 values; None: closed loop without noise),
    tv = (w1, w2, bias) fp32 values, replaced, accepted, margin); cached."""
    key = (case.id, loop)
    if key in _DATA:
        return _DATA[key]
    dm, theta, pdims, pool = problem(case)
    rng = np.random.RandomState(case.seed + (0 if loop == 'open' else 500))
    B, T, S, ns, na = case.B, case.T, case.S, dm.ns, dm.na
    init = pool[rng.permutation(len(pool))[:S]].copy()
    if case.variant == 'ant_plant':
        init[:, 2] = f32(0.25 + 0.7 * ((np.arange(S) * 7) % 11) / 10.0)
        init[5::13, 2] = f32(1.15)
    if case.variant == 'tv_far':
        init[1::2, 0] = 12.0; init[1::2, 3] = -12.0
    tv = (f32(0.5 * rng.randn(ns)), f32(0.1 * rng.randn(ns)), f32(rng.randn(case.nb)))
    sigma = np.exp(O.policy_log_std(theta, pdims)) if (loop == 'closed' and case.in_std) else np.ones(na)
    draw = lambda n: f32(0.8 * rng.randn(T, n, na) / sigma)
    d = dict(case=case, loop=loop, dm=dm, theta=theta, pdims=pdims, init=init, tv=tv)
    no_noise = loop == 'closed' and not case.noise
    seq = None if no_noise else draw(B)
    ok, margin = guard(d, seq, tv)
    replaced = 0
    while not ok.all() and not no_noise:                            # (without noise there is nothing to draw afresh: the seed has to do)
        bad = np.flatnonzero(~ok)
        replaced += len(bad)
        if replaced > MAX_REPLACED * B:
            break                                                   # (asserted by tests/test_terminal_value_ref.py, from these figures)
        seq[:, bad] = draw(len(bad))
        ok, margin = guard(d, seq, tv)
    d.update(seq=seq, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _DATA[key] = d
    return d


def walk(d, dtype=np.float64, mut=None, tv='set', grad=True):
    """terminal_value_ref.walk on a case's data (tv None: without the terminal value)"""
    c = d['case']
    return R.walk(d['dm'], c.env, d['init'], d['seq'], d['tv'] if tv == 'set' else tv, dtype=dtype, mut=mut, grad=grad,
                  **walk_kw(c, d['loop'], d['theta'], d['pdims']))


def reference(d):
    """The float64 reference of a case (terminal_value_ref.reference's dict); cached in d and never changed."""
    if 'ref' not in d:
        ref = walk(d)
        ref['grad_mean'] = ref['grad'].sum(axis=0) / d['dm'].K
        d['ref'] = ref
    return d['ref']


def ret_bound(ref, case):
    """[K, B]: score_actions_ref.bound with the terminal term"""
    row = GC.reward_row(case.T)
    return SA.bound(ref['rew'], case.gamma, GC.reward_row) + abs(case.gamma) ** case.T * (row['atol'] + row['rtol'] * ref['tv_mag'])


def shares(got, ref, case):
    """Worst share over the heads of every bound: np.array([grad whole, grad per step, grad per candidate, lam0 whole, lam0 per candidate, ret]);
    <= 1 passes.  got may lack grad / lam0 / ret (their shares are then 0)."""
    import tolerances as TOL
    row = TOL.BPTT_GRAD_REL_L2
    out = np.zeros(6)
    for k in range(ref['grad'].shape[0]):
        if got.get('grad') is not None:
            out[:3] = np.maximum(out[:3], GC.grad_use(got['grad'][k], ref['grad'][k], row))
        if got.get('lam0') is not None:
            out[3:5] = np.maximum(out[3:5], GC.lam_use(got['lam0'][k], ref['lam0'][k], row))
    if got.get('ret') is not None:
        g = np.asarray(got['ret'], np.float64)
        out[5] = float((np.abs(g - ref['ret']) / ret_bound(ref, case)).max()) if np.all(np.isfinite(g)) else float('inf')
    return out
