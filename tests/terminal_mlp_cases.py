"""The case table of tests/test_gpu_terminal_mlp.py and its float64 side, on the CPU alone (tests/test_terminal_mlp_ref.py checks the table, the kink
guard and the bounds without the library).  The table is tests/terminal_value_cases.py's -- the same edges on both paths and both loops -- with the
terminal value's MLP form (metrpo_set_terminal_value_mlp) in the quadratic's place:

    hid     the net's hidden widths, (32, 32), (17, 5), (1, 1), (32, 8) in turn over the table (the turn shifted by one every four cases)

Draws: actions / noise as there; W0 ~ N(0, 1) / sqrt(ns), W1 ~ N(0, 1) / sqrt(h1), W2 ~ 2 N(0, 1) / sqrt(h2) (so that V weighs like a few steps'
reward, as the quadratic's draws do), b0, b1, b2 ~ 0.1 N(0, 1), bias ~ N(0, 1).  Variants 'ant_plant' and 'tv_far' as there.

Bounds (tests/tolerances.py, none new): grad / lam0 by BPTT_GRAD_REL_L2 per head, and by block_bound per step and per candidate
(score_grad_cases.grad_use / lam_use); ret by score_actions_ref.bound extended by one term,
    sum_t gamma^t (row(t).atol + row(t).rtol |r_t|) + gamma^T (row(T).atol + row(T).rtol mag + tanh_term),
    mag       = |bias_row| + |b2| + sum_j |W2_j p1_j| + sum_d |dV/ds_d o_d|
    tanh_term = 2e-7 (sum_j |W2_j| + sum_j |W2_j| (1 - p1_j^2) sum_i |W1_ij|)       tanh_fast's stated absolute error carried through the net
row(t) = REWARD for t <= 10, LONG_RUN beyond."""
from collections import namedtuple

import numpy as np

from oracle import metrpo_oracle as O
import score_actions_ref as SA
import score_grad_cases as GC
import terminal_value_cases as TC
import terminal_mlp_ref as R

KINK_FACTOR = TC.KINK_FACTOR
MAX_REPLACED = TC.MAX_REPLACED       # of a case's candidates
FUSED_ENVS = TC.FUSED_ENVS
LOOPS = TC.LOOPS
WIDTHS = ((32, 32), (17, 5), (1, 1), (32, 8))

Case = namedtuple('Case', TC.Case._fields + ('hid',))

# seeds are 33000 + the case's index, except where that draw cannot meet the kink guard's conditions (found on the reference alone)
SEEDS = {}


def _build():
    cases = []
    for i, c in enumerate(TC.CASES):
        hid = WIDTHS[(i + i // len(WIDTHS)) % len(WIDTHS)]                  # in turn, shifted by one every round: neighbours of a family differ
        cid = '%s-h%dx%d' % (c.id, hid[0], hid[1])
        cases.append(Case(*(c._replace(id=cid, seed=SEEDS.get(cid, 33000 + i)) + (hid,))))
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}
RUNS = [(c, loop) for c in CASES for loop in LOOPS]
RUN_IDS = ['%s-%s' % (c.id, loop) for c, loop in RUNS]

f32 = GC.f32
shape_key = GC.shape_key
problem = GC.problem                 # (dm, theta, pdims, pool) of the case's shape, rounded to fp32
walk_kw = TC.walk_kw

_DATA = {}


def draw_net(rng, ns, hid, nb):
    h1, h2 = hid
    return (f32(rng.randn(ns, h1) / np.sqrt(ns)), f32(0.1 * rng.randn(h1)), f32(rng.randn(h1, h2) / np.sqrt(h1)), f32(0.1 * rng.randn(h2)),
            f32(2.0 * rng.randn(h2) / np.sqrt(h2)), f32(0.1 * rng.randn(1)), f32(rng.randn(nb)))


def guard(d, seq, tv):
    """terminal_value_cases.guard on this walk: -> (ok [B], margin [B])"""
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
    tv = (W0, b0, W1, b1, W2, b2, bias) fp32 values, replaced, accepted, margin); cached."""
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
    tv = draw_net(rng, ns, case.hid, case.nb)
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
            break                                                   # (asserted by tests/test_terminal_mlp_ref.py, from these figures)
        seq[:, bad] = draw(len(bad))
        ok, margin = guard(d, seq, tv)
    d.update(seq=seq, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _DATA[key] = d
    return d


def walk(d, dtype=np.float64, mut=None, tv='set', grad=True):
    """terminal_mlp_ref.walk on a case's data (tv None: without the terminal value)"""
    c = d['case']
    return R.walk(d['dm'], c.env, d['init'], d['seq'], d['tv'] if tv == 'set' else tv, dtype=dtype, mut=mut, grad=grad,
                  **walk_kw(c, d['loop'], d['theta'], d['pdims']))


def reference(d):
    """The float64 reference of a case (terminal_mlp_ref.walk's dict with grad_mean [T, B, na]); cached in d and never changed."""
    if 'ref' not in d:
        ref = walk(d)
        ref['grad_mean'] = ref['grad'].sum(axis=0) / d['dm'].K
        d['ref'] = ref
    return d['ref']


def ret_bound(ref, case):
    """[K, B]: score_actions_ref.bound with the terminal term"""
    row = GC.reward_row(case.T)
    return SA.bound(ref['rew'], case.gamma, GC.reward_row) + abs(case.gamma) ** case.T * (row['atol'] + row['rtol'] * ref['tv_mag'] + ref['tv_tanh'])


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
