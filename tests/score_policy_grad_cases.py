"""The case table of tests/test_gpu_score_policy_grad.py and its float64 side, on the CPU alone (tests/test_score_policy_grad_ref.py checks the table
and the kink guard without the library).

The table is score_grad_cases' (both paths, the generic-only shapes included: same shapes, same ensembles and policies), with noise_in_std alternating
over the cases.  The noise is 0.8 N(0, 1) in ACTION units: where the noise is in units of the policy's std it is divided by sigma, so that the clip
acts in every case (sigma is ~0.1 .. 1: undivided, a few per cent of swimmer's actions would clip).  The kink guard is score_grad_cases' (KINK_FACTOR,
MAX_REPLACED), with the clip site |a_t| - 1 taken on every head's own a_t = mean_t + noise_t sigma, in float32 and float64."""
from collections import namedtuple

import numpy as np

from oracle import metrpo_oracle as O
import score_grad_cases as GC
import score_policy_grad_ref as R

KINK_FACTOR = GC.KINK_FACTOR
MAX_REPLACED = GC.MAX_REPLACED
SEED_OFFSET = 40000

PCase = namedtuple('PCase', GC.Case._fields + ('in_std',))

# seeds are the open-loop case's + SEED_OFFSET, except where that draw cannot meet the kink guard's conditions (found on the reference alone)
SEEDS = {}


def _build():
    cases = []
    for i, c in enumerate(GC.CASES):
        cid = c.id + ('-std' if i % 2 else '-act')
        cases.append(PCase(*(c._replace(id=cid, seed=SEEDS.get(cid, c.seed + SEED_OFFSET)) + (bool(i % 2),))))
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}

f32 = GC.f32
shape_key = GC.shape_key
problem = GC.problem                 # (dm, theta, pdims, pool) of the case's shape, rounded to fp32

_DATA = {}


def guard(dm, theta, pdims, case, init, noise):
    """score_grad_cases.guard on the closed-loop walk: -> (ok [B], margin [B])"""
    kw = dict(gamma=case.gamma, stop_at_done=case.stop, noise_in_std=case.in_std, grad=False)
    a64 = R.walk(dm, theta, pdims, case.env, init, noise, dtype=np.float64, **kw)['sites']
    a32 = R.walk(dm, theta, pdims, case.env, init, noise, dtype=np.float32, **kw)['sites']
    B = noise.shape[1]
    ok, margin = np.ones(B, bool), np.full(B, np.inf)
    for n in a64:
        diff = np.abs(a32[n] - a64[n])
        ok &= np.all((np.sign(a32[n]) == np.sign(a64[n])) & (a64[n] != 0) & (np.abs(a64[n]) >= KINK_FACTOR * diff), axis=1)
        margin = np.minimum(margin, np.min(np.abs(a64[n]) / np.maximum(diff, 1e-300), axis=1))
    return ok, margin


def case_data(case):
    """-> dict(case, dm, theta, pdims, init [S, ns], noise [T, B, na] (fp32 values), replaced, accepted, margin); cached."""
    if case.id in _DATA:
        return _DATA[case.id]
    dm, theta, pdims, pool = problem(case)
    rng = np.random.RandomState(case.seed)
    B, T, S, na = case.B, case.T, case.S, dm.na
    init = pool[rng.permutation(len(pool))[:S]].copy()
    if case.variant == 'ant_plant':
        init[:, 2] = f32(0.25 + 0.7 * ((np.arange(S) * 7) % 11) / 10.0)
        init[5::13, 2] = f32(1.15)
    sigma = np.exp(O.policy_log_std(theta, pdims)) if case.in_std else np.ones(na)
    draw = lambda n: f32(0.8 * rng.randn(T, n, na) / sigma)
    noise = draw(B)
    ok, margin = guard(dm, theta, pdims, case, init, noise)
    replaced = 0
    while not ok.all():
        bad = np.flatnonzero(~ok)
        replaced += len(bad)
        if replaced > MAX_REPLACED * B:
            break                                                   # (asserted by tests/test_score_policy_grad_ref.py, from these figures)
        noise[:, bad] = draw(len(bad))
        ok, margin = guard(dm, theta, pdims, case, init, noise)
    d = dict(case=case, dm=dm, theta=theta, pdims=pdims, init=init, noise=noise, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _DATA[case.id] = d
    return d


def reference(d):
    """The float64 reference of a case (score_policy_grad_ref.score_policy_actions_grad's dict); cached in d."""
    if 'ref' not in d:
        c = d['case']
        d['ref'] = R.score_policy_actions_grad(d['dm'], d['theta'], d['pdims'], c.env, d['init'], d['noise'], gamma=c.gamma, stop_at_done=c.stop,
                                               noise_in_std=c.in_std)
    return d['ref']


def shares(got, ref, case):
    """score_grad_cases.shares (grad whole / per step / per candidate, lam0 whole / per candidate, ret) with a seventh entry: grad_mean's worst of
    whole, per step and per candidate, held by the same row; <= 1 passes."""
    out = np.concatenate([GC.shares(got, ref, case), [0.0]])
    if got.get('grad_mean') is not None:
        import tolerances as TOL
        out[6] = max(GC.grad_use(got['grad_mean'], ref['grad_mean'], TOL.BPTT_GRAD_REL_L2))
    return out
