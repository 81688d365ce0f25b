"""The case table of tests/test_gpu_trpo_solve.py and its float64 side, on the CPU alone (tests/test_solve_cases.py checks the table, that every
bound is a small share of what it bounds, that the reference's line-search decisions are clear and that the bounds discriminate, without the library).

A solve case is a case of tests/update_cases.py (family, env, policy shape, N, mask: its data, masks and seeds) and a solve length k = cg_iters.
Every case runs at k = 2 (the init tail, a middle CG step, the last step with its finish; a case whose bounds were too wide there would run at
k = 1: RUNS_SHORT, empty); one lead case per (family, env, policy shape) runs also at k = 0, 1, 3, 10.
residual_tol = 0: the early exit has its own test.

Reference: oracle.metrpo_oracle on the valid rows -- krylov.cg (restated in run_solve so that single products can be replaced) over
fisher_vector_product, the step scale sqrt(2 max_kl / (d.(H d) + 1e-8)) from an explicit product and from the recurrence x.(g - r), the
backtracking search over surrogate_loss_kl at fp32-rounded trial thetas.  The solve starts from whatever gradient it is handed: the GPU test hands
it the device's, so that the gradient kernel's error (held to GRAD_REL_L2 on its own) does not spend the solve's budget.

Bounds (tolerances.SOLVE_DRAWS / SOLVE_MARGIN): the movement of that float64 solve when each of its products z_i is perturbed by what the FVP_REL_L2
row already admits -- a seeded random direction whose norm per variable block is tolerances.block_bound(FVP_REL_L2, z_i[blk], z_i) -- worst over
the draws, times the margin, on d, beta and step = beta d; whole vector and per block W_l, b_l, log_std; never more than CAP = 0.1 of the block's own
norm.  Nothing in them comes from a kernel."""
from collections import namedtuple

import numpy as np
from oracle import metrpo_oracle as O
import tolerances as TOL
import update_cases as U

MAX_KL, RATIO, MAX_BACKTRACKS = 0.01, 0.8, 15                   # [rllab] ConjugateGradientOptimizer's defaults (algos/trpo.py:18-20)
# reg_coeff: NOT rllab's 1e-5.  At 1e-5 the term reg * p is as large as the error the FVP_REL_L2 row admits of a product (1e-5 of it, Fisher
# eigenvalues being O(1) here), so no bound derived from that row can notice that it is missing (measured on the reference: a solve without it
# uses 0.04 ... 1.8 of the bounds).  100 x the row makes its absence visible at every case; the default is what tests/test_gpu_engine.py runs.
REG = 1e-3
K_ALL, K_SHORT, LEAD_KS = 2, 1, (0, 1, 3, 10)
# update_cases ids that run at K_SHORT because a per-block bound of theirs exceeds 0.1 of the block at K_ALL (condition (a)).  None does: the rank-deficient
# Fisher matrices of N = 1 and of mask `one` (rank <= 2 na) still leave k = 2 well-conditioned (largest share 7.4e-4 of a block).
RUNS_SHORT = frozenset()
GEMM_WIDTHS = ((), (3,), (17,), (65, 33), (24, 24, 24, 24))     # P below one block ... a padded, stacked shape
TILE = 16                                                       # sample tile of the fused kernels
CORRUPTIONS = ('block_scaled', 'tile_left_out', 'invalid_included', 'stale_vector', 'reg_left_out', 'reg_left_out_of_dhd')
# The float64 side's own rounding (another summation order than the device's float64 tails, amplified by the solve): no bound is held below this
# share of the reference's norm.  At k = 0 it is all there is (d = 0 exactly, beta = sqrt(2 max_kl / 1e-8)).
FLOAT64_FLOOR = 1e-12
# Condition (a): no bound is wider than this share of what it bounds.  The rule gives more only at k = 10 (7 of the 14 lead cases: up to 3.0 of a block);
# those bounds are cut to it.
CAP = 0.1

SCase = namedtuple('SCase', 'id ucase k draws lead')


def lead_n(uc):
    """The lead N of a case's family: 129; 65 on the GEMM path (its table's largest N below 129); PT + 1 = 129, 65, 33 on the generic kernels."""
    if uc.family == 'generic':
        return {(32, 32): 129, (100, 50, 25): 65, (256, 128): 33}[uc.ph]
    return {'mfma': 129, 'fused3': 129, 'gemm': 65}[uc.family]


# Seeds are update_cases' own, except where a line-search decision of the float64 solve lies within the LOSS_RTOL / KL_* rows of its threshold
# (condition (b)): those cases take the next seed that is clear, found on the reference alone (tests/test_solve_cases.py checks every case).
SEEDS = {'generic-humanoid-100x50x25-N63-none-k2': 1149, 'generic-humanoid-100x50x25-N64-none-k2': 1153, 'generic-humanoid-100x50x25-N64-edges-k2': 1155,
         'generic-humanoid-100x50x25-N65-none-k2': 1157}


def _build():
    cases = []
    for uc in U.CASES:
        if uc.family == 'gemm' and (uc.env != 'swimmer' or uc.ph not in GEMM_WIDTHS):
            continue
        k = K_SHORT if uc.id in RUNS_SHORT else K_ALL
        sid = '%s-k%d' % (uc.id, k)
        cases.append(SCase(sid, uc._replace(seed=SEEDS.get(sid, uc.seed)), k, TOL.SOLVE_DRAWS, False))
        if uc.nspec == lead_n(uc) and uc.mask == 'none':
            for kk in LEAD_KS:
                sid = '%s-k%d' % (uc.id, kk)
                cases.append(SCase(sid, uc._replace(seed=SEEDS.get(sid, uc.seed)), kk, TOL.SOLVE_DRAWS, True))
    return cases


CASES = _build()


# ---- the float64 solve ------------------------------------------------------------------------------------------------------------------------------
def problem(d, rows=None):
    """What the solve reads of update_cases.case_data(case): the valid rows (or `rows`, a boolean mask) and the mean's denominator."""
    keep = d['keep'] if rows is None else np.asarray(rows, bool)
    sel = tuple(d[k][keep] for k in ('obs', 'act', 'adv', 'om', 'ols'))
    return dict(th=d['th'], pd=d['pdims'], sel=sel, n=int(d['keep'].sum()))


def fisher(pb):
    """v -> Fisher-vector product WITHOUT the reg term (what the device's FVP kernels return), mean over the case's n valid samples."""
    th, pd, obs, n = pb['th'], pb['pd'], pb['sel'][0], pb['n']
    if obs.shape[0] == 0:
        return lambda v: np.zeros_like(v)
    scale = obs.shape[0] / float(n)                      # (a corrupted row set keeps the true denominator, as a kernel's inv_n_global would)
    return lambda v: scale * O.fisher_vector_product(th, pd, obs, v, reg_coeff=0.0)


def run_solve(g, k, prod, reg=REG, reg_in_dhd=True):
    """[rllab] krylov.cg (oracle.metrpo_oracle.cg, residual_tol = 0) with z_i = prod(i, p_i) + reg p_i, then both forms of the step scale.
    prod(i, v): the Fisher part of the i-th product; i = k is the explicit d.(H d) product.  k = 0: d = 0, both scales from x.(g - r) = 0."""
    g = np.asarray(g, np.float64)
    p, r, x = g.copy(), g.copy(), np.zeros_like(g)
    rdotr = r.dot(r)
    zs, ps = [], []
    with np.errstate(all='ignore'):
        for i in range(k):
            zf = prod(i, p)
            z = zf + reg * p
            zs.append(zf); ps.append(p.copy())
            v = rdotr / p.dot(z)
            x = x + v * p
            r = r - v * z
            newrdotr = r.dot(r)
            p = r + (newrdotr / rdotr) * p
            rdotr = newrdotr
        xhx_imp = x.dot(g - r)
        xhx_exp = xhx_imp
        if k > 0:
            zf = prod(k, x)
            zs.append(zf); ps.append(x.copy())
            xhx_exp = x.dot(zf + (reg * x if reg_in_dhd else 0.0))
        beta = [np.sqrt(2.0 * MAX_KL * (1.0 / (q + 1e-8))) for q in (xhx_exp, xhx_imp)]
    beta = [1.0 if np.isnan(b) else float(b) for b in beta]
    return dict(d=x, beta=beta[0], beta_imp=beta[1], step=beta[0] * x, step_imp=beta[1] * x, zs=zs, ps=ps, k=k)


def admitted_error(z, pdims, rng):
    """A random direction whose norm per variable block is what the FVP row admits of that block: block_bound(FVP_REL_L2, z[blk], z)."""
    out = np.zeros_like(z)
    for _, sl in U.blocks(pdims):
        u = rng.randn(z[sl].size)
        out[sl] = u * (TOL.block_bound(TOL.FVP_REL_L2, z[sl], z) / max(np.linalg.norm(u), 1e-300))
    return out


def _norms(vec, pdims):
    out = {'whole': float(np.linalg.norm(vec))}
    for nm, sl in U.blocks(pdims):
        out[nm] = float(np.linalg.norm(vec[sl]))
    return out


def solve_and_bounds(d, k, g=None, draws=None):
    """-> (ref, bounds): the float64 solve of the case from gradient g (default: the float64 gradient) and the bounds on a device's d, beta and step:
    bounds['d' | 'step'][block or 'whole'] on the 2-norm of the difference, bounds['beta'] on |beta - ref|; ref['norms'] holds the reference's norms."""
    draws = TOL.SOLVE_DRAWS if draws is None else draws
    pb = problem(d)
    F = fisher(pb)
    pd = d['pdims']
    if g is None:
        g = O.surrogate_loss_grad(pb['th'], pd, *pb['sel'])[1]
    ref = run_solve(g, k, lambda i, v: F(v))
    ref['g'] = np.asarray(g, np.float64)
    ref['norms'] = {'d': _norms(ref['d'], pd), 'step': _norms(ref['step'], pd)}
    worst = {'d': dict.fromkeys(ref['norms']['d'], 0.0), 'step': dict.fromkeys(ref['norms']['d'], 0.0), 'beta': 0.0}
    for m in range(draws):
        rng = np.random.RandomState((d['case'].seed * 131 + 17 * k + m) % (2 ** 31))

        def prod(i, v):
            z = F(v)
            return z + admitted_error(z, pd, rng)
        got = run_solve(g, k, prod)
        for key, a, b in (('d', got['d'], got['d']), ('step', got['step'], got['step_imp'])):
            for form in (a, b):
                for nm, val in _norms(form - ref[key], pd).items():
                    worst[key][nm] = max(worst[key][nm], val)
        worst['beta'] = max(worst['beta'], abs(got['beta'] - ref['beta']), abs(got['beta_imp'] - ref['beta']))
    def bound(w, norm, whole):
        # never wider than condition (a) allows: where the perturbed solves move a block by more than CAP of itself (ten iterations on N <= 129 samples),
        # the block is held to CAP of its norm instead -- a bound of the block's own size would pass anything
        b = TOL.SOLVE_MARGIN * w
        if norm > 0.0:
            b = min(b, CAP * norm)
        return max(b, FLOAT64_FLOOR * whole)
    bounds = {key: {nm: bound(w, ref['norms'][key][nm], ref['norms'][key]['whole']) for nm, w in worst[key].items()} for key in ('d', 'step')}
    bounds['beta'] = bound(worst['beta'], abs(ref['beta']), abs(ref['beta']))
    ref['capped'] = sorted('%s %s' % (key, nm) for key in ('d', 'step') for nm, w in worst[key].items() if TOL.SOLVE_MARGIN * w > CAP * ref['norms'][key][nm] > 0.0)
    if TOL.SOLVE_MARGIN * worst['beta'] > CAP * abs(ref['beta']):
        ref['capped'].append('beta')
    return ref, bounds


def shares(got_d, got_beta, ref, bounds, pdims, implicit=True):
    """Worst share of its bound each of d, beta, step uses -> {'d': (share, block), 'beta': share, 'step': (share, block)}; <= 1 passes."""
    got_d = np.asarray(got_d, np.float64)
    out = {}
    for key, vec in (('d', got_d), ('step', float(got_beta) * got_d)):
        worst, where = 0.0, 'whole'
        for nm, val in _norms(vec - ref[key], pdims).items():
            b = bounds[key][nm]
            use = 0.0 if val == 0.0 else (val / b if b > 0.0 else float('inf'))
            if use > worst:
                worst, where = use, nm
        if not np.all(np.isfinite(vec)):
            worst, where = float('inf'), 'non-finite'
        out[key] = (worst, where)
    err = abs(float(got_beta) - ref['beta'])
    out['beta'] = 0.0 if err == 0.0 else (err / bounds['beta'] if bounds['beta'] > 0.0 else float('inf'))
    if not np.isfinite(got_beta):
        out['beta'] = float('inf')
    return out


def worst_share(sh):
    return max(sh['d'][0], sh['step'][0], sh['beta'])


# ---- the line search --------------------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def trial_theta(th, beta, dvec, n):
    """cur_param = prev_param - ratio^n * (beta d), formed in float64 and stored as fp32 (k_try_theta / ls_next_theta)."""
    return f32(th - (RATIO ** n) * (beta * np.asarray(dvec, np.float64)))


def decision(loss, kl, loss_before):
    """-> (accept, clear): the loop's break test loss < loss_before and kl <= max_kl, and whether it is clear of its thresholds by the LOSS_RTOL /
    KL_ATOL / KL_RTOL rows (both losses carry the row; a NaN is a clear 'no')."""
    if np.isnan(loss) or np.isnan(kl):
        return False, True
    ml = TOL.LOSS_RTOL * (max(1.0, abs(loss)) + max(1.0, abs(loss_before)))
    mk = max(TOL.KL_ATOL, TOL.KL_RTOL * abs(kl))
    accept = bool(loss < loss_before and kl <= MAX_KL)
    clear_yes = loss < loss_before - ml and kl < MAX_KL - mk
    clear_no = loss > loss_before + ml or kl > MAX_KL + mk
    return accept, bool(clear_yes or clear_no)


def line_search(d, beta, dvec, loss_before=None, upto=None):
    """The backtracking loop on the valid rows from (beta, d) -> list of (n, loss, kl, accept, clear), up to the accepted trial (or trial `upto`)."""
    pb = problem(d)
    if loss_before is None:
        loss_before = O.surrogate_loss_kl(pb['th'], pb['pd'], *pb['sel'])[0]
    out = []
    for n in range(MAX_BACKTRACKS):
        with np.errstate(all='ignore'):
            loss, kl = O.surrogate_loss_kl(trial_theta(pb['th'], beta, dvec, n), pb['pd'], *pb['sel'])
        acc, clear = decision(loss, kl, loss_before)
        out.append((n, float(loss), float(kl), acc, clear))
        if (upto is None and acc) or (upto is not None and n >= upto):
            break
    return out


# ---- seeded corruptions of the float64 solve (condition (c)) ------------------------------------------------------------------------------------------
def corrupted(d, k, name, g, ref):
    """The float64 solve with one seeded defect of the kinds a cached product or a tail could have -> run_solve's dict, or None where the defect is the
    identity on this case's data (no invalid sample to include)."""
    pb = problem(d)
    F = fisher(pb)
    pd, N, keep = d['pdims'], d['N'], d['keep']
    rng = np.random.RandomState(d['case'].seed + 99)
    if name == 'block_scaled':
        # One drawn block of every product scaled by 1 + 1e-3 (a kernel's defect is in each of its launches), the block among those that carry at
        # least their even share of the first product's norm: there block_bound is FVP_REL_L2 of the block itself and the defect is 100 x what the
        # row admits.  (Below the even share the row admits an absolute error, which 1e-3 of a small enough block does not reach: such a defect is
        # within the FVP row, not a miss of these bounds.)
        z = ref['zs'][0]
        blks = [sl for _, sl in U.blocks(pd) if np.linalg.norm(z[sl]) >= (z[sl].size / float(z.size)) ** 0.5 * np.linalg.norm(z)]
        sl = blks[rng.randint(len(blks))]

        def prod(i, v):
            z = F(v).copy()
            z[sl] *= 1.0 + 1e-3
            return z
        return run_solve(g, k, prod)
    if name == 'tile_left_out':                             # the last 16-sample tile that holds a valid sample is not summed (denominator unchanged)
        rows = keep.copy()
        t = int(np.flatnonzero(keep)[-1]) // TILE
        rows[TILE * t:TILE * (t + 1)] = False
        Fc = fisher(problem(d, rows))
        return run_solve(g, k, lambda i, v: Fc(v))
    if name == 'invalid_included':                          # the mask is ignored by the products (denominator unchanged)
        if keep.all():
            return None
        Fc = fisher(problem(d, np.ones(N, bool)))
        return run_solve(g, k, lambda i, v: Fc(v))
    if name == 'stale_vector':                              # the second product is taken of the first product's vector (k = 1: the step-scale product)
        first = []

        def prod(i, v):
            if i == 0:
                first.append(v.copy())
            return F(first[0]) if i == 1 else F(v)
        return run_solve(g, k, prod)
    if name == 'reg_left_out':
        return run_solve(g, k, lambda i, v: F(v), reg=0.0, reg_in_dhd=True)
    if name == 'reg_left_out_of_dhd':
        return run_solve(g, k, lambda i, v: F(v), reg_in_dhd=False)
    raise ValueError(name)


def corruption_share(bad, ref, bounds, pdims):
    """Worst share over d, beta, step and both forms of the step scale."""
    a = worst_share(shares(bad['d'], bad['beta'], ref, bounds, pdims))
    b = worst_share(shares(bad['d'], bad['beta_imp'], ref, bounds, pdims))
    return max(a, b)
