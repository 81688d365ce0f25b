"""The case table of tests/test_gpu_bptt_edges.py and its float64 side, on the CPU alone (tests/test_bptt_cases.py checks the table, the kink guard
and that the bounds discriminate, without the library).

A case is (sweep family, VJP family, env, K, dynamics widths, policy widths, B, T, gamma, variant).  The references are the ones the suite already
trusts: oracle.bptt_oracle.policy_costs_and_grad (deterministic) and tests/bptt_stochastic_ref.py (stochastic), on the fp32-rounded parameters and x0.
`walk` below is the same computation restated once more with the number format as an argument and the kink arguments kept: in float64 it must
reproduce both references (test_bptt_cases.py), in float32 beside float64 it is the kink guard, and with a `mut` it is the wrong result the bounds
have to catch.

Sweep families (Engine.set_det_path -> 1 fused MFMA, 2 GEMM path, 0 generic):
  mfma      k_det_mfma on the exact 2 x 64 layout, every environment of kDet; 64 envs per workgroup as four 16-env wave tiles
  mfma_pad  the same kernels over the zero-padded copy of a narrower net
  gemm      det_gemm.hip: k_dg_post closes a step in blocks of 32 rows, the pre-step kernels run in 256-thread blocks
  generic   k_bptt_forward / k_bptt_backward, one thread per env, bs = 64 halved until bptt_floats(pd) * bs * 4 bytes <= 160 KiB (generic_bs below
            restates the rule): half_cheetah (32, 32) and ant (64, 64) keep bs = 64, humanoid (48, 48, 32) with the 100-50-25 policy has 786 floats
            per env = 196.5 KiB at 64 and runs at bs = 32.
The policy VJP (the gradient kernels with the mean adjoint supplied, N = K (T + 1) B samples) runs on what the shape picks; on a 2 x 32 policy the
generic and GEMM-path kernels are forced in addition (Engine.set_update_path)."""
from collections import namedtuple

import numpy as np
from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
import helpers as Hh
import tolerances as TOL

KINK_FACTOR = 16.0                   # batch_clear_of_relu_kinks' factor (tests/test_gpu_dyn_train_grad.py)
MAX_REPLACED = 0.25                  # of a case's envs
SIZES_B = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
SHORT_B = (1, 17, 65)
STOCH_B = (1, 17, 65, 129)
FUSED_ENVS = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant')           # kDet (bptt_mfma.hip), in its order: the VJP's table index
DET_PATH = {'mfma': 1, 'mfma_pad': 1, 'gemm': 2, 'generic': 0}
LDS_MAX = 160 * 1024

Case = namedtuple('Case', 'id sweep vjp force env K dh ph B T gamma variant stoch seed')

# (sweep family, env, dynamics widths, policy widths, VJP family the shape picks)
SHAPES = [('mfma', env, (64, 64), (32, 32), 'mfma') for env in FUSED_ENVS] + [
    ('mfma_pad', 'swimmer', (48, 20), (32, 32), 'mfma'),
    ('mfma_pad', 'ant', (16, 16), (32, 32), 'mfma'),
    ('gemm', 'swimmer', (128, 128), (32, 32), 'mfma'),
    ('gemm', 'ant', (128, 160, 128), (24, 16), 'generic'),
    ('gemm', 'swimmer', (24, 16), (8, 8), 'generic'),
    ('generic', 'half_cheetah', (32, 32), (32, 32), 'mfma'),                # bs = 64
    ('generic', 'humanoid', (48, 48, 32), (100, 50, 25), 'gemm'),            # bs = 32; f3_active excludes the VJP: GEMM path (12 471 parameters >= 4096)
]
# one shape per family for K = 1, gamma = 1, the clipped policy, the stochastic form, the forced VJP families
LEAD = {'mfma': SHAPES[0], 'mfma_pad': SHAPES[5], 'gemm': SHAPES[7], 'generic': SHAPES[10]}
ANT = {'mfma': SHAPES[4], 'mfma_pad': SHAPES[6], 'gemm': SHAPES[8], 'generic': ('generic', 'ant', (64, 64), (32, 32), 'mfma')}
# seeds are 4000 + the case's index, except where that draw cannot meet the kink guard's conditions (found on the reference alone)
SEEDS = {}


def net_rows(dims, with_output):
    return sum(dims[1:] if with_output else dims[1:-1])


def bptt_floats(env, dh, ph):
    """floats of LDS per env of the generic sweeps (csrc/bptt.hip: bptt_floats)."""
    ns, na, n_drop = O.ENV_SPECS[env]
    ddims, pdims = [ns + na - n_drop] + list(dh) + [ns], [ns] + list(ph) + [na]
    mw = max(max(ddims), max(pdims), ns + na)
    return 3 * ns + na + (ns + na) + net_rows(pdims, True) + net_rows(ddims, False) + 2 * mw


def generic_bs(env, dh, ph):
    bs = 64
    while bs > 1 and bptt_floats(env, dh, ph) * bs * 4 > LDS_MAX:
        bs >>= 1
    return bs


def _build():
    cases = []

    def add(shape, B, T, gamma=0.97, variant='plain', K=2, stoch=False, vjp=None):
        sweep, env, dh, ph, dflt = shape
        force = vjp is not None and vjp != dflt
        v = vjp or dflt
        cid = '%s-%s-%s-%s-K%d-B%d-T%d-g%s-%s%s-vjp_%s' % (sweep, env, 'x'.join(map(str, dh)), 'x'.join(map(str, ph)), K, B, T, gamma, variant,
                                                          '-stoch' if stoch else '', v)
        cases.append(Case(cid, sweep, v, force, env, K, dh, ph, B, T, gamma, variant, stoch, SEEDS.get(cid, 4000 + len(cases))))

    for shape in SHAPES:
        for B in SIZES_B:
            add(shape, B, 3)
        for T in (1, 2):
            for B in SHORT_B:
                add(shape, B, T)
    for fam in ('mfma', 'mfma_pad', 'gemm', 'generic'):
        lead = LEAD[fam]
        for B, T in ((1, 1), (1, 3), (17, 3), (65, 3)):
            add(lead, B, T, K=1)
        add(lead, 33, 3, gamma=1.0)
        for B in (17, 65):
            add(lead, B, 3, variant='clipped')
        for B in STOCH_B:
            for T in (1, 3):
                add(lead, B, T, stoch=True)
        if lead[3] == (32, 32):                                # forced VJP families on a 2 x 32 policy (N = K (T + 1) B = 4 is below every tile)
            for vjp in ('generic', 'gemm'):
                for B, T in ((1, 1), (17, 1), (1, 3), (17, 3), (65, 3), (129, 3)):
                    add(lead, B, T, vjp=vjp)
        ant = ANT[fam]
        for B in (17, 33, 65, 129):
            add(ant, B, 3, variant='ant_tile')
        for B in (17, 65):
            add(ant, B, 2, variant='ant_tile')
        for B in SHORT_B:
            add(ant, B, 1, variant='ant_all')
            for T in (2, 3):
                for gamma in (0.97, 1.0):
                    add(ant, B, T, gamma=gamma, variant='ant_all')
    # k_dg_pre_mfma<ENV, STOCH> (det_gemm.hip) on the envs SHAPES leaves to swimmer; appended, so that no earlier case's index or seed moves
    for env in FUSED_ENVS[1:]:
        shape = ('gemm', env, (128, 128), (32, 32), 'mfma')
        for B in SHORT_B:
            add(shape, B, 2)
        add(shape, 17, 2, stoch=True)
    return cases


CASES = _build()


def blocks(pdims):
    """[(name, slice)] of the variables W_l, b_l, log_std in the flat parameter vector."""
    out, o = [], 0
    for l, (i, j) in enumerate(zip(pdims[:-1], pdims[1:])):
        out.append(('W%d' % l, slice(o, o + i * j))); o += i * j
        out.append(('b%d' % l, slice(o, o + j))); o += j
    out.append(('log_std', slice(o, o + pdims[-1])))
    return out


def vector_use(got, ref, pdims, row=None):
    """Shares of its bounds a gradient uses: -> (whole-vector rel-L2 / row, worst block share, its name, the log_std block's share); <= 1 passes."""
    row = TOL.BPTT_GRAD_REL_L2 if row is None else row
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    whole = float(np.linalg.norm(got - ref) / max(row * np.linalg.norm(ref), 1e-300))
    worst, name, ls = 0.0, None, 0.0
    for nm, sl in blocks(pdims):
        use = float(np.linalg.norm(got[sl] - ref[sl]) / max(TOL.block_bound(row, ref[sl], ref), 1e-300))
        if nm == 'log_std':
            ls = use
        if use > worst:
            worst, name = use, nm
    if not np.all(np.isfinite(got)):
        whole = worst = float('inf'); name = 'non-finite'
    return whole, worst, name, ls


def cost_use(got, ref):
    """Share of TOL.BPTT_COST (assert_allclose semantics) the costs use."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.all(np.isfinite(got)):
        return float('inf')
    return float(np.max(np.abs(got - ref) / (TOL.BPTT_COST['atol'] + TOL.BPTT_COST['rtol'] * np.abs(ref))))


# ---------------------------------------------------------------------------------------------------------------------------------------------
def walk(dm, theta, dims, env, x0, T, gamma, eps=None, dtype=np.float64, mut=None, grad=True):
    """build_policy_graph's unrolled rollout and its adjoint, as oracle/bptt_oracle.py states them, in `dtype` throughout; eps [K, T, B, na]:
    u = clip(mean + eps exp(log_std)) and the log_std slots (tests/bptt_stochastic_ref.py).  Also -> sites: name -> [B, n] signed distances of every
    kink argument from its kink, over all models and steps.
    mut (the wrong results of tests/test_bptt_cases.py): ('gamma',) weight gamma^(t+1); ('drop', b) env b contributes nothing; ('terminal',) the
    terminal state's row of the VJP carries step 0's mean adjoint
    (always of non-zero weight); ('done', b) env b's done flag is never set (b = None: nobody's)."""
    f = dtype
    th = np.asarray(theta, dtype=f)
    Ws, bs, log_std = O.policy_unflatten(th, dims)
    d = dm.astype(f)
    K, B, ns, na, L = d.K, x0.shape[0], d.ns, d.na, len(d.Ws)
    kind = mut[0] if mut else None
    std = np.exp(log_std) if eps is not None else None
    costs = np.zeros(K)
    gWs = [np.zeros_like(W) for W in Ws]; gbs = [np.zeros_like(b) for b in bs]; gls = np.zeros(na, f)
    nsat = np.zeros((B, na), np.int64)
    sites = {}

    def site(name, a):
        sites.setdefault(name, []).append(np.asarray(a, np.float64).reshape(B, -1))

    for k in range(K):
        xs, us, ups, dyn_hs, pol_hs, ws = [np.asarray(x0, dtype=f)], [], [], [], [], []
        dones = np.zeros(B, f)
        for t in range(T):
            x = xs[-1]
            mu, hs_p = O._policy_forward(Ws, bs, x)
            up = mu + np.asarray(eps[k, t], dtype=f) * std if eps is not None else mu
            u = np.clip(up, -1.0, 1.0)
            nsat += (np.abs(u) == 1.0)
            site('clip', np.abs(up) - 1.0)
            h = ((np.concatenate([x, u], axis=1) - d.in_mean) / d.in_std)[:, d.n_drop:]
            hs_d = [h]
            for l in range(L):
                h = h @ d.Ws[l][k] + d.bs[l][k]
                if l < L - 1:
                    if d.acts[l] == 'relu':                          # the only hidden activation with a kink
                        site('relu', h)
                    h = O._ACTS[d.acts[l]](h); hs_d.append(h)
            xn = d.diff_mean[:ns] + d.diff_std[:ns] * h + x
            if env == 'half_cheetah':
                site('hc_inner', np.abs(xn[:, 9] - f(1e-1 * 0.5) * np.sum(np.square(u), axis=1)) - 10.0)
            elif env == 'hopper':
                site('hopper_045', 0.45 - xn[:, 0]); site('hopper_02', np.abs(xn[:, 1]) - 0.2); site('hopper_100', np.abs(xn[:, 2:]) - 100.0)
            elif env == 'ant':
                site('ant_lo', xn[:, 2] - 0.2); site('ant_hi', 1.0 - xn[:, 2])
            c = O.cost_np_vec(env, x, u, xn)
            gt = f(gamma ** (t + 1 if kind == 'gamma' else t))
            w = gt * (1 - dones) / f(B) if env == 'ant' else np.full(B, gt / f(B), f)
            if kind == 'drop':
                w = w.copy(); w[mut[1]] = 0
            costs[k] += np.sum((w * c).astype(np.float64))
            if env == 'ant':
                dn = O.is_done(env, x, xn).astype(f)
                if kind == 'done':
                    if mut[1] is None:
                        dn[:] = 0
                    else:
                        dn[mut[1]] = 0
                dones = np.maximum(dones, dn)
            xs.append(xn); us.append(u); ups.append(up); dyn_hs.append(hs_d); pol_hs.append(hs_p); ws.append(w / f(K))
        if not grad:
            continue
        lam = np.zeros((B, ns), f)
        for t in range(T - 1, -1, -1):
            gu_c, gx_c = Bp._cost_grads(env, us[t], xs[t + 1], ws[t])
            gs, gu_d = Bp._dyn_vjp(d, k, dyn_hs[t], lam + gx_c)
            gmu = ((gu_c + gu_d) * ((ups[t] >= -1.0) & (ups[t] <= 1.0))).astype(f)
            if kind == 'terminal' and t == 0:
                gW, gb = O._backward(Ws, O._policy_forward(Ws, bs, xs[T])[1], gmu)
                for l in range(len(Ws)):
                    gWs[l] += gW[l]; gbs[l] += gb[l]
            gW, gb = O._backward(Ws, pol_hs[t], gmu)
            for l in range(len(Ws)):
                gWs[l] += gW[l]; gbs[l] += gb[l]
            if eps is not None:
                gls += np.sum(gmu * np.asarray(eps[k, t], dtype=f), axis=0) * std
            dh = gmu @ Ws[-1].T
            for l in range(len(Ws) - 2, -1, -1):
                dh = (dh * (1 - np.square(pol_hs[t][l + 1]))) @ Ws[l].T
            lam = (gs + dh).astype(f)
    return dict(costs=costs, grad=np.asarray(O.policy_flatten(gWs, gbs, gls), np.float64), nsat=nsat,
                sites={n: np.concatenate(a, axis=1) for n, a in sites.items()})


def guard(dm, theta, dims, env, x0, T, gamma, eps):
    """The kink guard: the walk in float64 and in float32 beside it.  -> (ok [B]: same branch at every site and the float64 argument at least
    KINK_FACTOR x the float32 - float64 difference of that argument from the kink; margin [B]: the smallest |argument| / difference of the env)."""
    a64 = walk(dm, theta, dims, env, x0, T, gamma, eps, np.float64, grad=False)['sites']
    a32 = walk(dm, theta, dims, env, x0, T, gamma, eps, np.float32, grad=False)['sites']
    B = x0.shape[0]
    ok, margin = np.ones(B, bool), np.full(B, np.inf)
    for n in a64:
        diff = np.abs(a32[n] - a64[n])
        ok &= np.all((np.sign(a32[n]) == np.sign(a64[n])) & (a64[n] != 0) & (np.abs(a64[n]) >= KINK_FACTOR * diff), axis=1)
        margin = np.minimum(margin, np.min(np.abs(a64[n]) / np.maximum(diff, 1e-300), axis=1))
    return ok, margin


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _slot_state(case, pool_row, slot):
    """The candidate pool row as slot `slot` of the case's x0: the scaled-up states and populated cost kinks of tests/test_gpu_bptt.py for hopper
    and half_cheetah (its first-10 / next-10 / next-4 pattern dealt out by slot so that every B has them), Ant's done envs."""
    x = pool_row.copy()
    if case.env in ('hopper', 'half_cheetah'):
        x *= 3.0
    if case.env == 'hopper':
        if slot % 8 == 1: x[1] = 0.5
        if slot % 8 == 3: x[0] = 0.2
        if slot % 8 == 5: x[4] = 150.0
    if (case.variant == 'ant_tile' and slot < 16) or case.variant == 'ant_all':
        x[2] = 0.15                                             # done at the step-0 transition
    return x


_DATA = {}


def problem(case):
    """The problem of the case's shape (one per (env, K, widths): the GPU test keeps one engine per shape); the case's own seed draws the policy
    perturbation, the noise and the order of the pool."""
    return Hh.problem_data(case.env, case.K, case.dh, case.ph, seed=300 + FUSED_ENVS.index(case.env) if case.env in FUSED_ENVS else 306)


def case_data(case):
    """-> dict(dm (fp32-rounded, float64), th, pdims, x0 [B, ns] fp32 values, eps [K, T, B, na] fp32 values or None, replaced, margin); cached."""
    if case.id in _DATA:
        return _DATA[case.id]
    dm, theta, pdims, pool = problem(case)
    rng = np.random.RandomState(case.seed + 7)
    pool = pool[rng.permutation(len(pool))]
    na = dm.na
    theta = theta + (0.05 if len(case.ph) == 3 else 0.25) * rng.randn(theta.size)          # some actions saturate the clip
    theta[-na:] = rng.uniform(-1.2, 0.3, size=na) if case.stoch else 0.0
    if case.variant == 'clipped':                               # every mean clearly outside [-1, 1], both sides
        Ws, bs, ls = O.policy_unflatten(theta, pdims)
        bs[-1][:] = 12.0 * (1 - 2 * (np.arange(na) % 2))
        theta = O.policy_flatten(Ws, bs, ls)
    th, dm = f32(theta), dm.astype(np.float32).astype(np.float64)
    B, T = case.B, case.T
    eps = f32(rng.randn(case.K, T, B, na)) if case.stoch else None
    if case.variant != 'clipped':                               # slot 0 has an action inside the clip at step 0 of model 0: B = 1 keeps a gradient
        cand = np.stack([f32(_slot_state(case, p, 0)) for p in pool])
        inside = walk(dm, th, pdims, case.env, cand, 1, case.gamma, None if eps is None else np.repeat(eps[:, :1, :1], len(pool), axis=2),
                      grad=False)['sites']['clip'][:, :na] < 0
        first = int(np.flatnonzero(inside.any(axis=1))[0])
        pool[[0, first]] = pool[[first, 0]]
    x0 = np.stack([f32(_slot_state(case, pool[b], b)) for b in range(B)])
    ok, margin = guard(dm, th, pdims, case.env, x0, T, case.gamma, eps)
    nxt, replaced = B, 0
    while not ok.all():
        bad = np.flatnonzero(~ok)
        replaced += len(bad)
        if nxt + len(bad) > len(pool) or replaced > MAX_REPLACED * B:
            break                                               # (the conditions are asserted by tests/test_bptt_cases.py, from these figures)
        for j, b in enumerate(bad):
            x0[b] = f32(_slot_state(case, pool[nxt + j], b))
        nxt += len(bad)
        ok2, m2 = guard(dm, th, pdims, case.env, x0[bad], T, case.gamma, None if eps is None else eps[:, :, bad])
        ok[bad], margin[bad] = ok2, m2
    d = dict(case=case, dm=dm, th=th, pdims=pdims, x0=x0, eps=eps, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _DATA[case.id] = d
    return d


def reference(d):
    """The float64 reference of a case: (costs [K], grad [P], n_saturates [B, na] or None); cached in d."""
    if 'ref' not in d:
        c = d['case']
        if c.stoch:
            import bptt_stochastic_ref as R
            d['ref'] = R.stochastic_costs_and_grad(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma, d['eps'])
        else:
            d['ref'] = Bp.policy_costs_and_grad(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma) + (None,)
    return d['ref']


def restated(d, dtype=np.float64, mut=None):
    c = d['case']
    return walk(d['dm'], d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma, d['eps'], dtype, mut)
