"""The case table of tests/test_gpu_update_kernels.py and its float64 side, on the CPU alone (tests/test_update_cases.py checks the table,
the PPO near-bound cap and that the bounds discriminate, without the library).

A case is (family, env, policy hidden layers, N, mask).  Where an N follows from the launch rule (the block count of the fused kernels, the CU
count behind the generic kernels' grid) it is symbolic here: the GPU test derives it from what the library reports of its launches
(Engine.last_update_launch), the CPU test takes its nominal value -- the rule's result on an MI355X (256 CUs, 8 tiles per fused block).
The problem of a case is helpers.update_data (= test_gpu_engine._update_problem without the engine), everything rounded to fp32 on both sides;
the references are oracle.metrpo_oracle, vpg_ref and ppo_ref; the near-bound masking is test_gpu_ppo's (BAND, CAP, near_bound)."""
from collections import namedtuple

import numpy as np
from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import vpg_ref
import ppo_ref
from test_gpu_ppo import BAND, CAP, near_bound      # noqa: F401  (BAND is part of near_bound; re-exported for the tests)

METRPO_MAX_LAYERS = 6                # include/metrpo.h
CLIP_LR = 0.3
ENT_COEFFS = (0.0, 0.01)
TRIAL_SCALE = 0.02                   # trial theta = theta + 0.02 randn
NOMINAL_CUS = 256
MASKS = ('none', 'seven', 'edges', 'one')
FUSED_ENVS = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant')       # policy_mfma.hip's table, in its order
# family -> set_update_path argument, expected update_path(N)
PATHS = {'mfma': (True, 'mfma'), 'fused3': (True, 'mfma'), 'generic': (False, 'generic'), 'gemm': ('gemm', 'gemm')}

Case = namedtuple('Case', 'id family env ph nspec mask seed')


def nominal_n(nspec):
    """N of a case on an MI355X with the default launch rule; an int is itself."""
    if isinstance(nspec, int):
        return nspec
    kind, arg = nspec
    if kind == 'two_blocks':         # fused 2 x 32: the smallest N with two blocks and a partial last tile (8 tiles per block: 9 tiles)
        return 8 * 16 + 1
    if kind == 'deal':               # ... the smallest N with >= arg blocks at which waves 4-7 of every block own a tile, last tile partial
        return {1: 4 * 16 + 1, 2: 12 * 16 + 1}[arg]
    if kind == 'full':               # generic kernels: past the grid cap of 2 blocks per CU, with a partial tile
        return 2 * arg * NOMINAL_CUS + 3
    raise ValueError(nspec)


def _nname(nspec):
    return 'N%d' % nspec if isinstance(nspec, int) else '%s%d' % nspec


def _build():
    shapes = []                                                            # (family, env, ph, [nspec])
    for env in FUSED_ENVS:
        shapes.append(('mfma', env, (32, 32), [1, 15, 16, 17, 129, ('two_blocks', 0), ('deal', 1), ('deal', 2)]))
    shapes.append(('fused3', 'humanoid', (100, 50, 25), [1, 15, 17, 129]))        # (N = 16: tests/test_gpu_fused3.py)
    # generic kernels, forced: the sample tile PT the widest operation of the shape lands on (asserted from the reported launch)
    for env, ph, pt in (('swimmer', (32, 32), 128), ('humanoid', (100, 50, 25), 64), ('swimmer', (256, 128), 32)):
        shapes.append(('generic', env, ph, [1, pt - 1, pt, pt + 1, ('full', pt)]))
    for ph in ((), (3,), (17,), (30, 21, 10), (65, 33), (128, 64), (24, 24, 24, 24)):
        shapes.append(('gemm', 'swimmer', ph, [1, 15, 17, 63, 65, 4099]))
    shapes.append(('gemm', 'hopper', (17,), [1, 15, 17, 63, 65, 4099]))       # na = 3, padded to 4
    cases = []
    for family, env, ph, ns in shapes:
        for nspec in ns:
            n = nominal_n(nspec)
            for mask in MASKS:
                if (mask == 'seven' and n < 2) or (mask == 'edges' and n < 33) or (mask == 'one' and n < 17):      # (valid[::7] = 0 leaves nothing of N = 1)
                    continue
                cid = '%s-%s-%s-%s-%s' % (family, env, 'x'.join(str(h) for h in ph) or 'nohidden', _nname(nspec), mask)
                cases.append(Case(cid, family, env, ph, nspec, mask, SEEDS.get(cid, 1000 + len(cases))))
    return cases


# Seeds are 1000 + the case's index, except where that draw puts a sample's float64 PPO ratio within BAND of 1 +- CLIP_LR in a case with N <= 129
# (the issue asks for none there) or more than CAP of them in a larger one: those cases take the next seed that does not (found on the
# reference alone; tests/test_update_cases.py::test_ppo_near_bound_cap checks every case).
SEEDS = {'mfma-swimmer-32x32-deal1-seven': 5170, 'gemm-swimmer-65x33-N65-none': 7610}
CASES = _build()


def make_mask(mask, N):
    """-> uint8 [N] or None (no `valid` pointer)."""
    if mask == 'none':
        return None
    valid = np.ones(N, np.uint8)
    if mask == 'seven':
        valid[::7] = 0
    elif mask == 'edges':                                   # first sample, last sample and one whole 16-sample tile
        valid[0] = 0; valid[-1] = 0; valid[16:32] = 0
    elif mask == 'one':                                     # exactly one valid sample, inside a tile
        valid[:] = 0; valid[(N * 5) // 7] = 1
    else:
        raise ValueError(mask)
    return valid


def blocks(pdims):
    """[(name, slice)] of the variables W_l, b_l, log_std in the flat parameter vector."""
    out, o = [], 0
    for l, (i, j) in enumerate(zip(pdims[:-1], pdims[1:])):
        out.append(('W%d' % l, slice(o, o + i * j))); o += i * j
        out.append(('b%d' % l, slice(o, o + j))); o += j
    out.append(('log_std', slice(o, o + pdims[-1])))
    return out


def vector_use(got, ref, row, pdims):
    """Worst share of its bound a gradient / FVP uses: whole-vector rel-L2 against `row` and every block against TOL.block_bound.
    -> (worst share, name of the worst check, whole-vector share); <= 1 passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    whole = float(np.linalg.norm(got - ref) / max(row * np.linalg.norm(ref), 1e-300))
    worst, name = whole, 'whole'
    for nm, sl in blocks(pdims):
        bound = TOL.block_bound(row, ref[sl], ref)
        use = float(np.linalg.norm(got[sl] - ref[sl]) / max(bound, 1e-300))
        if use > worst:
            worst, name = use, nm
    if not np.all(np.isfinite(got)):
        worst, name = float('inf'), 'non-finite'
    return worst, name, whole


def case_data(case, N=None):
    """The data and float64 references of a case (N: the derived N of a symbolic case; default its nominal one)."""
    N = nominal_n(case.nspec) if N is None else int(N)
    dm, th, pdims, obs, act, adv, om, ols = Hh.update_data(case.env, N, seed=case.seed, pol_hidden=case.ph)
    rng = np.random.RandomState(case.seed + 7)
    if N == 1:                                              # (one centred advantage is 0: every gradient would be 0 = 0)
        adv = rng.randn(1).astype(np.float32).astype(np.float64)
    th2 = (th + TRIAL_SCALE * rng.randn(th.size)).astype(np.float32).astype(np.float64)
    v = rng.randn(th.size)
    valid = make_mask(case.mask, N)
    keep = np.ones(N, bool) if valid is None else valid.astype(bool)
    ratio = ppo_ref.ratios(th2, pdims, obs, act, om, ols)[0]
    near = near_bound(ratio, CLIP_LR) & keep
    valid_ppo = valid
    if near.any():
        valid_ppo = keep.astype(np.uint8); valid_ppo[near] = 0
    return dict(case=case, N=N, dm=dm, th=th, th2=th2, v=v, pdims=pdims, obs=obs, act=act, adv=adv, om=om, ols=ols, valid=valid, keep=keep,
                valid_ppo=valid_ppo, removed=int(near.sum()), n_valid=int(keep.sum()), ratio=ratio)


def references(d, valid='case'):
    """name -> float64 reference.  Gradients as (loss, g), loss_kl as (loss, kl), fvp as the vector.  `valid`: another mask than the case's."""
    if isinstance(valid, str):
        valid, valid_ppo = d['valid'], d['valid_ppo']
    else:
        valid_ppo = valid
    keep = np.ones(d['N'], bool) if valid is None else np.asarray(valid).astype(bool)
    th, th2, pd = d['th'], d['th2'], d['pdims']
    sel = tuple(d[k][keep] for k in ('obs', 'act', 'adv', 'om', 'ols'))
    ref = {'loss_grad': O.surrogate_loss_grad(th, pd, *sel),
           'fvp': O.fisher_vector_product(th, pd, sel[0], d['v'], reg_coeff=0.0),
           'loss_kl_old': O.surrogate_loss_kl(th, pd, *sel),
           'loss_kl_trial': O.surrogate_loss_kl(th2, pd, *sel),
           'vpg': vpg_ref.loss_grad(th, pd, d['obs'], d['act'], d['adv'], valid=valid)}
    for i, ent in enumerate(ENT_COEFFS):
        ref['ppo%d' % i] = ppo_ref.loss_grad(th2, pd, d['obs'], d['act'], d['adv'], d['om'], d['ols'], CLIP_LR, ent, valid_ppo)[:2]
    return ref
