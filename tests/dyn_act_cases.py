"""Case table and float64 side of tests/test_gpu_dyn_act.py: dynamics nets whose hidden layers are tanh or identity (the reference's
dynamics_model.nonlinearity, one activation per hidden layer, training.py:156-208) on every entry point that reads the ensemble.  CPU only; never imports
the library.  tests/test_dyn_act_cases.py holds the table to its own promises (coverage, first-layer scale, kink shares, and that every bound fails a net
with the wrong activation).

Every fused family is written for relu and declines anything else, so a non-relu net runs on the fallbacks: the thread-per-env rollout and metrpo_step
(act_apply), the step-wise tile GEMMs (EPI_BIAS_TANH / EPI_BIAS_ID), the skinny split-K reduce (its `act`), the bf16 layer GEMMs (`act`), the generic BPTT
sweeps (dact), the generic SVG and scoring sweeps.  A case names the family the library must REPORT for it; the GPU test asserts it.

VARIANTS: the six two-layer nets TWO and the three-layer net THREE.  The float64 side is the suite's own, all of which read dm.acts: oracle.dynamics_forward_all,
helpers.oracle_rollout through rollout_check._check, oracle.bptt_oracle, tests/bptt_stochastic_ref.py, tests/terminal_value_ref.py (the four scoring calls, with
and without a terminal value), tests/rollout_actions_ref.py, tests/model_error_ref.py, tests/disagreement_ref.py, tests/svg_ref.py,
oracle.dynamics_oracle.validation_losses, tests/dyn_bf16_ref.py.  Weights, normalisers, pool and theta are rounded to fp32 before anything is computed.

First-layer scale.  Xavier weights on pool states of size 0.1 give first-layer pre-activations of |z| ~ 0.1 - 0.3, where tanh(z) = z - z^3 / 3 is the
identity to 1e-3 relative and the two activations differ by less than many bounds times a small output weight.  gain_first_layer() multiplies W_0 and b_0 by
1 / median |z_0| (over the pool rows under the policy's clipped mean action), so that the median |z_0| is 1: on every problem of this table at least
MIN_NEAR_SHARE = 0.5 of the first-layer pre-activations have 0.5 <= |z| <= 2 (measured 0.57 ... 0.71; tests/test_dyn_act_cases.py asserts it per problem).

Mutations (mutations(acts)): one layer's activation replaced by each of the other two; the activations in reverse order (where that is another net); and, in
the adjoint only (adjoint_mutation), relu' used for a tanh layer and tanh' left out.  Every mutation must miss every bound of every case it applies to.

Kink guards as in tests/bptt_cases.py and tests/terminal_value_cases.py (clip, cost, done; relu where a layer is relu), with at most MAX_REPLACED = 5 % of a
case's rows replaced.

Bounds: the rows of tests/tolerances.py, none new.  Rollout and step: STEP up to 96 hidden units, WIDE beyond (wide_rollout_cases.state_tol), ACTION, REWARD;
BPTT_COST, BPTT_GRAD_REL_L2 whole and per variable; GRAD_REL_L2 (svg); DYN_LOSS; the supplied-action calls on their own files' bounds."""
import collections
import contextlib

import numpy as np

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from oracle import dynamics_oracle as D
import helpers as Hh
import tolerances as TOL
import rollout_cases as RC
import wide_rollout_cases as WR
import bptt_cases as BC
import score_grad_cases as GC
import score_grad_ref as G0
import terminal_value_cases as TC
import svg_cases as SV
import svg_ref as SR
from rollout_check import _check

ACTS = ('relu', 'tanh', 'identity')
TWO = (('tanh', 'tanh'), ('identity', 'identity'), ('tanh', 'relu'), ('relu', 'tanh'), ('relu', 'identity'), ('identity', 'tanh'))
THREE = ('tanh', 'identity', 'relu')
VARIANTS = TWO + (THREE,)
NEAR = (0.5, 2.0)
MIN_NEAR_SHARE = 0.5
MAX_REPLACED = 0.05                  # of a case's rows
MODES = RC.MODES
H32 = (32, 32)

f32 = RC.f32


def tag(acts):
    return '-'.join(acts)


# ---- the first-layer scale ---------------------------------------------------------------------------------------------------------------------------
def first_layer_z(dm, theta, pdims, states):
    """[K, n, width]: first-layer pre-activations of every head at `states` under the policy's clipped mean action."""
    a = np.clip(O.policy_mean(theta, pdims, states), -1.0, 1.0)
    x = ((np.concatenate([states, a], axis=1) - dm.in_mean) / dm.in_std)[:, dm.n_drop:]
    return np.matmul(x, dm.Ws[0]) + dm.bs[0][:, None, :]


def gain_first_layer(dm, theta, pdims, pool):
    """W_0, b_0 *= 1 / median |z_0| (in place): the median first-layer pre-activation has |z| = 1."""
    g = 1.0 / np.median(np.abs(first_layer_z(dm, theta, pdims, pool)))
    dm.Ws[0] = dm.Ws[0] * g; dm.bs[0] = dm.bs[0] * g


def near_share(dm, theta, pdims, states):
    z = np.abs(first_layer_z(dm, theta, pdims, states))
    return float(np.mean((z >= NEAR[0]) & (z <= NEAR[1])))


# ---- mutations -------------------------------------------------------------------------------------------------------------------------------------------
ADJOINT_MUTATIONS = ('relu_prime_in_tanh', 'tanh_prime_left_out')


def mutations(acts):
    """[(name, wrong activations)]: one layer replaced by each of the other two; the reverse order where that is another net."""
    out = []
    for l, a in enumerate(acts):
        for b in ACTS:
            if b != a:
                out.append(('layer%d_%s' % (l, b), acts[:l] + (b,) + acts[l + 1:]))
    if tuple(reversed(acts)) != tuple(acts):
        out.append(('exchanged', tuple(reversed(acts))))
    return out


def adjoint_mutations(acts):
    return ADJOINT_MUTATIONS if 'tanh' in acts else ()


def with_acts(dm, acts):
    """The same weights under other activations."""
    return O.DynamicsEnsemble(dm.Ws, dm.bs, list(acts), dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std, dm.n_drop, dm.ns, dm.na)


@contextlib.contextmanager
def adjoint_mutation(kind):
    """Inside the block the adjoints of oracle/bptt_oracle.py, tests/score_grad_ref.py (and the restatements built on it) and tests/svg_ref.py use a wrong
    derivative for tanh layers: relu' = [h > 0], or none at all.  The forward passes are untouched."""
    assert kind in ADJOINT_MUTATIONS
    wrong = (lambda h: (h > 0).astype(h.dtype)) if kind == 'relu_prime_in_tanh' else (lambda h: np.ones_like(h))
    saved = (Bp._dact, G0._act_deriv, SR._dact)
    patch = lambda orig: (lambda name, h: wrong(h) if name == 'tanh' else orig(name, h))
    Bp._dact, G0._act_deriv, SR._dact = patch(saved[0]), patch(saved[1]), patch(saved[2])
    try:
        yield
    finally:
        Bp._dact, G0._act_deriv, SR._dact = saved


# ---- 1. metrpo_rollout and metrpo_step ---------------------------------------------------------------------------------------------------------------------
Shape = collections.namedtuple('Shape', 'name env K hidden family variants opts exclusive')


def _shapes():
    out = []
    add = lambda name, env, K, hidden, family, variants, opts=(), exclusive=False: out.append(Shape(name, env, K, tuple(hidden), family, tuple(variants), dict(opts), exclusive))
    add('thread-12x12', 'swimmer', 3, (12, 12), 'generic', TWO)                          # a width below 16: the thread-per-env kernel (act_apply)
    add('tile-64x64-hc', 'half_cheetah', 2, (64, 64), 'gemm-stepwise', TWO)              # cooperative with relu
    add('tile-64x64-ant', 'ant', 3, (64, 64), 'gemm-stepwise', TWO)                      # cooperative with relu; early dones
    add('tile-96x96', 'swimmer', 1, (96, 96), 'gemm-stepwise', (('tanh', 'tanh'), ('relu', 'identity'), ('tanh', 'relu')))
    add('tile-128x128', 'ant', 2, (128, 128), 'gemm-stepwise', (('tanh', 'tanh'), ('tanh', 'relu'), ('relu', 'tanh'), ('relu', 'identity')))   # contraction 128: no split
    add('tile-128x128x128', 'snake', 3, (128, 128, 128), 'gemm-stepwise', (THREE,))
    # contraction 256 in front of a tanh / identity layer: gemm_skinny_bias splits it (k_splitk_bias_reduce with act != 0).  stream-K mode 1 with relu; forced, it must stay off
    add('split-256x256', 'hopper', 2, (256, 256), 'gemm-stepwise', (('tanh', 'tanh'), ('relu', 'tanh'), ('relu', 'identity')), opts=dict(STREAMK='1'))
    add('wide-512x512', 'swimmer', 1, (512, 512), 'gemm-stepwise', (('tanh', 'tanh'),), exclusive=True)     # resident with relu on an exclusive context
    add('narrow-48x20', 'swimmer', 3, (48, 20), 'gemm-stepwise', (('tanh', 'tanh'), ('relu', 'tanh')))      # zero-padded cooperative with relu
    return out


SHAPES = _shapes()
SHAPE = {s.name: s for s in SHAPES}
ROLLOUTS = [(s.name, a) for s in SHAPES for a in s.variants]
STEP_SHAPES = ('thread-12x12', 'tile-64x64-hc')
ROLL_T, ROLL_H = 3, 2


def rollout_cases(name, acts):
    """B = 17 in all six modes; B = 1 and B = 65 in one rotating mode; a deterministic policy; chunks (2, 1), bitwise the one call."""
    s = SHAPE[name]
    base = SHAPES.index(s) + s.variants.index(tuple(acts))
    rot = lambda j: MODES[(base + j) % len(MODES)]
    mk = lambda nm, B, mode, determ=False, chunks=None, resets=False: RC.Case(nm, B, ROLL_T, ROLL_H, mode, determ, chunks, False, True, resets)
    out = [mk('all-modes', 17, m, resets=True) for m in MODES]
    out += [mk('edges', 1, rot(0)), mk('edges', 65, rot(1), resets=True)]
    out += [mk('determ', 17, rot(2), determ=True), mk('chunked', 17, rot(3), chunks=(2, 1), resets=True)]
    return out


class Problem(RC.Problem):
    """rollout_cases.Problem under per-layer activations, the first layer scaled; bounds by width as tests/wide_rollout_cases.py deals them."""

    def __init__(self, env, K, hidden, acts, pol=H32):
        RC.Problem.__init__(self, env, K, hidden, pol, row=TOL.wide_or_step(hidden), dyn_act=tuple(acts), shape=gain_first_layer)
        self.acts = tuple(acts)
        assert tuple(self.dm.acts) == self.acts
        self.tol = WR.state_tol(hidden)
        self.mean_tol = TOL.wide_or_step(pol)
        self.act_tol = TOL.ACTION


_PROBLEMS = {}


def problem(name, acts):
    key = (name, tuple(acts))
    if key not in _PROBLEMS:
        s = SHAPE[name]
        _PROBLEMS[key] = Problem(s.env, s.K, s.hidden, acts)
    return _PROBLEMS[key]


def check_rollout(p, c, dev, label, form=None):
    dr, rad, _ = p.draws(c)
    _check(p, dev, dr, rad, c.B, c.T, c.H, c.mode, c.determ, label, own=(), expect_resets=c.expect_resets, ant_free_run=True, form=form,
           act_tol=p.act_tol, rew_tol=p.tol, mean_tol=p.mean_tol)


def hidden_splits(hidden, acts, nin, B, K):
    """[(layer, splits)] of the hidden layers gemm_skinny_bias runs as split-K partials + k_splitk_bias_reduce (its `act` argument): skinny_splits restated."""
    out = []
    dims = [(nin + 3) & ~3] + list(hidden)
    for l in range(len(hidden)):
        S = WR._skinny_out_splits(B, dims[l + 1], dims[l], K)
        if S > 1:
            out.append((l, S))
    return out


def expect_launch(s, acts, B):
    """Fields of Engine.last_rollout_launch a tile-GEMM launch of this net must report: no stream-K mode, no persistent or resident launch; the fused output tile
    only behind a relu layer; else the output layer's own split-K partials."""
    ns = O.ENV_SPECS[s.env][0]
    fuse = WR._fused_out_tile(B, s.hidden[-1], s.K, ns) if acts[-1] == 'relu' else 0
    splits = s.hidden[-1] // (64 * fuse) if fuse else WR._skinny_out_splits(B, ns, s.hidden[-1], s.K)
    return dict(family='gemm-stepwise', sk_mode=0, late=0, fuse_tile=fuse, out_splits=splits, persist_wide=0, nclose=0, rounds='single', res_ws=0, res_threads=0, res_pw=0,
                res_rg=0, res_rot=0)


def step_ref(p, s, a, mode, idx, noise):
    """metrpo_step in float64: -> (next, reward, done, all heads)"""
    ac = np.clip(a, -1.0, 1.0)
    heads = O.dynamics_forward_all(p.dm, s, ac)
    nxt = O.select_next(heads, mode, idx, noise)
    return nxt, -O.cost_np_vec(p.env, s, ac, nxt), O.is_done(p.env, nxt, nxt), heads


# bf16 operands: the measured-bound rule of tests/dyn_bf16_ref.py (random_bound) on the same case under other activations
BF16_HIDDEN = (128, 128)
BF16_VARIANTS = (('tanh', 'tanh'), ('tanh', 'relu'), ('relu', 'tanh'))


# ---- 2. the BPTT sweeps --------------------------------------------------------------------------------------------------------------------------------------
BPTT_SHAPES = (('swimmer', 2, (64, 64)), ('half_cheetah', 2, (64, 64)), ('swimmer', 2, (128, 128)))
BPTT_BT = ((1, 3), (17, 3), (65, 3), (17, 1))
BPTT_GAMMA = 0.97
BpttCase = collections.namedtuple('BpttCase', 'id env K dh ph acts B T gamma stoch seed')
BPTT_SEEDS = {}


def _bptt():
    out = []
    for env, K, dh in BPTT_SHAPES:
        for acts in TWO:
            for B, T in BPTT_BT:
                for stoch in (False, True):
                    cid = '%s-%s-%s-B%d-T%d%s' % (env, 'x'.join(map(str, dh)), tag(acts), B, T, '-stoch' if stoch else '')
                    out.append(BpttCase(cid, env, K, dh, H32, acts, B, T, BPTT_GAMMA, stoch, BPTT_SEEDS.get(cid, 9000 + len(out))))
    return out


BPTT_CASES = _bptt()
_BPTT_PROBLEMS, _BPTT_DATA = {}, {}


def net_problem(env, K, dh, acts, seed, n_pool=257):
    """(dm, theta, pdims, pool): helpers.problem_data under `acts`, first layer scaled, everything rounded to fp32."""
    dm, theta, pdims, pool = Hh.problem_data(env, K, dh, H32, seed=seed, n_pool=n_pool, dyn_act=tuple(acts))
    gain_first_layer(dm, theta, pdims, pool)
    return dm.astype(np.float32).astype(np.float64), f32(theta), pdims, f32(pool)


def bptt_problem(c):
    key = (c.env, c.K, c.dh, c.acts)
    if key not in _BPTT_PROBLEMS:
        _BPTT_PROBLEMS[key] = net_problem(c.env, c.K, c.dh, c.acts, seed=310 + BC.FUSED_ENVS.index(c.env))
    return _BPTT_PROBLEMS[key]


def bptt_data(c):
    """tests/bptt_cases.case_data for these nets: -> dict(case, dm, th, pdims, x0, eps, replaced, accepted, margin); cached."""
    if c.id in _BPTT_DATA:
        return _BPTT_DATA[c.id]
    dm, theta, pdims, pool = bptt_problem(c)
    rng = np.random.RandomState(c.seed + 7)
    pool = pool[rng.permutation(len(pool))]
    na = dm.na
    theta = theta + 0.25 * rng.randn(theta.size)                  # some actions saturate the clip
    theta[-na:] = rng.uniform(-1.2, 0.3, size=na) if c.stoch else 0.0
    th = f32(theta)
    eps = f32(rng.randn(c.K, c.T, c.B, na)) if c.stoch else None
    # slot 0 has an action inside the clip at step 0 of model 0: B = 1 keeps a gradient
    inside = BC.walk(dm, th, pdims, c.env, pool, 1, c.gamma, None if eps is None else np.repeat(eps[:, :1, :1], len(pool), axis=2), grad=False)['sites']['clip'][:, :na] < 0
    if inside.any():                                              # (else slot 0's draw saturates every pool row; tests/test_dyn_act_cases.py asserts a gradient)
        first = int(np.flatnonzero(inside.any(axis=1))[0])
        pool[[0, first]] = pool[[first, 0]]
    x0 = pool[:c.B].copy()
    ok, margin = BC.guard(dm, th, pdims, c.env, x0, c.T, c.gamma, eps)
    nxt, replaced = c.B, 0
    while not ok.all():
        bad = np.flatnonzero(~ok)
        replaced += len(bad)
        if nxt + len(bad) > len(pool) or replaced > MAX_REPLACED * c.B:
            break                                                 # (asserted by tests/test_dyn_act_cases.py, from these figures)
        x0[bad] = pool[nxt:nxt + len(bad)]
        nxt += len(bad)
        ok2, m2 = BC.guard(dm, th, pdims, c.env, x0[bad], c.T, c.gamma, None if eps is None else eps[:, :, bad])
        ok[bad], margin[bad] = ok2, m2
    d = dict(case=c, dm=dm, th=th, pdims=pdims, x0=x0, eps=eps, replaced=replaced, accepted=int(ok.sum()), margin=float(margin.min()))
    _BPTT_DATA[c.id] = d
    return d


def bptt_reference(d, dm=None):
    """(costs [K], grad [P]) in float64 from the references the suite trusts (oracle.bptt_oracle; tests/bptt_stochastic_ref.py: torch autograd); cached for
    the case's own net, recomputed for another `dm` (a mutated one)."""
    c = d['case']

    def run(net):
        if c.stoch:
            import bptt_stochastic_ref as R
            return R.stochastic_costs_and_grad(net, d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma, d['eps'])[:2]
        return Bp.policy_costs_and_grad(net, d['th'], d['pdims'], c.env, d['x0'], c.T, c.gamma)
    if dm is not None:
        return run(dm)
    if 'ref' not in d:
        d['ref'] = run(d['dm'])
    return d['ref']


def bptt_shares(costs, grad, d):
    """(share of BPTT_COST, share of BPTT_GRAD_REL_L2 on the whole vector, worst share of block_bound over the variables, its name)"""
    rc, rg = bptt_reference(d)
    whole, worst, where, _ = BC.vector_use(grad, rg, d['pdims'])
    return BC.cost_use(costs, rc), whole, worst, where


LBFGS_CASE = ('swimmer', 2, (64, 64), ('tanh', 'tanh'), 17, 3)


# ---- 3. metrpo_svg_grad --------------------------------------------------------------------------------------------------------------------------------------
SVG_NETS = (('swimmer', 2, (64, 64), ('identity', 'identity')), ('swimmer', 2, (64, 64), ('tanh', 'relu')), ('swimmer', 2, (64, 64), ('relu', 'tanh')),
            ('snake', 2, (48, 48, 32), THREE))
SVG_N, SVG_T, SVG_GAMMA, SVG_MODEL = 3, 5, 0.97, 1
_SVG = {}


def svg_data(env, K, dh, acts):
    """tests/svg_cases._case_data for these nets: recorded rollouts clear of every kink (svg_cases.rollout_margin)."""
    key = (env, K, dh, acts)
    if key in _SVG:
        return _SVG[key]
    dm, theta, pdims, pool = net_problem(env, K, dh, acts, seed=7)
    Ws, bs, ls = O.policy_unflatten(theta.copy(), pdims)
    bs[-1][0] += 1.3                                             # action 0's mean beyond the clip bound (svg applies NO clip)
    theta = f32(O.policy_flatten(Ws, bs, ls))
    lens = SV.lengths_of(SVG_N, SVG_T)
    obs = np.zeros((SVG_N, SVG_T + 1, dm.ns)); act = np.zeros((SVG_N, SVG_T, dm.na))
    replaced, margin = 0, np.inf
    for r in range(SVG_N):
        for attempt in range(8):
            rng = np.random.RandomState(700003 + r * 101 + attempt)
            Os, As = SV.draw_rollout(dm, theta, pdims, pool, SVG_MODEL, SVG_T, rng)
            m = SV.rollout_margin(dm, env, SVG_MODEL, Os[:lens[r]], As[:lens[r]])
            if m >= SV.KINK_FACTOR:
                break
            replaced += 1
        else:
            raise AssertionError('%s: no rollout clear of the kinks in 8 draws' % (key,))
        obs[r], act[r], margin = Os, As, min(margin, m)
    d = dict(env=env, acts=acts, dm=dm, theta=theta, pdims=pdims, obs=obs[:, :-1].copy(), obs_next=obs[:, 1:].copy(), act=act, lengths=lens, replaced=replaced,
             margin=margin)
    _SVG[key] = d
    return d


def svg_reference(d, dm=None):
    run = lambda net: SR.svg_gradient(net, d['theta'], d['pdims'], d['env'], d['obs'], d['act'], d['lengths'], model=SVG_MODEL, gamma=SVG_GAMMA, dtype=np.float64,
                                      wrong=None, obs_next=d['obs_next'])
    if dm is not None:
        return run(dm)
    if 'ref' not in d:
        d['ref'] = run(d['dm'])
    return d['ref']


def svg_shares(got, d):
    """(share of GRAD_REL_L2 on theta, worst share of block_bound over the variables, share on the state gradient)"""
    ref = svg_reference(d)
    whole, worst, _ = SV.vector_use(np.asarray(got['theta'], np.float64), ref['theta'], d['pdims'])
    return whole, worst, SV.state_use(np.asarray(got['state'], np.float64), ref['state'])


# ---- 4. metrpo_dyn_eval_losses, metrpo_dyn_train_step ---------------------------------------------------------------------------------------------------------
EVAL_ENV, EVAL_K = 'swimmer', 3
EVAL_NETS = [((64, 64), a) for a in TWO] + [((128, 128), a) for a in TWO] + [((128, 128, 128), THREE)]
EVAL_REGS = (0.0, 1e-3)
_EVAL = {}


def eval_rows(hidden):
    """n = 1, 17, 129; at (64, 64) also 8193: the second 8192-row pass holds one row."""
    return (1, 17, 129) + ((8193,) if tuple(hidden) == (64, 64) else ())


def eval_problem(hidden, acts):
    key = (tuple(hidden), tuple(acts))
    if key not in _EVAL:
        _EVAL[key] = net_problem(EVAL_ENV, EVAL_K, hidden, acts, seed=71)
    return _EVAL[key]


def eval_data(dm, pool, n, seed=9):
    """Validation rows at the scale the first layer was set for: pool states plus noise, actions in [-1, 1], targets near the state; fp32 values."""
    rng = np.random.RandomState(seed + n)
    s = pool[rng.randint(len(pool), size=n)] + 0.02 * rng.randn(n, dm.ns)
    a = np.clip(0.7 * rng.randn(n, dm.na), -1.0, 1.0)
    x = f32(np.concatenate([s, a], axis=1))
    y = f32(x[:, :dm.ns] + 0.1 * rng.randn(n, dm.ns))
    return x, y


def loss_share(got, ref):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (TOL.DYN_LOSS['atol'] + TOL.DYN_LOSS['rtol'] * np.abs(ref))))


TRAIN_REFUSED = (('tanh', 'tanh'), ('relu', 'identity'))


# ---- 5. the supplied-action family ---------------------------------------------------------------------------------------------------------------------------------
# a shape inside the fused class apart from the activations: 2 x 64, K <= 8, a fused env
SUPPLIED_VARIANTS = (('tanh', 'tanh'), ('identity', 'identity'), ('tanh', 'relu'))
SUPPLIED_NETS = (('swimmer', 3), ('half_cheetah', 2))
SUPPLIED_BS = ((17, 1), (33, 3))
SUPPLIED_T = 3
SUPPLIED_SEEDS = {}


def supplied_problem(env, K, acts):
    """(dm, theta, pdims, pool) of a supplied-action net, registered as the problem of its shape in tests/score_grad_cases.py (whose case_data, and that of
    tests/terminal_value_cases.py, then draw on it)."""
    key = (env, K, (64, 64), tuple(acts))
    if key not in GC._PROBLEMS:
        GC._PROBLEMS[key] = net_problem(env, K, (64, 64), acts, seed=500 + GC.FUSED_ENVS.index(env), n_pool=256)
    return GC._PROBLEMS[key]


def _supplied():
    out = []
    for env, K in SUPPLIED_NETS:
        for acts in SUPPLIED_VARIANTS:
            for B, S in SUPPLIED_BS:
                cid = 'act-%s-K%d-%s-B%d-S%d' % (env, K, tag(acts), B, S)
                out.append(TC.Case(cid, 'generic', env, K, (64, 64), tuple(acts), B, SUPPLIED_T, S, 0.99, True, 'plain', SUPPLIED_SEEDS.get(cid, 31000 + len(out)),
                                   S, 'all', bool(len(out) % 2), True))
    return out


SUPPLIED_CASES = _supplied()
SUPPLIED_RUNS = [(c, loop) for c in SUPPLIED_CASES for loop in TC.LOOPS]


def supplied_data(case, loop):
    supplied_problem(case.env, case.K, case.act)
    return TC.case_data(case, loop)


def relu_twin(dm):
    return with_acts(dm, ['relu'] * len(dm.acts))


def rollout_actions_ref(dm, env, init, actions, mode, model=None, model_idx=None, noise=None):
    """metrpo_rollout_actions in every sampling mode, float64, feeding its own state back and never resetting (tests/rollout_actions_ref.py's loop with
    oracle.select_next for the modes the fused kernel does not hold).  -> dict(obs [T + 1, B, ns], rew [T, B], done [T, B])"""
    s = np.asarray(init, np.float64)
    a = np.clip(np.asarray(actions, np.float64), -1.0, 1.0)
    obs, rew, done = [s], [], []
    for t in range(a.shape[0]):
        heads = O.dynamics_forward_all(dm, s, a[t])
        idx = model_idx[t] if mode == 'step_rand' else model
        nxt = O.select_next(heads, mode, idx, None if noise is None else noise[t])
        rew.append(-O.cost_np_vec(env, s, a[t], nxt)); done.append(np.asarray(O.is_done(env, nxt, nxt), bool)); obs.append(nxt)
        s = nxt
    return dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done))


# ---- what the table reaches -----------------------------------------------------------------------------------------------------------------------------------------
def reached():
    """{(entry point, fallback family, variant)} of every case of this file."""
    out = set()
    for name, acts in ROLLOUTS:
        s = SHAPE[name]
        fam = 'thread-per-env' if s.family == 'generic' else 'tile-gemm'
        out.add(('rollout', fam, acts))
        if s.family == 'gemm-stepwise' and any(acts[l] != 'relu' for l, _ in hidden_splits(s.hidden, acts, sum(O.ENV_SPECS[s.env][:2]) - O.ENV_SPECS[s.env][2], 17, s.K)):
            out.add(('rollout', 'skinny-split-reduce', acts))
        if name in STEP_SHAPES:
            out.add(('step', fam, acts))
    for acts in BF16_VARIANTS:
        out.add(('rollout', 'bf16-layer-gemm', acts))
    for c in BPTT_CASES:
        out.add(('bptt_grad_stochastic' if c.stoch else 'bptt_grad', 'generic-sweeps', c.acts))
        if not c.stoch:
            out.add(('validation_cost', 'generic-sweeps', c.acts))
    out.add(('lbfgs_policy', 'generic-sweeps', LBFGS_CASE[3]))
    for env, K, dh, acts in SVG_NETS:
        out.add(('svg_grad', 'generic', acts))
    for hidden, acts in EVAL_NETS:
        out.add(('dyn_eval_losses', 'tile-gemm', acts))
    for acts in TRAIN_REFUSED:
        out.add(('dyn_train_step', 'refused', acts))
    for c in SUPPLIED_CASES:
        for ep in ('rollout_actions', 'model_error', 'ensemble_disagreement'):
            out.add((ep, 'step-loop' if ep != 'ensemble_disagreement' else 'generic', c.act))
        for ep in ('score_actions', 'score_policy_actions', 'score_actions_grad', 'score_policy_actions_grad'):
            out.add((ep, 'generic', c.act)); out.add((ep + '+terminal_value', 'generic', c.act))
    return out
