"""NumPy restatement of metrpo_ensemble_disagreement (include/metrpo.h), float64 arithmetic on the fp32 inputs the device stores, plus the cases and the
bounds tests/test_gpu_disagreement.py and tests/test_disagreement_ref.py share.

    next_possible_observations = dynamics_forward_all(s, clip(a))          # env_helpers.py:612-616, every head
    mean = np.mean(next_possible_observations, axis=0)                      # :621-622
    std  = np.std(next_possible_observations, axis=0)                       # :625 (ddof = 0)
    score = ||std||_2, maxdev = max_k ||s'_k - mean||_2, rew_std = np.std over k of -cost_np_vec(s, clip(a), s'_k)

mode 'f64' is that, in float64.  mode 'f32' follows the device: the heads' next states rounded to fp32 (the forward itself stays the oracle's), the mean as
the f32 sum in head order divided by K, the variance two-pass with fmaf in head order, divided by K, the root; the score's sum over the dims in index
order.  mode 'f32_onepass' replaces the variance by E[x^2] - mean^2 in float32 -- the mistake the offset case exists to catch; used only to show it bites.
"""
import numpy as np

from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL

F = np.float32


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two fp32 numbers is exact in float64, one rounding of the float64 sum to fp32 (double rounding aside)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _pop_std32(x, onepass=False):
    """x [K, ...] float32 -> (mean, variance, std) over axis 0 in float32, the device's order."""
    K = x.shape[0]
    m = np.zeros(x.shape[1:], F)
    for k in range(K):
        m = (m + x[k]).astype(F)
    m = (m / F(K)).astype(F)
    if onepass:
        sq = np.zeros(x.shape[1:], F)
        for k in range(K):
            sq = _fma32(x[k], x[k], sq)
        var = np.maximum((sq / F(K)).astype(F) - (m * m).astype(F), F(0)).astype(F)
    else:
        var = np.zeros(x.shape[1:], F)
        for k in range(K):
            d = (x[k] - m).astype(F)
            var = _fma32(d, d, var)
        var = (var / F(K)).astype(F)
    return m, var, np.sqrt(var).astype(F)


def disagreement(dm, env, obs, actions, valid=None, rows_per_group=0, mode='f64'):
    """obs [N, ns], actions [N, na] unclipped, valid [N] or None.  -> dict(next_all [K, N, ns], mean, std [N, ns], score, maxdev, rew_std [N], rew_all [K, N],
    sums [G, 4]); skipped rows are zero everywhere and left out of sums."""
    s = np.asarray(obs, np.float64)
    a = np.clip(np.asarray(actions, np.float64), -1.0, 1.0)                               # env_helpers.py:599
    N = len(s)
    with np.errstate(all='ignore'):
        nall = O.dynamics_forward_all(dm, s, a)                                           # [K, N, ns]
        rew = np.stack([-O.cost_np_vec(env, s, a, nall[k]) for k in range(dm.K)])         # [K, N]
    if mode == 'f64':
        mean = np.mean(nall, axis=0)
        std = np.std(nall, axis=0)
        score = np.linalg.norm(std, axis=1)
        maxdev = np.max(np.linalg.norm(nall - mean, axis=2), axis=0)
        rew_std = np.std(rew, axis=0)
    else:
        x = nall.astype(F)
        mean, var, std = _pop_std32(x, onepass=(mode == 'f32_onepass'))
        ssq = np.zeros(N, F)
        for d in range(dm.ns):
            ssq = (ssq + var[:, d]).astype(F)
        score = np.sqrt(ssq).astype(F)
        dev = np.zeros((dm.K, N), F)
        for k in range(dm.K):
            for d in range(dm.ns):
                dd = (x[k, :, d] - mean[:, d]).astype(F)
                dev[k] = _fma32(dd, dd, dev[k])
        maxdev = np.max(np.sqrt(dev).astype(F), axis=0)
        rew_std = _pop_std32(rew.astype(F), onepass=(mode == 'f32_onepass'))[2]
    out = dict(next_all=nall, mean=mean, std=std, score=score, maxdev=maxdev, rew_std=rew_std, rew_all=rew)
    v = np.ones(N, bool) if valid is None else (np.asarray(valid) != 0)
    for key in ('mean', 'std', 'score', 'maxdev', 'rew_std'):
        out[key] = np.where(v.reshape((N,) + (1,) * (out[key].ndim - 1)), out[key], 0)
    out['next_all'] = np.where(v[None, :, None], nall, 0)
    out['sums'] = group_sums(out['score'], v, rows_per_group)
    return out


def group_sums(score, valid, rows_per_group):
    """d_sums of a score vector: per group (valid rows, sum, sum of squares, max) in float64."""
    N = len(score)
    rpg = int(rows_per_group) if rows_per_group else N
    G = max(1, -(-N // rpg))
    sums = np.zeros((G, 4))
    for g in range(G):
        sc = np.asarray(score[g * rpg:(g + 1) * rpg], np.float64)[np.asarray(valid[g * rpg:(g + 1) * rpg], bool)]
        sums[g] = (len(sc), sc.sum(), (sc * sc).sum(), sc.max() if len(sc) else 0.0)
    return sums


def bounds(ref, row):
    """Element-wise bounds on |device - ref| from the float64 restatement `ref`; row = tolerances.STEP (fused shapes) or wide_or_step(hidden).
      next_all, mean: the row itself.
      std[d]: atol + rtol (max_k |s'_k[d]| + std[d]) -- the population std is 1-Lipschitz in the heads' errors, so it inherits the per-head bound at the
              largest head; the + std term covers the f32 deviation, sum and root.
      score: the 2-norm over the dims of the std bounds.  maxdev: twice that (head and mean both carry the error).
      rew_std: the std argument with tolerances.REWARD at max_k |r_k|."""
    a, r = row['atol'], row['rtol']
    nall = np.abs(ref['next_all'])
    b = dict(next_all=a + r * nall, mean=a + r * np.abs(ref['mean']))
    b['std'] = a + r * (nall.max(axis=0) + ref['std'])
    b['score'] = np.linalg.norm(b['std'], axis=1)
    b['maxdev'] = 2.0 * b['score']
    b['rew_std'] = TOL.REWARD['atol'] + TOL.REWARD['rtol'] * (np.abs(ref['rew_all']).max(axis=0) + ref['rew_std'])
    return b


def shares(got, ref, row, keys=('next_all', 'mean', 'std', 'score', 'maxdev', 'rew_std')):
    """worst |got - ref| / bound per output"""
    b = bounds(ref, row)
    return {k: float(np.max(np.abs(np.asarray(got[k], np.float64) - ref[k]) / b[k])) if np.size(ref[k]) else 0.0 for k in keys if k in got}


# ---- the problems and inputs of the GPU cases (CPU only: the engines are made by the GPU test) -------------------------------------------------------
#          name           env            K  dynamics hidden  seed
SHAPES = {'swimmer':      ('swimmer',      5, (64, 64), 3),     # ns 10: one output block
          'half_cheetah': ('half_cheetah', 5, (64, 64), 4),     # n_drop 1, ns 18: two output blocks
          'hopper':       ('hopper',       5, (64, 64), 6),     # n_drop 0
          'snake':        ('snake',        5, (64, 64), 7),
          'ant':          ('ant',          5, (64, 64), 5),     # ns 29, more than 64 KB of LDS at K = 8 only
          'swimmer_k1':   ('swimmer',      1, (64, 64), 8),     # K = 1: exact zeros
          'swimmer_k8':   ('swimmer',      8, (64, 64), 9),     # the 8-wave workgroup
          'padded':       ('swimmer',      5, (48, 32), 10),    # the zero-padded copy
          # generic path
          'wide':         ('swimmer',      5, (128, 128), 11),
          'k9':           ('swimmer',      9, (64, 64), 12),
          'humanoid':     ('humanoid',     5, (1024, 1024), 13)}
FUSED = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant', 'swimmer_k1', 'swimmer_k8', 'padded')
GENERIC = ('wide', 'k9', 'humanoid')
POL_HIDDEN = {'humanoid': (100, 50, 25)}
# fused cases (shape, N, rows_per_group): every shape at a partial last tile with a group boundary inside a tile; swimmer at every N of {1, 16, 17, 33}
# with every rows_per_group of {0, 5, 17}; and one size at which a workgroup strides over many tiles (more tiles than any grid: the double-buffered
# exchange area, the prefetch and the output wave's turn all wrap)
STRIDED_N = 50001
FUSED_CASES = [(sh, 33, 5) for sh in FUSED] + [(sh, 17, 17) for sh in FUSED if sh != 'swimmer'] + \
              [('swimmer', N, rpg) for N in (1, 16, 17, 33) for rpg in (0, 5, 17) if (N, rpg) != (33, 5)] + [('swimmer', STRIDED_N, 1000), ('swimmer_k8', 20005, 0)]
_problems = {}


def problem(shape):
    """(dm, theta, pdims, pool) of a shape, everything rounded to fp32 (the device's storage type)."""
    if shape not in _problems:
        env, K, hidden, seed = SHAPES[shape]
        dm, theta, pdims, pool = Hh.problem_data(env, K, hidden, POL_HIDDEN.get(shape, (32, 32)), seed=seed, n_pool=64)
        _problems[shape] = (dm.astype(F).astype(np.float64), theta.astype(F).astype(np.float64), pdims, pool.astype(F).astype(np.float64))
    return _problems[shape]


def inputs(shape, N, seed=0):
    """fp32 pool rows and 1.5 * randn actions (so that some clip)."""
    dm, _, _, pool = problem(shape)
    rng = np.random.RandomState(1000 * (N % 1000) + seed + 7)
    obs = pool[rng.randint(len(pool), size=N)].astype(F)
    actions = (1.5 * rng.randn(N, dm.na)).astype(F)
    assert actions.size < 32 or ((actions > 1).any() and (actions < -1).any())
    return obs, actions


def offset_problem():
    """swimmer, N = 33: states with a common offset of O(1e3) on the dropped position feature 0, heads that are head 0 with weights perturbed by 1e-3 of
    themselves: |s'| >> spread.  -> (dm, obs, actions)"""
    dm, _, _, pool = problem('swimmer')
    rng = np.random.RandomState(99)
    Ws = [np.repeat(W[:1], dm.K, axis=0) * (1.0 + 1e-3 * rng.randn(*W.shape)) for W in dm.Ws]
    bs = [np.repeat(b[:1], dm.K, axis=0) * (1.0 + 1e-3 * rng.randn(*b.shape)) for b in dm.bs]
    dmo = O.DynamicsEnsemble(Ws, bs, dm.acts, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std, dm.n_drop, dm.ns, dm.na).astype(F).astype(np.float64)
    obs, actions = inputs('swimmer', 33, seed=5)
    obs = obs.copy()
    obs[:, 0] += F(1000.0) + (100.0 * rng.rand(33)).astype(F)
    return dmo, obs.astype(F), actions


_refs = {}


def reference(shape, N, rows_per_group=0):
    key = (shape, N, rows_per_group)
    if key not in _refs:
        dm = problem(shape)[0]
        obs, actions = inputs(shape, N)
        _refs[key] = disagreement(dm, SHAPES[shape][0], obs, actions, rows_per_group=rows_per_group)
    return _refs[key]
