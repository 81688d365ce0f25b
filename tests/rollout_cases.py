"""Case table and float64 side of tests/test_gpu_rollout_edges.py: every compiled 2 x 64 rollout instantiation at the shapes where a tile kernel goes wrong.
CPU only; never imports the library.  tests/test_rollout_cases.py holds the table to its own promises (coverage, Ant margins, and that it fails a wrong kernel).

Pairs: the 47 (env, K) entries of rollout_coop.hip / rollout_coop_k6..k10.hip (five envs, K = 1 ... 10, Ant to 8, half-cheetah to 9) and the three 2 x 64
pairs that fall off the table onto the step-wise tile GEMMs.  Forms of a pair, each named by what the library reports of its launch (forms()):
  coop-one        one workgroup per CU, as the rule launches it (8 waves where the head-split form exists: swimmer / hopper / snake at K = 2 ... 5, else 4)
  coop-one-4wave  the same with set_coop_split(False), where the rule's own launch has 8
  coop-two        two workgroups per CU (set_rollout_variant(2)), K <= 5
  head-per-wave   set_rollout_variant(1), K <= 8
  generic         metrpo_rollout_generic, at K in {1, 5, 10} and at the env's largest K
  gemm-stepwise   the off-table pairs under the default dispatch
Cases of a form (cases()): draws supplied (helpers.draws rounded to fp32) unless `philox`; at most three 16-env tiles everywhere, so no launch takes the
migrating schedule or a kernel that waits on other workgroups.  One sampling mode per (B, T, H) tuple outside `all-modes`, rotating with pair + form + case
index, so that over the table every mode meets every B and every K parity.

Ant cases are drawn clear of the done thresholds: in the float64 free run no next-state z lies within ANT_MARGIN of 0.2 or 1.0 (single envs are redrawn,
Philox cases take the next seed).  ANT_MARGIN = 1e-3 is 1000 x STEP's atol: an fp32 device cannot land on the other side within T <= 6 steps, so its
done / tpath must equal the free-running reference's on every row.

reference() restates the rollout in float64 independently of helpers.oracle_rollout (which the check itself uses) and takes one of MUTATIONS: the faults a
kernel instantiation could have that the suite did not see before this table."""
import collections
import numpy as np
from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import rollout_draws_ref as R
from rollout_check import _check, ALL_DRAWS

N_POOL = 257
MODES = tuple(O.SAM_MODES)
ENVS = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant')
K_MAX = dict(swimmer=10, half_cheetah=9, hopper=10, snake=10, ant=8)            # the cooperative kernel's table (LDS)
TABLE = [(env, K) for env in ENVS for K in range(1, K_MAX[env] + 1)]
OFF_TABLE = [('half_cheetah', 10), ('ant', 9), ('ant', 10)]
PAIRS = TABLE + OFF_TABLE
SPLIT_ENVS = ('swimmer', 'hopper', 'snake')                                     # one output col-block: head-split form at K = 2 ... 5
NARROW = [(env, K, hid) for env, K in (('swimmer', 10), ('ant', 8)) for hid in ((16, 16), (64, 17), (63, 64))]
ANT_MARGIN = 1e-3
PROBLEM_SEED, DRAW_SEED = 7, 2

Case = collections.namedtuple('Case', 'name B T H mode determ chunks philox eval_all expect_resets')


def coop_waves(env, K):
    """Waves per workgroup of the one-workgroup-per-CU launch as the rule makes it."""
    return 8 if env in SPLIT_ENVS and 2 <= K <= 5 else 4


def forms(env, K):
    if (env, K) in OFF_TABLE:
        return ['gemm-stepwise'] + (['generic'] if K in (1, 5, 10) else [])
    out = ['coop-one'] + (['coop-one-4wave'] if coop_waves(env, K) == 8 else [])
    if K <= 5:
        out.append('coop-two')
    if K <= 8:
        out.append('head-per-wave')
    if K in (1, 5, 10) or K == K_MAX[env]:
        out.append('generic')
    return out


# (form -> (set_rollout_variant, set_coop_split, force_generic, last_rollout_kernel, last_coop_waves or None))
def launch_of(env, K, form):
    return {'coop-one': (0, True, False, 'mfma-cooperative', coop_waves(env, K)), 'coop-one-4wave': (0, False, False, 'mfma-cooperative', 4),
            'coop-two': (2, True, False, 'mfma-cooperative', 4), 'head-per-wave': (1, True, False, 'mfma-head-per-wave', None),
            'generic': (0, True, True, None, None), 'gemm-stepwise': (0, True, False, 'gemm-stepwise', None)}[form]


EDGES = ((1, 6, 4), (15, 6, 4), (16, 6, 4), (17, 6, 4))
HORIZON = ((17, 3, 1), (16, 1, 5), (17, 4, 9))       # H = 1: every step resets.  T = 1.  No reset at all
FULL = (33, 6, 4)                                    # two full tiles + a one-lane tile; a reset inside; the call ends mid-path (last_ts != 0)


def cases(env, K, form):
    base = PAIRS.index((env, K)) + forms(env, K).index(form)
    rot = lambda j: MODES[(base + j) % len(MODES)]
    out = [Case('all-modes', FULL[0], FULL[1], FULL[2], m, False, None, False, True, True) for m in MODES]
    out += [Case('edges', B, T, H, rot(j), False, None, False, True, False) for j, (B, T, H) in enumerate(EDGES)]
    out += [Case('horizon', B, T, H, rot(4 + j), False, None, False, True, False) for j, (B, T, H) in enumerate(HORIZON)]
    out.append(Case('chunked', FULL[0], FULL[1], FULL[2], rot(7), False, (4, 2), False, True, True))      # the boundary sits exactly behind the horizon reset
    out.append(Case('determ', 17, 6, 4, rot(8), True, None, False, True, False))
    if form.startswith('coop'):
        out.append(Case('philox', 17, 6, 4, rot(9), False, None, True, True, False))
    if form == 'generic':
        out += [Case('selected-head-only', FULL[0], FULL[1], FULL[2], m, False, None, False, False, True) for m in ('step_rand', 'eps_rand', 'one_model')]
    return out


def seed_of(i):
    """64-bit seeds with both halves non-zero (the key's high word is seed >> 32)."""
    return ((0x9E3779B9 + 7919 * i) << 32) | (0x7F4A7C15 + 977 * i)


def f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


class Problem(object):
    """helpers.problem_data(env, K, hidden, pol) with a pool of 257 distinct rows, everything rounded to fp32 (the device's storage type)."""

    def __init__(self, env, K, hidden=(64, 64), pol=(32, 32), row=TOL.STEP, dyn_act='relu', shape=None):
        """dyn_act: one activation name or one per hidden layer; shape(dm, theta, pdims, pool): changes the float64 net in place before it is rounded
        (tests/dyn_act_cases.py scales the first layer with it).  The defaults give the table of this file."""
        self.env, self.K, self.hidden, self.pol = env, K, tuple(hidden), tuple(pol)
        dm, theta, self.pdims, pool = Hh.problem_data(env, K, hidden, pol, seed=PROBLEM_SEED, n_pool=N_POOL, dyn_act=dyn_act)
        if env == 'ant':                                           # some envs start near the lower z bound: state-dependent dones inside the call
            pool[::3, 2] = 0.21; dm.diff_mean[2] = -0.02
        if shape is not None:
            shape(dm, theta, self.pdims, pool)
        self.dm = dm.astype(np.float32).astype(np.float64)
        self.th, self.pool32 = f32(theta), f32(pool)
        assert len({r.tobytes() for r in self.pool32}) == N_POOL    # distinct rows: a pool row identifies its index
        self.tol = TOL.wide_or_step(hidden)
        assert self.tol is row, (hidden, row)                       # this table is row 1's: no wide net by accident (tests/wide_rollout_cases.py passes row 2)
        self._draws = {}

    # ---- draws of a case: (draws, radii or None, seed)
    def draws(self, c):
        key = (c.B, c.T, c.H, c.mode, c.determ, c.philox)
        if key not in self._draws:
            self._draws[key] = self._philox(c) if c.philox else self._supplied(c)
        return self._draws[key]

    def _near(self, dr, c):
        """Envs whose float64 free run comes within ANT_MARGIN of a done threshold."""
        if self.env != 'ant':
            return np.zeros(c.B, bool)
        z = reference(self, dr, c.B, c.T, c.H, c.mode, c.determ)['next'][:, :, 2]
        return (np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) < ANT_MARGIN).any(axis=0)

    def _supplied(self, c):
        ns, na = self.dm.ns, self.dm.na
        rnd = lambda d: {k: (f32(v) if v.dtype == np.float64 else v) for k, v in d.items()}
        dr = rnd(Hh.draws(np.random.RandomState(DRAW_SEED), self.K, c.B, c.T, ns, na, N_POOL))
        for attempt in range(1, 100):
            bad = self._near(dr, c)
            if not bad.any():
                return dr, None, 0
            new = rnd(Hh.draws(np.random.RandomState(DRAW_SEED + 1000 * attempt), self.K, c.B, c.T, ns, na, N_POOL))
            for k in dr:                                               # envs are independent: only the offending ones are redrawn
                dr[k][:, bad] = new[k][:, bad]
        raise AssertionError('no draw clear of the Ant thresholds')

    def _philox(self, c):
        for i in range(100):
            seed = seed_of(200 + i)
            dr, rad = R.rollout_draws(seed, 0, 0, c.B, c.T, self.K, N_POOL, self.dm.ns, self.dm.na)
            if not self._near(dr, c).any():
                return dr, rad, seed
        raise AssertionError('no seed clear of the Ant thresholds')


MUTATIONS = ('upper_median', 'std_ddof1', 'step_rand_cur_model', 'eps_rand_no_switch', 'reset_row_t', 'tpath_off_by_one', 'horizon_gt', 'ant_bound_gt',
             'last_row_zeroed')


def mutation_applies(mut, env, K):
    """Pairs on which a mutation must be caught.  std_ddof1 at K = 2 is only at the bound (factor sqrt(2) on a std of two heads ~1e-2 apart times noise):
    required from K = 3.  ant_bound_gt shows only AT a threshold, which the rollout cases are drawn clear of: the identity pass holds it (ant_done.npz)."""
    return {'upper_median': K % 2 == 0, 'std_ddof1': K >= 3, 'step_rand_cur_model': K >= 2, 'eps_rand_no_switch': K >= 2, 'ant_bound_gt': False}.get(mut, True)


def _select(heads, mode, idx, noise, mut):
    K, B = heads.shape[:2]
    if mode in ('step_rand', 'eps_rand'):
        return heads[idx, np.arange(B)]
    if mode == 'model_mean_std':
        return heads.mean(axis=0) + noise * heads.std(axis=0, ddof=1 if mut == 'std_ddof1' and K > 1 else 0)
    if mode == 'model_mean':
        return heads.mean(axis=0)
    if mode == 'model_med':
        s = np.sort(heads, axis=0)
        if K % 2:
            return s[K // 2]
        return s[K // 2] if mut == 'upper_median' else 0.5 * (s[K // 2 - 1] + s[K // 2])
    assert mode == 'one_model'
    return heads[0]


def ant_not_done(x_next, mut=None):
    z = x_next[:, 2]
    inside = ((z > 0.2) & (z < 1.0)) if mut == 'ant_bound_gt' else ((z >= 0.2) & (z <= 1.0))
    return inside & np.isfinite(x_next).all(axis=1)


def reference(p, dr, B, T, H, mode, determ=False, teacher_obs=None, mut=None):
    """The rollout in float64, free-running (or teacher-forced on `teacher_obs` [T, B, ns]) -> every output tensor of Engine.rollout, in the layout of
    rollout_check._device_run, plus 'next' (the selected next state in front of the reset).  `mut`: one of MUTATIONS."""
    dm, env, ns, na = p.dm, p.env, p.dm.ns, p.dm.na
    out = dict(obs=np.zeros((T, B, ns)), act=np.zeros((T, B, na)), mean=np.zeros((T, B, na)), rew=np.zeros((T, B)), next=np.zeros((T, B, ns)),
               done=np.zeros((T, B), bool), tpath=np.zeros((T, B), np.int64))
    s, cm, ts = p.pool32[dr['reset_idx'][0]].copy(), dr['reset_model'][0].copy(), np.zeros(B, np.int64)
    for t in range(T):
        if teacher_obs is not None:
            s = np.asarray(teacher_obs[t], np.float64)
        a, info = O.policy_get_actions(p.th, p.pdims, s, dr['eps'][t])
        if determ:
            a = info['mean']
        ac = np.clip(a, -1.0, 1.0)
        idx = dr['model_idx'][t] if (mode == 'step_rand' and mut != 'step_rand_cur_model') else cm
        nxt = _select(O.dynamics_forward_all(dm, s, ac), mode, idx, dr['sel_noise'][t], mut)
        out['obs'][t], out['act'][t], out['mean'][t], out['next'][t] = s, a, info['mean'], nxt
        out['rew'][t] = -O.cost_np_vec(env, s, ac, nxt)
        ts = ts + 1
        dn = (ts > H) if mut == 'horizon_gt' else (ts >= H)
        if env == 'ant':
            dn = dn | ~ant_not_done(nxt, mut)
        out['done'][t], out['tpath'][t] = dn, ts - (0 if mut == 'tpath_off_by_one' else 1)
        row = dr['reset_idx'][t if mut == 'reset_row_t' else t + 1]
        s = np.where(dn[:, None], p.pool32[row], nxt)
        if mut != 'eps_rand_no_switch':
            cm = np.where(dn, dr['reset_model'][t + 1], cm)
        ts = np.where(dn, 0, ts)
    out['last_obs'], out['last_ts'], out['last_model'] = s, ts, cm
    if mut == 'last_row_zeroed' and B % 16:                        # the last live row of a partial tile
        for k in ('obs', 'act', 'mean', 'rew'):
            out[k][:, B - 1] = 0.0
        out['last_obs'][B - 1] = 0.0
    return out


def check_case(p, c, dev, label, form=None):
    """Every output tensor of one case (`dev`: the layout of rollout_check._device_run) against the float64 oracle: rollout_check._check on the rows STEP /
    ACTION / REWARD, done / tpath equal to the free-running oracle's on every row (Ant included: the cases are drawn clear of its thresholds)."""
    dr, rad, _ = p.draws(c)
    _check(p, dev, dr, rad, c.B, c.T, c.H, c.mode, c.determ, label, own=ALL_DRAWS if c.philox else (), expect_resets=c.expect_resets, ant_free_run=True,
           form=form, act_tol=TOL.ACTION, rew_tol=TOL.REWARD)
