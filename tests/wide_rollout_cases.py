"""Case table and float64 side of tests/test_gpu_wide_rollout_edges.py: the rollout kernels of the wide nets (rollout_gemm.hip, rollout_resident.hip, mlp_streamk.h,
mlp_persist.h, big_prepost.h) in every sub-form the dispatch chooses between, at the edges of THEIR tilings: the pre-step's 64 envs per workgroup, k_big_post's
8 / 4 envs, the 64-row GEMM tile, the 128-row x 256-column stream-K / persistent tile, the resident kernel's 16-env tile with B <= 128.
CPU only; never imports the library.  tests/test_wide_rollout_cases.py holds the table to its own promises (coverage, K per family, Ant margins, Philox radii,
and that the check fails a wrong kernel).  Problem, the Ant handling, f32 and seed_of are tests/rollout_cases.py's; the comparison is rollout_check._check.

FORMS: one (env, K, dynamics hidden, policy hidden, options, rollout variant) entry per sub-form, at the smallest net that selects it (stream-K needs the last
hidden width divisible by 256: 2 x 256).  expect() restates the dispatch rules of rollout_gemm_chunk / launch_rollout_gemm / launch_rollout_resident for one
launch -> the launch report (Engine.last_rollout_launch) it must produce, per CASE and per chunk, not per form: T = 1 cannot be persistent, only Philox calls
run rounds side by side, the resident kernel takes three sampling modes and B <= 128.  Rules that depend on the CU count take the nominal 256 of an MI355X (as
tests/update_cases.py does) on the CPU; the GPU test hands expect() the census of its process (Engine.schedulable_cus()), which sizes the resident grid -- slice
width, post waves, rounds per launch group, rotating deal -- and the closing workgroups of a persistent launch.

Cases of a form (cases()), draws supplied unless Philox, one sampling mode per shape rotating with the form's index:
  all-modes       B = 129 (two full 64-row tiles + one row; one 128-row block + one row), T = 6, H = 4; B = 33 for the 1024-wide forms; ends mid-path
  edges           B in 1, 15, 16, 17, 63, 64, 65, 127, 128 (1024-wide: 1, 15, 16, 17, 33); resident forms rotate over the resident kernel's three modes
  horizon         (17, 3, 1), (16, 1, 5), (17, 4, 9)
  chunked (4, 2)  on the all-modes shape: every form's chunks take the family and sub-form of the one call (expect() says so, the CPU test asserts it), so the
                  result must be field for field bitwise the one call's
  determ, philox  (17, 6, 4)
  philox-rounds   (17, 8, 4), non-Ant step-wise and stream-K forms: two rounds as ONE merged batch; with NO_MERGED_ROUNDS on parallel streams
  rotating        1024-wide resident forms: B = 65, five tiles that do not divide by the three columns the chip has room for: the rotating-deal instantiation
  resident-modes  512-wide resident forms: B = 113 (seven tiles + one lane) in the resident kernel's three modes (the all-modes shape has B > 128: non-resident)
Philox seeds are chosen so that no restated radius lies below rollout_check.SMALL_R: nothing is excluded from the normals check.

Bounds: the rows of tests/tolerances.py, no new numbers.  Next state, last_obs and reward: WIDE, STEP for the widths 72 / 96 (the stricter reading of the two the
issue allows); policy mean: wide_or_step(policy hidden); action: ACTION behind a policy <= 64 wide, else WIDE; pool rows, done, tpath, last_ts, last_model exact.

reference() restates the wide forward itself (not through oracle.dynamics_forward_all, which the check uses) and takes rollout_cases.MUTATIONS plus WIDE_MUTATIONS.

Deliberately out: the bf16 family (its own reference and test: tests/test_gpu_dyn_bf16.py); fused output tile 2 (>= 2048 tile blocks: no small shape); the
in-launch stop rule; the migrating and large-batch schedules."""
import collections
import numpy as np
from oracle import metrpo_oracle as O
import tolerances as TOL
import rollout_draws_ref as R
import rollout_cases as RC
from rollout_check import _check, ALL_DRAWS, SMALL_R

MODES = RC.MODES
RESIDENT_MODES = ('step_rand', 'eps_rand', 'one_model')
N_CU = 256                                           # MI355X; the dispatch rules restated in expect() read the device's count
MAX_PAR_ROUNDS = 8
H32, H3 = (32, 32), (100, 50, 25)

Form = collections.namedtuple('Form', 'name env K hidden pol opts variant group')
Case = collections.namedtuple('Case', RC.Case._fields + ('opts',))


def _forms():
    out = []
    add = lambda name, env, K, hidden, pol=H32, opts=(), variant=0, group='gemm': out.append(Form(name, env, K, tuple(hidden), tuple(pol), dict(opts), variant, group))
    # ---- tile GEMMs (gemm-stepwise) and the pre-steps in front of them; merged pre-step by default, STEP_MERGE=0 keeps k_big_post's own launch
    tile = dict(swimmer=(1, (96, 96)), hopper=(2, (256, 256)), snake=(3, (128, 128, 128)), half_cheetah=(5, (72, 72)), ant=(2, (128, 128)))
    for env, (K, hid) in tile.items():
        add('tile-%s' % 'x'.join(map(str, hid)), env, K, hid)
        add('tile-unmerged-%s' % env, env, K, hid, opts=dict(STEP_MERGE='0'))
    add('tile-256x256-split-out', 'hopper', 2, (256, 256), opts=dict(NO_FUSED_OUT='1'))
    add('pre-mfma3-split', 'humanoid', 2, (128, 128), H3)
    add('pre-mfma3', 'humanoid', 2, (128, 128), H3, opts=dict(NO_PRE_SPLIT='1'))
    add('pre-mfma3-merged', 'humanoid', 2, (128, 128), H3, opts=dict(STEP_MERGE='1'))
    add('pre-valu', 'humanoid', 3, (128, 128), H32)
    add('pre-gemm-chain', 'humanoid', 3, (128, 128), H32, opts=dict(PRE_GEMM='1'))
    # ---- stream-K per step
    sk = dict(STREAMK='1', NO_PERSIST='1')
    k256 = dict(swimmer=1, hopper=2, snake=3, half_cheetah=5, ant=2)
    for env, K in k256.items():
        add('streamk-1-%s' % env, env, K, (256, 256), opts=sk, variant=1, group='streamk')
    add('streamk-2', 'swimmer', 2, (256, 256, 256), opts=sk, variant=1, group='streamk')
    add('streamk-3-rows', 'humanoid', 3, (256, 256), H3, opts=sk, variant=1, group='streamk')
    add('streamk-3-gemm', 'humanoid', 3, (256, 256), H3, opts=dict(sk, NO_L0_ROWS='1'), variant=1, group='streamk')
    for ot, env, pol in ((1, 'swimmer', H32), (2, 'half_cheetah', H32), (4, 'humanoid', H3)):
        add('streamk-late-ot%d' % ot, env, 5, (1024, 1024), pol, opts=sk, variant=1, group='streamk')
        add('streamk-whole-ot%d' % ot, env, 5, (1024, 1024), pol, opts=dict(sk, STREAMK_LATE='0'), variant=1, group='streamk')
    add('streamk-place-flat', 'hopper', 2, (256, 256), opts=dict(sk, STREAMK_PLACE='flat'), variant=1, group='streamk')
    add('streamk-place-xcd', 'hopper', 2, (256, 256), opts=dict(sk, STREAMK_PLACE='xcd'), variant=1, group='streamk')
    # ---- persistent: one block per tile at 2 x 256, two at 2 x 512 (an even number of column blocks)
    for env, K in k256.items():
        add('persist-%s' % env, env, K, (256, 256), opts=dict(STREAMK='1', PERSIST_WIDE='0'), variant=1, group='persist')
    for env, K in k256.items():
        add('persist-wide-%s' % env, env, K, (512, 512), opts=dict(STREAMK='1', PERSIST_WIDE='1'), variant=1, group='persist')
    # ---- resident: the ten entries of resident_table()
    add('resident-512-swimmer-ws16', 'swimmer', 1, (512, 512), opts=dict(RESIDENT_WS='16'), group='resident')
    add('resident-512-swimmer-ws32', 'swimmer', 1, (512, 512), opts=dict(RESIDENT_WS='32'), group='resident')
    for env in ('hopper', 'snake', 'half_cheetah'):
        add('resident-512-%s' % env, env, k256[env], (512, 512), group='resident')
    for env in ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant'):     # K = 5: 80 compute workgroups per column, so that five tiles are dealt to three columns (below)
        add('resident-1024-%s' % env, env, 5, (1024, 1024), group='resident')
    assert len({f.name for f in out}) == len(out)
    return out


FORMS = _forms()
FORM = {f.name: f for f in FORMS}
FAMILY_OF_GROUP = dict(gemm='gemm-stepwise', streamk='gemm-streamk', persist='streamk-persistent', resident='resident')


def problem_key(f):
    return (f.env, f.K, f.hidden, f.pol)


def is_1024(f):
    return max(f.hidden) >= 1024


def full_shape(f):
    return (33 if is_1024(f) else 129, 6, 4)


def edge_batches(f):
    return (1, 15, 16, 17, 33) if is_1024(f) else (1, 15, 16, 17, 63, 64, 65, 127, 128)


HORIZON = RC.HORIZON
RESIDENT_FULL = (113, 6, 4)
ROTATING = (65, 6, 4)                                 # 1024-wide resident forms: five 16-env tiles on three workgroup columns -> the rotating deal (k_rollout_resident_wide<.., true>)


def cases(f):
    base = FORMS.index(f)
    pool = RESIDENT_MODES if f.group == 'resident' else MODES
    rot = lambda j: pool[(base + j) % len(pool)]
    B, T, H = full_shape(f)
    mk = lambda name, B, T, H, mode, determ=False, chunks=None, philox=False, resets=False, opts=(): Case(name, B, T, H, mode, determ, chunks, philox, True, resets, dict(opts))
    out = [mk('all-modes', B, T, H, m, resets=True) for m in MODES]
    out += [mk('edges', b, 6, 4, rot(j)) for j, b in enumerate(edge_batches(f))]
    out += [mk('horizon', b, t, h, rot(9 + j)) for j, (b, t, h) in enumerate(HORIZON)]
    out.append(mk('chunked', B, T, H, rot(12), chunks=(4, 2), resets=True))
    out.append(mk('determ', 17, 6, 4, rot(13), determ=True))
    out.append(mk('philox', 17, 6, 4, rot(14), philox=True))
    if f.env != 'ant' and f.group in ('gemm', 'streamk'):
        out.append(mk('philox-rounds', 17, 8, 4, rot(15), philox=True))
        out.append(mk('philox-rounds', 17, 8, 4, rot(15), philox=True, opts=dict(NO_MERGED_ROUNDS='1')))
    if f.group == 'resident' and not is_1024(f):
        out += [mk('resident-modes', RESIDENT_FULL[0], RESIDENT_FULL[1], RESIDENT_FULL[2], m, resets=True) for m in RESIDENT_MODES]
    if f.group == 'resident' and is_1024(f):
        out.append(mk('rotating', ROTATING[0], ROTATING[1], ROTATING[2], rot(16), resets=True))
    return out


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------------------------
RESIDENT_TABLE = {('swimmer', 512): (16, 32), ('hopper', 512): (32,), ('snake', 512): (32,), ('half_cheetah', 512): (32,),
                  ('hopper', 1024): (64,), ('snake', 1024): (64,), ('half_cheetah', 1024): (64,), ('swimmer', 1024): (64,), ('ant', 1024): (64,)}
MFMA_ENVS = ('swimmer', 'half_cheetah', 'ant', 'hopper', 'snake')
L0_ROWS_S0 = (3, 4, 5, 6, 10, 20)
FUSED_S0_OT = {(3, 1), (4, 1), (5, 1), (6, 2), (9, 2)}


def _fused_out_tile(M, N, heads, no):
    blocks = lambda tm, tn: -(-M // (64 * tm)) * -(-N // (64 * tn)) * heads
    if no > 64:
        return 0
    if M > 64 and N > 64 and N % 128 == 0 and blocks(2, 2) >= 2048:
        return 2
    if N % 64 == 0 and blocks(2, 1) < 2048 and blocks(1, 2) < 2048:
        return 1
    return 0


def _skinny_out_splits(M, N, Kd, heads):
    if Kd < 256:
        return 0
    blocks = -(-M // 64) * -(-N // 64) * heads
    if blocks >= 512:
        return 0
    S = max(min(min(8, max(1, 1024 // max(blocks, 1))), Kd // 128), 1)
    if S <= 1:
        return 0
    kchunk = (-(-Kd // S) + 15) & ~15
    return -(-Kd // kchunk)


def _sk_select(f, o, B):
    """SkPath of rollout_gemm.hip's sk_select -> (mode, late of the launch that carries the output layer, OT)."""
    ns, na, nd = O.ENV_SPECS[f.env]
    nin, K, L = ns + na - nd, f.K, len(f.hidden) + 1
    force = o.get('STREAMK', '')[:1] == '1'
    if 'NO_STREAMK' in o or L < 3 or L > 4 or ns > 64:
        return 0, 0, 0
    K1, N = (nin if L == 2 else f.hidden[-2]), f.hidden[-1]
    if K1 % 32 or N % 256:
        return 0, 0, 0
    OT = 1 if ns <= 16 else 2 if ns <= 32 else 4
    late_ok = o.get('STREAMK_LATE', '1')[:1] == '1'

    def late_for(K1_, N_, eu):
        tiles = K * -(-B // 128) * (N_ // 256)
        return int(late_ok and tiles < N_CU and (tiles * (K1_ // 32 + eu)) // N_CU >= (2 if force else 5))
    eu = 2 if OT == 4 else 1
    if not force and K * -(-B // 128) * (N // 256) < N_CU and not late_for(K1, N, eu):
        return 0, 0, 0
    if L == 3:
        S0 = (nin + 1 + 3) // 4
        if (S0, OT) in FUSED_S0_OT:
            return 1, late_for(K1, N, eu), OT
        return 3, late_for(K1, N, eu), OT
    K0, N0 = f.hidden[0], f.hidden[1]
    if K0 % 32 or N0 % 256 or N0 != K1:
        return 0, 0, 0
    return 2, late_for(K1, N, eu), OT


def expect(f, B, T, H, mode, philox=False, opts=(), t0=0, n_cu=N_CU):
    """The launch report of ONE metrpo_rollout call (a chunk of a case: t0 > 0 continues) of form `f` -> dict with every field of Engine.last_rollout_launch.  n_cu: the CUs that schedule the process's waves (Engine.schedulable_cus(): the resident grid and the persistent
    launch's closing workgroups are sized by it); the device's own count, which the stream-K rules read, is N_CU."""
    o = dict(f.opts, **dict(opts))
    ns, na, nd = O.ENV_SPECS[f.env]
    nin, K = ns + na - nd, f.K
    zero = dict(pre=None, post_width=0, sk_mode=0, late=0, l0='producer', fuse_tile=0, out_splits=0, persist_wide=0, nclose=0, rounds='single', res_ws=0, res_threads=0,
                res_pw=0, res_rg=0, res_rot=0)
    # ---- resident (launch_rollout_resident)
    widths = RESIDENT_TABLE.get((f.env, f.hidden[0]), ()) if len(f.hidden) == 2 and f.hidden[0] == f.hidden[1] else ()
    if 'RESIDENT_WS' in o:
        widths = tuple(w for w in widths if w == int(o['RESIDENT_WS']))
    if f.variant != 1 and 'NO_RESIDENT' not in o and f.pol == H32 and widths and mode in RESIDENT_MODES and B <= 128:
        Rr = T // H if (T % H == 0 and T // H >= 2 and f.env != 'ant' and t0 == 0 and 'SEQ_ROUNDS' not in o) else 1
        NT, DH = -(-B // 16), f.hidden[0]

        def fits(ws, rg):                                              # -> post waves per workgroup, None: the grid does not fit the chip
            if ws == 64:                                               # 4-wave form: the tiles of the rg rounds are dealt to as many workgroup columns as fit
                return 4 if K * (DH // ws) + (rg * NT + 3) // 4 <= n_cu else None
            return next((pw for pw in (1, 2, 4, 8) if rg * K * (DH // ws) + -(-rg * NT // pw) <= n_cu), None)
        # narrowest slice whose grid fits with all rounds side by side, else as many rounds at a time as fit on the widest
        pick = next(((w, Rr, fits(w, Rr)) for w in widths if fits(w, Rr)), None) or next(((widths[-1], rg, fits(widths[-1], rg)) for rg in range(Rr - 1, 0, -1) if fits(widths[-1], rg)), None)
        if pick is not None:
            ws, Rg, PW = pick
            rot = 0
            if ws == 64:                                               # the rotating deal of the LAST launch group: few tiles that do not divide by the columns
                G = (Rr - (Rr - 1) // Rg * Rg) * NT
                ncol = max(1, min(G, (n_cu - -(-G // PW)) // (K * (DH // ws))))
                NTC = -(-G // ncol)
                cols = -(-G // NTC)
                rot = int(cols > 1 and NTC <= 4 and G % cols != 0 and G >= cols)
            return dict(zero, family='resident', res_ws=ws, res_threads=256 if ws == 64 else 512, res_pw=PW, res_rg=Rg, res_rot=rot, rounds='parallel' if Rr > 1 else 'single')
    # ---- step-wise (launch_rollout_gemm, rollout_gemm_chunk)
    Rg = T // H if T % H == 0 else 1
    par = philox and 2 <= Rg <= MAX_PAR_ROUNDS and f.env != 'ant' and K * B <= 8192 and t0 == 0 and 'SEQ_ROUNDS' not in o
    merged = par and Rg * B <= 1024 and 'NO_MERGED_ROUNDS' not in o
    Bc, Tc = (Rg * B, H) if merged else (B, H if par else T)
    sk_mode, late, OT = _sk_select(f, o, Bc)
    S0all = (nin + 1 + 3) // 4
    l0r = sk_mode >= 2 and not late and S0all in L0_ROWS_S0 and f.hidden[0] % 256 == 0 and 'NO_L0_ROWS' not in o
    mfma3 = f.env == 'humanoid' and f.pol == H3
    mfma = f.env in MFMA_ENVS and f.pol == H32
    sm = o.get('STEP_MERGE')
    sm_forced, sm_off = sm is not None and sm[:1] != '0', sm is not None and sm[:1] == '0'
    split_small = ns > 32 and Bc <= 16 * N_CU and 'NO_PRE_SPLIT' not in o and not sm_forced
    merge_ok = not sm_off and not split_small and (ns <= 32 or sk_mode != 0 or sm_forced)
    grid = min(n_cu, N_CU) // 8 * 8                                    # the persistent launch's workgroups
    persist = (sk_mode == 1 and not merged and Tc >= 2 and 'NO_PERSIST' not in o and mfma and grid >= 16 and
               (o.get('STREAMK', '')[:1] == '1' or K * -(-Bc // 128) * (f.hidden[-1] // 256) >= grid + grid // 16))
    nclose = 0
    if persist:                                                        # closing workgroups: ~17 us per (row block, step), under ~60 % busy at this launch's step time
        RBp, CBp = -(-Bc // 128), f.hidden[-1] // 256
        step_us = float(K) * CBp * RBp * (f.hidden[-2] // 32 + 1) * 4.6 / max(1, grid - 8)
        nclose = max(2, min(8, int(np.ceil(RBp * 17.0 / (0.6 * step_us)))))
        if 'PERSIST_NCLOSE' in o:
            nclose = max(1, min(8, int(o['PERSIST_NCLOSE'])))
    pre_merged = (mfma or mfma3) and merge_ok and Tc >= 2 and not persist
    if mfma3:
        pre = 'mfma3-merged' if pre_merged else 'mfma3-split' if (Bc <= 16 * N_CU and 'NO_PRE_SPLIT' not in o) else 'mfma3'
    elif mfma:
        pre = 'mfma-merged' if pre_merged else 'mfma'
    else:
        n_params = sum(a * b + b for a, b in zip((ns,) + f.pol, f.pol + (na,))) + na
        pg = o.get('PRE_GEMM')
        pre = 'gemm-chain' if (pg is not None and pg[:1] == '1') or (not (pg is not None and pg[:1] == '0') and (Bc >= 1024 or n_params >= 4096)) else 'valu'
    fuse = 0 if (sk_mode or 'NO_FUSED_OUT' in o) else _fused_out_tile(Bc, f.hidden[-1], K, ns)
    if sk_mode:
        splits = f.hidden[-1] // 256
    elif fuse:
        splits = f.hidden[-1] // (64 * fuse)
    else:
        splits = _skinny_out_splits(Bc, ns, f.hidden[-1], K)
    CB = f.hidden[-1] // 256
    pw = o.get('PERSIST_WIDE')
    wide = persist and CB % 2 == 0 and not (pw and pw[:1] == '0') and ((pw and pw[:1] == '1') or 10 * K * (CB // 2) * -(-Bc // 128) >= 12 * (N_CU - 8))
    return dict(zero, family='streamk-persistent' if persist else 'gemm-streamk' if sk_mode else 'gemm-stepwise', pre=pre,
                post_width=0 if persist else (32 if ns <= 32 else 64), sk_mode=sk_mode, late=late, l0='producer' if sk_mode == 1 else 'rows' if l0r else 'gemm',
                fuse_tile=fuse, out_splits=splits, persist_wide=int(bool(wide)), nclose=nclose, rounds='merged' if merged else 'parallel' if par else 'single')


def expect_chunks(f, c, n_cu=N_CU):
    """One expectation per launch of a case."""
    t0, out = 0, []
    for Tc in (c.chunks or (c.T,)):
        out.append(expect(f, c.B, Tc, c.H, c.mode, c.philox, c.opts, t0, n_cu))
        t0 += Tc
    return out


# ---- the problem -----------------------------------------------------------------------------------------------------------------------------------
def state_tol(hidden):
    return TOL.STEP if max(hidden) <= 96 else TOL.WIDE


class Problem(RC.Problem):
    """rollout_cases.Problem at a wide net, with this table's bounds; Philox seeds clear of the Ant thresholds AND of radii below SMALL_R."""

    def __init__(self, env, K, hidden, pol):
        RC.Problem.__init__(self, env, K, hidden, pol, row=TOL.WIDE)
        assert self.dm.acts == ['relu'] * len(hidden)
        self.tol = state_tol(hidden)
        self.mean_tol = TOL.wide_or_step(pol)
        self.act_tol = TOL.ACTION if max(pol) <= 64 else TOL.WIDE

    def _near(self, dr, c):
        if self.env != 'ant':
            return np.zeros(c.B, bool)
        z = reference(self, dr, c.B, c.T, c.H, c.mode, c.determ)['next'][:, :, 2]
        return (np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)) < RC.ANT_MARGIN).any(axis=0)

    def _philox(self, c):
        for i in range(400):
            seed = RC.seed_of(200 + i)
            dr, rad = R.rollout_draws(seed, 0, 0, c.B, c.T, self.K, RC.N_POOL, self.dm.ns, self.dm.na)
            if min(rad['eps'].min(), rad['sel_noise'].min()) >= SMALL_R and not self._near(dr, c).any():
                return dr, rad, seed
        raise AssertionError('no seed clear of the small radii and the Ant thresholds')


# ---- float64 side ------------------------------------------------------------------------------------------------------------------------------------
WIDE_MUTATIONS = ('out_partial_dropped', 'l0_bias_missing', 'row_block_tail', 'slice_batch_tail')
MUTATIONS = RC.MUTATIONS + WIDE_MUTATIONS
VALUE_MUTATIONS = ('upper_median', 'std_ddof1', 'out_partial_dropped', 'l0_bias_missing', 'slice_batch_tail')


def mutation_applies(mut, f):
    """Forms on which a mutation must be caught: rollout_cases.mutation_applies for its nine; the four of these paths everywhere (every form has B % 64 != 0)."""
    return RC.mutation_applies(mut, f.env, f.K)


def heads_forward(p, s, ac, mut=None):
    """Every head's next state [K, B, ns]: normalise, drop the leading columns, the hidden layers with dm.acts (relu on every net of this table: Problem
    asserts it), identity output layer, de-normalise + residual."""
    dm = p.dm
    x = ((np.concatenate([s, ac], axis=1) - dm.in_mean) / dm.in_std)[:, dm.n_drop:]
    h = np.broadcast_to(x, (dm.K,) + x.shape)
    L = len(dm.Ws)
    for l in range(L - 1):
        b = np.zeros_like(dm.bs[l]) if (l == 0 and mut == 'l0_bias_missing') else dm.bs[l]
        h = O._ACTS[dm.acts[l]](np.matmul(h, dm.Ws[l]) + b[:, None, :])
    W = h.shape[2]
    if mut == 'out_partial_dropped':                                   # one partial of the output layer never added: a 256-column block, a 64-column tile where narrower
        h = h.copy(); h[:, :, W - (256 if W > 256 else 64):] = 0.0
    if mut == 'slice_batch_tail':                                      # the last of 16 slices left out of one head's sum
        h = h.copy(); h[0, :, W - max(W // 16, 1):] = 0.0
    out = np.matmul(h, dm.Ws[L - 1]) + dm.bs[L - 1][:, None, :]
    return dm.diff_mean[:dm.ns] + dm.diff_std[:dm.ns] * out + s


def reference(p, dr, B, T, H, mode, determ=False, mut=None):
    """rollout_cases.reference with the wide forward restated here -> every output tensor in the layout of rollout_check._device_run, plus 'next'."""
    env, ns, na = p.env, p.dm.ns, p.dm.na
    out = dict(obs=np.zeros((T, B, ns)), act=np.zeros((T, B, na)), mean=np.zeros((T, B, na)), rew=np.zeros((T, B)), next=np.zeros((T, B, ns)),
               done=np.zeros((T, B), bool), tpath=np.zeros((T, B), np.int64))
    s, cm, ts = p.pool32[dr['reset_idx'][0]].copy(), dr['reset_model'][0].copy(), np.zeros(B, np.int64)
    for t in range(T):
        a, info = O.policy_get_actions(p.th, p.pdims, s, dr['eps'][t])
        if determ:
            a = info['mean']
        ac = np.clip(a, -1.0, 1.0)
        idx = dr['model_idx'][t] if (mode == 'step_rand' and mut != 'step_rand_cur_model') else cm
        nxt = RC._select(heads_forward(p, s, ac, mut), mode, idx, dr['sel_noise'][t], mut)
        out['obs'][t], out['act'][t], out['mean'][t], out['next'][t] = s, a, info['mean'], nxt
        out['rew'][t] = -O.cost_np_vec(env, s, ac, nxt)
        ts = ts + 1
        dn = (ts > H) if mut == 'horizon_gt' else (ts >= H)
        if env == 'ant':
            dn = dn | ~RC.ant_not_done(nxt, mut)
        out['done'][t], out['tpath'][t] = dn, ts - (0 if mut == 'tpath_off_by_one' else 1)
        row = dr['reset_idx'][t if mut == 'reset_row_t' else t + 1]
        s = np.where(dn[:, None], p.pool32[row], nxt)
        if mut != 'eps_rand_no_switch':
            cm = np.where(dn, dr['reset_model'][t + 1], cm)
        ts = np.where(dn, 0, ts)
    out['last_obs'], out['last_ts'], out['last_model'] = s, ts, cm
    tile = 16 if mut == 'last_row_zeroed' else 64 if mut == 'row_block_tail' else 0
    if tile and B % tile:                                              # the last live row of a partial tile / 64-row block
        for k in ('obs', 'act', 'mean', 'rew'):
            out[k][:, B - 1] = 0.0
        out['last_obs'][B - 1] = 0.0
    return out


def check_case(p, c, dev, label, form=None):
    """Every output tensor of one case against the float64 oracle: rollout_check._check on this table's rows, done / tpath equal to the free-running oracle's on
    every row (Ant included: the cases are drawn clear of its thresholds)."""
    dr, rad, _ = p.draws(c)
    _check(p, dev, dr, rad, c.B, c.T, c.H, c.mode, c.determ, label, own=ALL_DRAWS if c.philox else (), expect_resets=c.expect_resets, ant_free_run=True,
           form=form, act_tol=p.act_tol, rew_tol=p.tol, mean_tol=p.mean_tol)
