"""NumPy restatement of the bf16-operand dynamics forward of metrpo_rollout (include/metrpo.h, metrpo_set_dyn_precision; csrc/rollout_bf16.hip):

    out[b][j] = act_l( b_l[j] + sum_i bf16(in[b][i]) * bf16(W_l[i][j]) )

bf16(.) rounds an f32 to nearest, ties to even.  Products and sums are formed in float64 here; normalisation (x - mean) / std is formed in float32 as the
device forms it (both operations are correctly rounded on either side), the hidden activation is rounded to f32 first -- the device holds act(b + sum) as an
f32 -- and then to bf16, once.  Everything around the layers (residual s' = s + diff_mean + diff_std * out, training.py:257; selection over the heads,
reward, done, reset: env_helpers.py:597-635) is the float64 oracle's.

Three things live here, all CPU only:
  * bf16_round: the rounding helper (modes 'rne', 'trunc', 'half_up', 'none'), pinned against torch in tests/test_dyn_bf16_ref.py
  * rollout_ref: free-running rollout under a deterministic policy with supplied draws
  * exact_case / check_exact: nets, normalisers, pool and policy on which every product and every partial sum is exact in f32, so that ANY summation
    order gives the same bits; random_case / emu_f32_step: Xavier nets and a float32-accumulating emulation in another order, whose distance to the
    restatement sets the bound of the random-net GPU test.
"""
import numpy as np
from oracle import metrpo_oracle as O


def bf16_round(x, mode='rne'):
    """f32 array -> the f32 values of its bf16 rounding.  'rne': nearest, ties to even; 'trunc': toward zero; 'half_up': nearest, ties away from
    zero in magnitude; 'none': unchanged."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if mode == 'none':
        return x.copy()
    u = x.view(np.uint32).astype(np.uint64)
    if mode == 'rne':
        r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    elif mode == 'trunc':
        r = u >> 16
    elif mode == 'half_up':
        r = (u + 0x8000) >> 16
    else:
        raise ValueError(mode)
    nan = np.isnan(x)
    r = np.where(nan, (u >> 16) | 0x40, r)
    return (r << 16).astype(np.uint32).view(np.float32).reshape(x.shape)


_ACT = {'relu': lambda h: np.maximum(h, 0.0), 'tanh': np.tanh, 'identity': lambda h: h}


def normalise(dm, s, ac):
    """The layer-0 input rows as the device forms them: float32 (x - mean) / std, leading columns dropped."""
    xu = np.concatenate([s, ac], axis=1).astype(np.float32)
    return ((xu - dm.in_mean.astype(np.float32)) / dm.in_std.astype(np.float32))[:, dm.n_drop:]


def net_out(dm, k, x32, mode='rne', record=None):
    """Output layer of head k for the normalised f32 rows x32, float64 sums over rounded operands."""
    h = x32
    L = len(dm.Ws)
    for l in range(L):
        hr = bf16_round(h, mode).astype(np.float64)
        Wr = bf16_round(dm.Ws[l][k].astype(np.float32), mode).astype(np.float64)
        b = dm.bs[l][k].astype(np.float32).astype(np.float64)
        if record is not None:
            record.append((np.asarray(h, np.float32), dm.Ws[l][k].astype(np.float32), hr, Wr, b))
        z = b + hr @ Wr
        if l < L - 1:
            h = _ACT[dm.acts[l]](z).astype(np.float32)           # the f32 activation the device rounds
        else:
            return z


def step_all(dm, s, ac, mode='rne', record=None):
    """Next state of every head, [K, B, ns] float64, from f32-representable states s and clipped actions ac."""
    x32 = normalise(dm, s, ac)
    s64 = s.astype(np.float64)
    f = lambda v: v.astype(np.float32).astype(np.float64)
    return np.stack([f(dm.diff_mean) + f(dm.diff_std) * net_out(dm, k, x32, mode, record) + s64 for k in range(dm.K)], axis=0)


def rollout_ref(dm, theta, pdims, env, pool, B, T, H, sam_mode, model_idx, reset_idx, reset_model, mode='rne', record=None):
    """Free-running rollout under the deterministic policy (actions = mean), supplied draws; states are stored as f32 at every step, as the device
    stores them.  -> dict(obs [T,B,ns] f32, act [T,B,na], rew [T,B] float64, done, tpath, last_obs f32)."""
    ns, na = dm.ns, dm.na
    pool32 = pool.astype(np.float32)
    th = theta.astype(np.float32).astype(np.float64)
    out = dict(obs=np.zeros((T, B, ns), np.float32), act=np.zeros((T, B, na), np.float32), rew=np.zeros((T, B)), done=np.zeros((T, B), bool),
               tpath=np.zeros((T, B), np.int64))
    s = pool32[reset_idx[0]].copy()
    cur = reset_model[0].copy()
    ts = np.zeros(B, np.int64)
    for t in range(T):
        a = O.policy_mean(th, pdims, s.astype(np.float64)).astype(np.float32)
        ac = np.clip(a, -1.0, 1.0)
        nall = step_all(dm, s, ac, mode, record)
        idx = model_idx[t] if sam_mode == 'step_rand' else cur
        nxt = O.select_next(nall, sam_mode, idx, None).astype(np.float32)
        out['obs'][t], out['act'][t] = s, a
        out['rew'][t] = -O.cost_np_vec(env, s.astype(np.float64), ac.astype(np.float64), nxt.astype(np.float64))
        ts += 1
        dn = O.is_done(env, nxt, nxt) | (ts >= H)
        out['done'][t], out['tpath'][t] = dn, ts - 1
        s = np.where(dn[:, None], pool32[reset_idx[t + 1]], nxt)
        cur = np.where(dn, reset_model[t + 1], cur)
        ts[dn] = 0
    out['last_obs'] = s
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _sparse_int(rng, n_in, n_out, nnz, vals):
    W = np.zeros((n_in, n_out))
    for j in range(n_out):
        rows = rng.choice(n_in, size=min(nnz, n_in), replace=False)
        W[rows, j] = rng.choice(vals, size=len(rows))
    return W


def exact_case(env, K, hidden, seed, out_scale=2):
    """Small-integer sparse nets on a half-integer state grid.  States, clipped actions and biases are multiples of 1/2; hidden weights are -1 / 0 / +1
    (two non-zeros per column in layer 0, one or two behind it); the output layer's weights are +-out_scale with integer biases times out_scale / 2 and
    diff_std = 1/2, so a step moves a state by a multiple of out_scale / 4 ... of 1/2 for out_scale = 2: the grid is kept.  out_scale = 10 makes the K = 5 mean
    (model_mean) land on the grid as well: the sum over the heads of s + delta_k is a multiple of 5/2.  in_mean = 0, in_std = 1, diff_mean = 0.
    The policy has zero weights and dyadic output biases beyond +-1 in places (the clip is exercised): actions are exact constants.
    -> (dm, theta, pdims, pool); check_exact says whether a rollout on it stays exact."""
    ns, na, n_drop = O.ENV_SPECS[env]
    rng = np.random.RandomState(seed)
    dims = [ns + na - n_drop] + list(hidden) + [ns]
    Ws, bs = [], []
    for l in range(len(dims) - 1):
        last = l == len(dims) - 2
        Wk, bk = [], []
        for k in range(K):
            if last:
                Wk.append(_sparse_int(rng, dims[l], dims[l + 1], 2, [-out_scale, out_scale]))
                bk.append(rng.randint(-1, 2, size=dims[l + 1]) * (out_scale / 2.0))
            else:
                Wk.append(_sparse_int(rng, dims[l], dims[l + 1], 2 if l == 0 else 1 + (k + l) % 2, [-1.0, 1.0]))
                bk.append(rng.randint(-3, 2, size=dims[l + 1]) * 0.5)
        Ws.append(np.stack(Wk)); bs.append(np.stack(bk))
    dm = O.DynamicsEnsemble(Ws, bs, ['relu'] * len(hidden), np.zeros(ns + na), np.ones(ns + na), np.zeros(ns), np.full(ns, 0.5), n_drop, ns, na)
    pol_hidden = (100, 50, 25) if env == 'humanoid' else (32, 32)
    pdims = O.policy_dims(ns, pol_hidden, na)
    pW = [np.zeros((pdims[i], pdims[i + 1])) for i in range(len(pdims) - 1)]
    pb = [np.zeros(pdims[i + 1]) for i in range(len(pdims) - 1)]
    pb[-1] = rng.choice([-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5], size=na)
    theta = O.policy_flatten(pW, pb, np.zeros(na))
    pool = rng.randint(-2, 3, size=(64, ns)) * 0.5
    if env == 'ant':
        pool[:, 2] = rng.choice([0.5, 1.0], size=64)             # alive at the reset: 0.2 <= z <= 1
    return dm, theta, pdims, pool


def pow2_grid(*arrays):
    """Largest power of two that divides every entry of the arrays (1.0 for all-zero input)."""
    v = np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays])
    v = v[v != 0]
    for e in range(-8, 64):
        if np.all(v * 2.0 ** e == np.round(v * 2.0 ** e)):
            return 2.0 ** -e
    raise AssertionError('no dyadic grid')


def check_exact(record):
    """The two properties that make a recorded rollout order-independent in f32: (1) nothing the restatement rounds is changed by the rounding;
    (2) in every layer application the products and the bias are integer multiples of one grid g, and sum_i |x_i W_ij| + |b_j| < 2^24 g for every
    output -- so every partial sum, in any order, is an integer multiple of g below 2^24 g: exactly representable, no rounding anywhere."""
    assert record
    for h, W, hr, Wr, b in record:
        assert np.array_equal(h.astype(np.float64), hr) and np.array_equal(W.astype(np.float64), Wr)
        g = min(pow2_grid(hr) * pow2_grid(Wr), pow2_grid(b))
        worst = np.max(np.abs(hr) @ np.abs(Wr) + np.abs(b))
        assert worst < 2.0 ** 24 * g, (worst, g)


def exact_rollout(env, K, hidden, B, T, H, sam_mode, seed):
    """A case and its restated rollout that passes check_exact: seeds seed, seed + 1000, ... are tried in turn (an activation that outgrows bf16's eight
    significand bits fails check_exact; the next seed is taken).  -> (dm, theta, pdims, pool, draws, ref)"""
    out_scale = 10 if (sam_mode == 'model_mean' and K > 1) else 2
    for attempt in range(50):
        sd = seed + 1000 * attempt
        dm, theta, pdims, pool = exact_case(env, K, hidden, sd, out_scale)
        rng = np.random.RandomState(sd + 7)
        dr = dict(model_idx=rng.randint(K, size=(T, B)), reset_idx=rng.randint(len(pool), size=(T + 1, B)), reset_model=rng.randint(K, size=(T + 1, B)))
        rec = []
        ref = rollout_ref(dm, theta, pdims, env, pool, B, T, H, sam_mode, dr['model_idx'], dr['reset_idx'], dr['reset_model'], record=rec)
        try:
            check_exact(rec)
        except AssertionError:
            continue
        return dm, theta, pdims, pool, dr, ref
    raise AssertionError('no exact case found for %s' % ((env, K, hidden, B, sam_mode, seed),))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# random real-valued nets
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def random_case(hidden, env='half_cheetah', K=3, B=4097, seed=5, acts='relu'):
    """Xavier nets as synthetic makes them (oracle make_problem), states from the pool, actions in [-1, 1]; everything f32-representable.
    B = 4097 rows (not a multiple of any tile; 33 row tiles), not 129: a hidden activation within f32 error of a bf16 tie rounds the other way under another
    summation order, about two in a million do, and ONE such flip moves a head's rel-L2 over 129 rows by 3e-5 at hidden (128, 128) -- 600 x the
    flip-free figure (5e-8) and 1/60 of the distance to the unrounded model (1.8e-3).  At 129 rows the measured figure is therefore 5e-8 or 3e-5 by the luck
    of the order, and 8 x 10 x 3e-5 exceeds 1.8e-3: margin and discrimination cannot both hold.  Over 4097 rows every head sees a few flips, the figure
    is stable (1.8e-5 / 8.3e-6) and both hold (the unrounded model is 102 / 112 figures away).  The case was enlarged, not the bound.
    acts: one activation name, or one per hidden layer (the weights do not depend on it)."""
    dm, theta, pdims, pool = O.make_problem(env, K=K, dyn_hidden=hidden, pol_hidden=(32, 32), seed=seed, n_pool=B, dyn_act=acts)
    dm = dm.astype(np.float32).astype(np.float64)
    rng = np.random.RandomState(seed + 1)
    s = pool.astype(np.float32)
    ac = rng.uniform(-1, 1, size=(B, dm.na)).astype(np.float32)
    return dm, s, ac


def emu_f32_step(dm, s, ac):
    """The same step with every sum accumulated in FLOAT32, in another order than any matrix instruction's: k in chunks of 4 (a float32 matmul each), the
    chunks added one after the other; hidden activations act(b + sum) in f32, then rounded to bf16.  -> delta [K, B, ns] (s' - s) float64."""
    x32 = normalise(dm, s, ac)
    out = []
    for k in range(dm.K):
        h = x32
        L = len(dm.Ws)
        for l in range(L):
            hr, Wr = bf16_round(h), bf16_round(dm.Ws[l][k].astype(np.float32))
            acc = np.zeros((hr.shape[0], Wr.shape[1]), np.float32)
            for k0 in range(0, hr.shape[1], 4):
                acc = acc + hr[:, k0:k0 + 4] @ Wr[k0:k0 + 4]
            z = dm.bs[l][k].astype(np.float32) + acc
            h = _ACT[dm.acts[l]](z).astype(np.float32) if l < L - 1 else z
        out.append(dm.diff_mean.astype(np.float32) + dm.diff_std.astype(np.float32) * h)
    return np.stack(out).astype(np.float64)


def ref_delta(dm, s, ac, mode='rne'):
    return step_all(dm, s, ac, mode) - s.astype(np.float64)


def rel_l2_per_head(got, ref):
    return np.array([np.linalg.norm(got[k] - ref[k]) / np.linalg.norm(ref[k]) for k in range(len(ref))])


RANDOM_HIDDEN = [(128, 128), (512, 512)]
BOUND_FACTOR = 8.0          # margin for a third summation order (the matrix instruction's)


def random_bound(hidden, acts='relu'):
    """rel-L2 bound of the random-net GPU test at this width: 8 x the distance between the float32-accumulating emulation and the restatement
    (worst head).  -> (bound, emulation figure, case, restated delta)"""
    dm, s, ac = random_case(hidden, acts=acts)
    ref = ref_delta(dm, s, ac)
    fig = float(np.max(rel_l2_per_head(emu_f32_step(dm, s, ac), ref)))
    return BOUND_FACTOR * fig, fig, (dm, s, ac), ref
