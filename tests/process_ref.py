"""process_samples (samplers/base.py:48-104,163-167) restated in float64 on TIME-MAJOR arrays, vectorised over the env columns.

The oracle's O.process_samples walks a list of path dicts (helpers.paths_from_timemajor), one Python step per element: fine for the
T <= 30 fixtures, minutes at T * B in the millions.  This module computes the same quantities with one reverse scan over t whose
every step is a NumPy operation on the B env columns, with the arithmetic of the oracle in the same order (so the two agree to
float64 rounding, tests/test_process_ref.py):

    delta_t = (r_t + g * V_{t+1}) - V_t,   adv_t = delta_t + (g * lam) * adv_{t+1},   ret_t = r_t + g * ret_{t+1}

restarting (V_{t+1} = adv_{t+1} = ret_{t+1} = 0) at every done step; samples behind the last done of a column belong to a path
that never finished and get valid = 0 (the reference drops such paths, vectorized_sampler.py:60,104).

Features are rllab's LinearFeatureBaseline._features in float64: [o, o^2, al, al^2, al^3, 1], o = clip(obs, -10, 10),
al = tpath / 100 with tpath the 0-based step index inside the path.  Inputs are taken as given (the device's fp32 values
widened to float64); nothing here rounds to fp32.
"""
import numpy as np


def features(obs, tpath):
    """obs [..., ns], tpath [...] -> [..., 2 ns + 4] float64."""
    o = np.clip(np.asarray(obs, dtype=np.float64), -10.0, 10.0)
    al = np.asarray(tpath, dtype=np.float64)[..., None] / 100.0
    return np.concatenate([o, o * o, al, al * al, al * al * al, np.ones_like(al)], axis=-1)


def baseline_values(obs, tpath, coeffs):
    """LinearFeatureBaseline.predict of every sample: features . coeffs, [T, B] float64."""
    return features(obs, tpath) @ np.asarray(coeffs, dtype=np.float64)


def gae(rew, done, gamma, lam, V=None):
    """rew, done [T, B]; V [T, B] float64 baseline values or None (zeros) -> adv, ret [T, B] float64, valid [T, B] bool."""
    rew = np.asarray(rew, dtype=np.float64)
    done = np.asarray(done).astype(bool)
    T, B = rew.shape
    gl = gamma * lam
    adv = np.zeros((T, B)); ret = np.zeros((T, B)); valid = np.zeros((T, B), bool)
    a_n = np.zeros(B); v_n = np.zeros(B); r_n = np.zeros(B); comp = np.zeros(B, bool)
    zero = np.zeros(B)
    for t in range(T - 1, -1, -1):
        d = done[t]
        a_n = np.where(d, 0.0, a_n); v_n = np.where(d, 0.0, v_n); r_n = np.where(d, 0.0, r_n)
        comp = comp | d
        v = V[t] if V is not None else zero
        delta = (rew[t] + gamma * v_n) - v
        a_n = delta + gl * a_n
        r_n = rew[t] + gamma * r_n
        v_n = v
        adv[t], ret[t], valid[t] = a_n, r_n, comp
    return adv, ret, valid


def stats(adv, valid):
    """(sum adv, sum adv^2, count) over the valid samples, float64."""
    a = np.asarray(adv, dtype=np.float64)[np.asarray(valid).astype(bool)]
    return np.array([a.sum(), (a * a).sum(), float(a.size)])


def center(adv, valid=None):
    """[rllab] center_advantages over the valid samples with two-pass mean / std (np.mean, np.std); invalid samples -> 0."""
    a = np.asarray(adv, dtype=np.float64)
    m = np.ones(a.shape, bool) if valid is None else np.asarray(valid).astype(bool)
    out = np.zeros(a.shape)
    if m.any():
        x = a[m]
        out[m] = (x - x.mean()) / (x.std() + 1e-8)
    return out


def normal_equations(obs, ret, tpath, valid=None, chunk=1 << 18):
    """A^T A [F, F] and A^T y [F] of LinearFeatureBaseline.fit over the valid samples (flattened), in float64, summed in chunks
    of `chunk` samples so that the feature matrix of a 2e6-sample batch is never formed whole."""
    ns = obs.shape[-1]
    obs = np.asarray(obs).reshape(-1, ns); ret = np.asarray(ret).reshape(-1); tpath = np.asarray(tpath).reshape(-1)
    m = np.ones(ret.shape, bool) if valid is None else np.asarray(valid).reshape(-1).astype(bool)
    F = 2 * ns + 4
    AtA = np.zeros((F, F)); Aty = np.zeros(F)
    for s in range(0, ret.size, chunk):
        sl = slice(s, s + chunk)
        k = m[sl]
        Fm = features(obs[sl][k], tpath[sl][k])
        AtA += Fm.T @ Fm
        Aty += Fm.T @ ret[sl][k].astype(np.float64)
    return AtA, Aty


def path_counts(done, tpath):
    """Samples of the paths completed at each step: sum_b done[t, b] * (tpath[t, b] + 1), [T] float64."""
    return (np.asarray(done).astype(bool) * (np.asarray(tpath, dtype=np.float64) + 1.0)).sum(axis=1)


def stop_step(done, tpath, t0, batch_size, cum0=0.0):
    """Loop condition of obtain_samples over a chunk that starts at global step t0 with cum0 samples already counted:
    -> (cum, stop step or None).  cum is the total at the stop step (or over the whole chunk when it is not reached)."""
    cum = float(cum0)
    for t, c in enumerate(path_counts(done, tpath)):
        cum += c
        if cum >= batch_size:
            return cum, t0 + t
    return cum, None


# ---------------------------------------------------------------------------------------------------------------------------------
# done patterns of the tests (time-major done [T, B] uint8 and the matching path-time index tpath [T, B] int32)
# ---------------------------------------------------------------------------------------------------------------------------------
DONE_PATTERNS = ('every', 'single', 'none', 'straddle', 't0', 'ant')


def make_done(pattern, T, B, rng, nw=8, t_offset=0):
    """every    every step ends a path (paths of length 1)
    single   one path of length T per env (done at t = T - 1 only)
    none     no done at all: every sample belongs to an unfinished path (count 0)
    straddle column b ends paths every L_b steps, L_b running over 1 ... 2 Tc + 3 (Tc = ceil(T / nw), the kernel's time chunk)
             with a per-column phase: paths end on, before and after every chunk boundary and span whole chunks
    t0       done at t = 0 in every column, then random ends (p = 0.1)
    ant      random early termination (p = 0.02, Ant's is_done) under a horizon of 100 steps
    t_offset > 0: the first path of each column started up to t_offset - 1 steps before t = 0 (a chunked rollout's later chunk)."""
    done = np.zeros((T, B), bool)
    if pattern == 'every':
        done[:] = True
    elif pattern == 'single':
        done[T - 1] = True
    elif pattern == 'none':
        pass
    elif pattern == 'straddle':
        Tc = -(-T // nw)
        L = 1 + np.arange(B) % (2 * Tc + 3)
        ph = rng.randint(0, 1 << 20, size=B) % L
        done = ((np.arange(T)[:, None] + ph[None, :] + 1) % L[None, :]) == 0
    elif pattern == 't0':
        done = rng.rand(T, B) < 0.1
        done[0] = True
    elif pattern == 'ant':
        done = rng.rand(T, B) < 0.02
    else:
        raise ValueError(pattern)
    tpath = np.zeros((T, B), np.int32)
    ts = rng.randint(0, t_offset, size=B).astype(np.int64) if t_offset > 0 else np.zeros(B, np.int64)
    for t in range(T):
        tpath[t] = ts
        ts += 1
        if pattern == 'ant':
            done[t] |= ts >= 100
        ts[done[t]] = 0
    return done.astype(np.uint8), tpath
