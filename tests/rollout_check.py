"""One rollout against the float64 oracle, every output tensor: shared by tests/test_gpu_rollout_draws.py (production draws of every kernel family) and
tests/test_gpu_rollout_edges.py (every 2 x 64 instantiation at the tile edges), and run without a device by tests/test_rollout_cases.py on a float64
trajectory in the device's place.  The bounds are the rows of tests/tolerances.py; the widening by the draws' own error is described in
test_gpu_rollout_draws.py and applies only to tensors the device drew itself (`own`)."""
import numpy as np
from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL

SMALL_R = 2.0 ** -6            # normals of a smaller restated radius are left out of the normals check (only)
EXCLUDE_CAP = 1e-3             # ... at most this share of a case's normals (expected 1.2e-4)
ALL_DRAWS = ('eps', 'model_idx', 'sel_noise', 'reset_idx', 'reset_model')
REPORT = {}                    # (form, tensor) -> worst share of its bound over every _check(..., form=...) of this process


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _device_run(p, B, T, H, mode, kernel, seed, stream_offset=0, determ=False, force_generic=False, supplied=None, chunks=None, eval_all_heads=True,
                launched=None):
    """One production-mode rollout (or the chunks of one: `chunks` = lengths summing to T, continued with t0 / resume / last_state) -> NumPy fields.
    `launched(eng)`: called behind every launch (further assertions on the library's launch report)."""
    import torch
    eng, dev = p.eng, p.eng.device
    lts, lmd = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    parts, resume, t0 = [], None, 0
    for Tc in (chunks or (T,)):
        kw = {k: v[t0:t0 + Tc + (1 if k.startswith('reset') else 0)] for k, v in (supplied or {}).items()}
        tr = eng.rollout(B, Tc, H, mode, p.pool_t, determ=determ, eval_all_heads=eval_all_heads, seed=seed, stream_offset=stream_offset, force_generic=force_generic,
                         t0=t0, resume=resume, last_state=(lts, lmd), **kw)
        if not force_generic:                                      # metrpo_rollout_generic IS the kernel: it goes through no dispatch and records none
            assert eng.last_rollout_kernel() == kernel, (eng.last_rollout_kernel(), eng.rollout_note())
        if launched is not None:
            launched(eng)
        parts.append({k: cpu(getattr(tr, k)) for k in ('obs', 'act', 'mean', 'rew', 'done', 'tpath', 'last_obs')})
        resume = (tr.last_obs.clone(), lts.clone(), lmd.clone())
        t0 += Tc
    assert t0 == T
    out = {k: np.concatenate([q[k] for q in parts], 0) for k in ('obs', 'act', 'mean', 'rew', 'done', 'tpath')}
    out['done'] = out['done'].astype(bool); out['tpath'] = out['tpath'].astype(np.int64)
    out['last_obs'] = parts[-1]['last_obs']
    out['last_model'], out['last_ts'] = cpu(lmd).astype(np.int64), cpu(lts).astype(np.int64)
    return out


def _close(got, ref, tol, extra, what, form=None):
    lim = tol['atol'] + extra + tol['rtol'] * np.abs(ref)
    err = np.abs(got - ref)
    used = float((err / lim).max()) if err.size else 0.0
    print('    %-8s max |err| %.3g  = %.2f of the bound' % (what, float(err.max()) if err.size else 0.0, used))
    if form is not None:
        REPORT[(form, what)] = max(REPORT.get((form, what), 0.0), used if np.isfinite(got).all() else float('inf'))
    assert np.isfinite(got).all() and used <= 1.0, (what, float(err.max()), used)


def _check(p, dev, dr, rad, B, T, H, mode, determ, label, own=ALL_DRAWS, expect_resets=True, ant_free_run=False, form=None, act_tol=None, rew_tol=None,
           mean_tol=None):
    """`dr`: the draws the device must have used; `own`: those it drew itself (the restated ones; the others were supplied).
    expect_resets=False: the case is not required to hold a reset (B = 1, T < H): that is then a property of the case table, not of the device.
    ant_free_run=True: the case was drawn clear of Ant's done thresholds, so done / tpath must equal the FREE-RUNNING oracle's on every row for Ant too.
    form: record the worst share of every bound under this name in REPORT.  act_tol / rew_tol: the row for the action / the reward where it is not the
    state's (TOL.ACTION / TOL.REWARD beside TOL.STEP); mean_tol: the row of the policy mean where the policy's width class is not the dynamics net's (a 2 x 32
    policy in front of a wide ensemble: TOL.STEP beside TOL.WIDE)."""
    env, K, ns, na, tol = p.env, p.K, p.dm.ns, p.dm.na, p.tol
    dn, tpath = dev['done'], dev['tpath']
    print('%s: B %d T %d H %d %s, %d resets' % (label, B, T, H, mode, int(dn.sum())))
    # ---- pool rows, exact
    np.testing.assert_array_equal(dev['obs'][0], p.pool32[dr['reset_idx'][0]])
    nxt_obs = np.concatenate([dev['obs'][1:], dev['last_obs'][None]], 0)
    assert dn.any() or not expect_resets
    np.testing.assert_array_equal(nxt_obs[dn], p.pool32[dr['reset_idx'][1:]][dn])
    # ---- heads and episode structure, exact
    cm, ts = dr['reset_model'][0].copy(), np.zeros(B, np.int64)
    for t in range(T):
        np.testing.assert_array_equal(tpath[t], ts)
        cm = np.where(dn[t], dr['reset_model'][t + 1], cm)
        ts = np.where(dn[t], 0, ts + 1)
    np.testing.assert_array_equal(dev['last_model'], cm)
    np.testing.assert_array_equal(dev['last_ts'], ts)
    assert dn[tpath == H - 1].all()
    ref = Hh.oracle_rollout(p.dm, p.th, p.pdims, env, p.pool32, dr, B, T, H, mode, determ, teacher_obs=dev['obs'])
    assert np.array_equal(dn, ref['done']) and np.array_equal(tpath, ref['tpath'])
    if env != 'ant' or ant_free_run:
        free = Hh.oracle_rollout(p.dm, p.th, p.pdims, env, p.pool32, dr, B, T, H, mode, determ)
        assert np.array_equal(dn, free['done']) and np.array_equal(tpath, free['tpath'])
    if env != 'ant':
        assert np.array_equal(dn, tpath == H - 1)
    elif expect_resets:
        assert (dn & (tpath < H - 1)).any()                           # some episodes did end on the state
    # ---- normals
    sd = np.exp(np.maximum(p.th[-na:], O.LOG_MIN_STD))
    bound = TOL.PHILOX_NORMAL
    extra_act = np.zeros((T, B, na))
    if determ:
        np.testing.assert_array_equal(dev['act'], dev['mean'])
    else:
        z = (dev['act'] - dev['mean']) / sd
        keep = (rad['eps'] >= SMALL_R) if 'eps' in own else np.ones(z.shape, bool)
        share = 1.0 - keep.mean()
        err = np.abs(z - dr['eps'])
        worst = float(err[keep].max())
        print('    PHILOX_NORMAL %s %s worst %.4g excluded %.3g (%d of %d; worst among them %.3g)' % (
            label, 'drawn' if 'eps' in own else 'floor', worst, share, int((~keep).sum()), keep.size, float(err[~keep].max()) if (~keep).any() else 0.0))
        if form is not None:
            REPORT[(form, 'normal')] = max(REPORT.get((form, 'normal'), 0.0), worst / bound)
        assert share <= EXCLUDE_CAP, share
        assert worst <= bound, worst
        if 'eps' in own:
            extra_act = bound * sd * np.where(keep, 1.0, SMALL_R / np.maximum(rad['eps'], 1e-300))
    # ---- the step, teacher-forced
    extra_tb = extra_act.max(axis=2)
    extra_next = np.repeat(extra_tb[:, :, None], ns, axis=2)
    if mode == 'model_mean_std' and 'sel_noise' in own:
        grow = np.where(rad['sel_noise'] >= SMALL_R, 1.0, SMALL_R / np.maximum(rad['sel_noise'], 1e-300))
        assert (grow > 1.0).mean() <= EXCLUDE_CAP
        for t in range(T):
            heads = O.dynamics_forward_all(p.dm, dev['obs'][t], np.clip(ref['act'][t], -1, 1))
            extra_next[t] += bound * np.std(heads, axis=0) * grow[t]
    _close(dev['mean'], ref['mean'], mean_tol or tol, 0.0, 'mean', form)
    _close(dev['act'], ref['act'], act_tol or tol, extra_act, 'act', form)
    _close(dev['rew'], ref['rew'], rew_tol or tol, extra_next.max(axis=2) + extra_tb, 'rew', form)
    _close(nxt_obs[~dn], ref['next'][~dn], tol, extra_next[~dn], 'next', form)
