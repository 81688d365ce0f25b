"""How far the ensemble can be trusted: the reference's two model diagnostics (env_helpers.py:96-172 evaluate_model_predictions, :175-269
get_error_distribution; imported by model_based_rl.py:7-8, call sites :619-651 commented out there) on metrpo_model_error (include/metrpo.h).

The real-simulator half of both functions (sample_fixed_init_trajectories, :132-137; the env.step loop, :195-212) is the caller's, as everywhere
in this project: both functions take recorded trajectories.  Everything else runs on the device -- one fused rollout from every window start,
one comparison kernel, the percentiles by torch.quantile -- and only the statistics are read back.
"""
import ctypes as C
import os
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import lib, check

TIMESTEPS = (1, 3, 5, 7, 10, 12, 15, 18, 20, 100)                                   # env_helpers.py:107
_STAT_KEYS = ('100%', '0%', '75%', '25%', '50%', 'avg', 'batch_size')               # :112-129


def _dev_f32(x, dev, shape, name):
    t = torch.as_tensor(x, device=dev).to(torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _check_recorded(engine, Os, As, Rs):
    Os_shape = tuple(np.shape(Os)) if not isinstance(Os, torch.Tensor) else tuple(Os.shape)
    if len(Os_shape) != 3 or Os_shape[2] != engine.ns or Os_shape[1] < 2:
        raise ValueError("Os: expected [n, T + 1, %d] with T >= 1, got %s" % (engine.ns, Os_shape))
    n, T = Os_shape[0], Os_shape[1] - 1
    if n < 1:
        raise ValueError("Os: no trajectory")
    return n, T


def model_error(engine, Os, As, Rs, hs, model=-1, known_actions=False, t0_only=False, signed_diff=False, trajectory=None):
    """metrpo_model_error on device tensors.  Os [n, T+1, ns], As [n, T, na] or None, Rs [n, T]; hs strictly increasing horizons in 1 ... T.
    -> dict(state_diff [n_h, W, ns], cost_diff [n_h, W], valid [n_h, W] uint8, sums [n_h, 4] float64 (count, sum state_diff, sum of its last column,
    sum cost_diff), n, T, W, hs) -- device tensors, nothing synchronised; W = n T windows (n with t0_only), window w = i T + t.
    trajectory = (obs [hmax, W, ns], rew [hmax, W], done [hmax, W] uint8, last_obs [W, ns]): compare this caller-made trajectory, run no rollout."""
    dev = engine.device
    n, T = _check_recorded(engine, Os, As, Rs)
    hs = [int(h) for h in hs]
    Os = _dev_f32(Os, dev, (n, T + 1, engine.ns), 'Os')
    Rs = _dev_f32(Rs, dev, (n, T), 'Rs')
    As = _dev_f32(As, dev, (n, T, engine.na), 'As') if As is not None else None
    if known_actions and As is None:
        raise ValueError("known_actions=True needs the recorded actions As")
    W = n * (1 if t0_only else T)
    n_h = len(hs)
    state_diff = torch.empty(n_h, W, engine.ns, dtype=torch.float32, device=dev)
    cost_diff = torch.empty(n_h, W, dtype=torch.float32, device=dev)
    valid = torch.empty(n_h, W, dtype=torch.uint8, device=dev)
    sums = torch.empty(n_h, 4, dtype=torch.float64, device=dev)
    a = _lib.ModelErrorArgs()
    a.d_Os, a.d_Rs, a.d_As = Os.data_ptr(), Rs.data_ptr(), (As.data_ptr() if As is not None else None)
    a.n, a.T = n, T
    h_arr = (C.c_int32 * max(n_h, 1))(*hs)
    a.hs, a.n_h = h_arr, n_h
    a.model, a.known_actions, a.t0_only, a.signed_diff = int(model), int(bool(known_actions)), int(bool(t0_only)), int(bool(signed_diff))
    a.d_state_diff, a.d_cost_diff, a.d_valid, a.d_sums = state_diff.data_ptr(), cost_diff.data_ptr(), valid.data_ptr(), sums.data_ptr()
    keep = [Os, Rs, As]
    if trajectory is not None:
        hmax = hs[-1] if hs else 0
        obs, rew, done, last = trajectory
        obs = _dev_f32(obs, dev, (hmax, W, engine.ns), 'trajectory obs'); rew = _dev_f32(rew, dev, (hmax, W), 'trajectory rew')
        last = _dev_f32(last, dev, (W, engine.ns), 'trajectory last_obs')
        done = torch.as_tensor(done, device=dev).to(torch.uint8).contiguous()
        if tuple(done.shape) != (hmax, W):
            raise ValueError("trajectory done: expected shape %s, got %s" % ((hmax, W), tuple(done.shape)))
        a.d_dbg_obs, a.d_dbg_rew, a.d_dbg_done, a.d_dbg_last_obs = obs.data_ptr(), rew.data_ptr(), done.data_ptr(), last.data_ptr()
        keep += [obs, rew, done, last]
    check(lib.metrpo_model_error(engine._ctx, C.byref(a), engine._stream()), engine._ctx)
    engine._model_error_keep = keep                                                # alive until the stream has consumed them
    return dict(state_diff=state_diff, cost_diff=cost_diff, valid=valid, sums=sums, n=n, T=T, W=W, hs=hs)


def model_error_windows(engine, Os):
    """metrpo_model_error_windows: the rollout batch of the diagnostic, Os[:, :-1] flattened to [n T, ns] on the device."""
    n, T = _check_recorded(engine, Os, None, None)
    Os = _dev_f32(Os, engine.device, (n, T + 1, engine.ns), 'Os')
    out = torch.empty(n * T, engine.ns, dtype=torch.float32, device=engine.device)
    check(lib.metrpo_model_error_windows(engine._ctx, C.c_void_p(Os.data_ptr()), n, T, C.c_void_p(out.data_ptr()), engine._stream()), engine._ctx)
    engine._model_error_keep = [Os]
    return out


def open_loop_predictions(engine, initial_states, actions, model=-1):
    """Replay recorded actions through the ensemble: the loop of get_error_distribution(known_actions=True), env_helpers.py:216-230, without the
    comparison.  initial_states [n, ns]; actions [n, T, na], trajectory-major as recorded, unclipped (clipped on the device, :216).
    model = -1: the mean over the heads, else that head.  -> (states [n, T+1, ns] with states[:, 0] = initial_states, costs [n, T], done [n, T]
    uint8) device tensors, trajectory-major.  A done (Ant's is_done of the predicted state) neither stops nor resets a trajectory.
    One fused launch on the shapes Engine.last_rollout_actions_kernel() reports as 'fused', step()'s kernel once per step otherwise."""
    dev = engine.device
    init = torch.as_tensor(initial_states, device=dev).to(torch.float32)
    if init.dim() != 2 or init.shape[1] != engine.ns or init.shape[0] < 1:
        raise ValueError("initial_states: expected [n, %d] with n >= 1, got %s" % (engine.ns, tuple(init.shape)))
    n = init.shape[0]
    act = torch.as_tensor(actions, device=dev).to(torch.float32)
    if act.dim() != 3 or act.shape[0] != n or act.shape[2] != engine.na or act.shape[1] < 1:
        raise ValueError("actions: expected [%d, T, %d] with T >= 1, got %s" % (n, engine.na, tuple(act.shape)))
    if not (-1 <= int(model) < engine.K):
        raise ValueError("model = %r is neither -1 (ensemble mean) nor a head below K = %d" % (model, engine.K))
    act_tm = act.transpose(0, 1).contiguous()                                      # time-major [T, n, na], the device layout
    if int(model) < 0:
        obs, rew, done = engine.rollout_actions(init.contiguous(), act_tm, 'model_mean')
    else:
        obs, rew, done = engine.rollout_actions(init.contiguous(), act_tm, 'eps_rand', model=int(model))
    return obs.transpose(0, 1).contiguous(), (-rew).transpose(0, 1).contiguous(), done.transpose(0, 1).contiguous()


def ensemble_disagreement(engine, traj, force_generic=False):
    """Where in an imagined batch the K heads stop agreeing: metrpo_ensemble_disagreement on every visited (s, a) of a rollout.  traj: a Trajectory
    (Engine.rollout) or a DevicePaths (VectorizedSampler.obtain_samples; its .traj); obs [T, B, ns] and act [T, B, na] are used, every row is a
    visited pair, so there is no mask.  -> dict of device tensors (one synchronisation, for the length of by_path_step):
      score [T, B]         ||std over the heads of s'||_2 per row (np.std(next_possible_observations, axis=0), env_helpers.py:625)
      sums [T, 4]          float64 per rollout step, from the device: rows, sum score, sum score^2, max score
      by_step [T]          float64 mean score per rollout step, sums[:, 1] / sums[:, 0]
      by_path_step [L]     float64 mean score by steps since the env's last reset (traj.tpath; L = its largest value + 1; NaN where no row has that
                           count) -- the curve that shows the policy walking out of the model's support.  Formed HERE, on the host side, with torch in
                           float64 (index_add_ over tpath on the device), not by the library
      path_step_count [L]  int64 rows per tpath value."""
    tr = getattr(traj, 'traj', traj)
    obs, act, tpath = tr.obs, tr.act, tr.tpath
    if obs.dim() != 3 or act.dim() != 3 or tuple(tpath.shape) != tuple(obs.shape[:2]):
        raise ValueError("traj: expected time-major obs [T, B, ns], act [T, B, na], tpath [T, B]; got %s, %s, %s"
                         % (tuple(obs.shape), tuple(act.shape), tuple(tpath.shape)))
    r = engine.ensemble_disagreement(obs, act, want=('score', 'sums'), force_generic=force_generic)
    score, sums = r['score'], r['sums']
    idx = tpath.reshape(-1).to(torch.int64)
    L = int(idx.max().item()) + 1 if idx.numel() else 0                             # synchronises: the curve's length is data
    tot = torch.zeros(L, dtype=torch.float64, device=score.device).index_add_(0, idx, score.reshape(-1).to(torch.float64))
    cnt = torch.zeros(L, dtype=torch.int64, device=score.device).index_add_(0, idx, torch.ones_like(idx))
    return dict(score=score, sums=sums, by_step=sums[:, 1] / sums[:, 0], by_path_step=tot / cnt.to(torch.float64), path_step_count=cnt)


def _write_stats(stats, data):
    """write_stats (env_helpers.py:61-70) on a device tensor [N] or [N, ns]; percentiles by linear interpolation, as np.percentile."""
    q = torch.quantile(data.to(torch.float64), torch.tensor([1.0, 0.0, 0.75, 0.25, 0.5], dtype=torch.float64, device=data.device), dim=0)
    q = q.cpu().numpy()
    for row, key in enumerate(('100%', '0%', '75%', '25%', '50%')):
        stats[key].append(q[row])
    stats['avg'].append(data.to(torch.float64).mean(dim=0).cpu().numpy())
    stats['batch_size'].append(int(data.shape[0]))


def write_to_csv(data, timesteps, path):
    """write_to_csv (env_helpers.py:71-81): header 'timesteps' + the sorted keys, one row per horizon, every cell str() of the NumPy value."""
    import csv
    data = {k: np.array(v) for k, v in data.items()}                                # make_values_np_array (:90-92)
    header = sorted(data.keys())
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(['timesteps'] + header)
        for i, timestep in enumerate(timesteps):
            writer.writerow([str(timestep)] + [str(data[h][i]) for h in header])


def _horizons(timesteps, T):
    """The horizons of `timesteps` a recording of T steps can serve, sorted; the others are skipped with a warning (the reference would crash on them)."""
    ts = sorted(set(int(h) for h in timesteps))
    if not ts or ts[0] < 1:
        raise ValueError("timesteps must be positive integers, got %r" % (tuple(timesteps),))
    if len(ts) != len(tuple(timesteps)):
        raise ValueError("timesteps must not repeat, got %r" % (tuple(timesteps),))
    skipped = [h for h in ts if h > T]
    if skipped:
        warnings.warn("evaluate_model_predictions: horizons %s exceed the recorded length T = %d and are skipped" % (skipped, T))
    ts = [h for h in ts if h <= T]
    if not ts:
        raise ValueError("no horizon of %r fits the recorded length T = %d" % (tuple(timesteps), T))
    if len(ts) > _lib.MODEL_ERROR_MAX_HORIZONS:
        raise ValueError("at most %d horizons per call" % _lib.MODEL_ERROR_MAX_HORIZONS)
    return ts


def evaluate_model_predictions(engine, Os, As, Rs, timesteps=TIMESTEPS, model=-1, log_dir=None, count=0):
    """env_helpers.py:96-172 on recorded trajectories Os [n, T+1, ns], As [n, T, na] (unused: the actions are the current policy's, :149), Rs [n, T].
    Returns the reference's `errors` dict: 'timesteps', 'l1_sum', 'l1_state_cost', 'l2_sum' -- which the reference fills with the SAME expression as
    l1_sum (:163, mean of the summed absolute differences); kept -- and 'state_diff' / 'cost_diff' with the '0%', '25%', '50%', '75%', '100%', 'avg'
    and 'batch_size' lists of write_stats, one entry per horizon; plus one extension key, 'dropped': windows per horizon whose rollout reported `done`
    before the horizon (Ant only; the statistics are over the remaining windows).  model = -1: the mean over the heads (avg_prediction, :626), else
    one head.  Horizons above T are skipped with a warning (the reference would crash on them); 'timesteps' lists the ones evaluated.
    With log_dir: state_diff_<count>.csv and cost_diff_<count>.csv in write_to_csv's format."""
    n, T = _check_recorded(engine, Os, As, Rs)
    ts = _horizons(timesteps, T)
    if tuple(np.shape(Rs)) != (n, T):
        raise ValueError("Rs: expected [%d, %d], got %s" % (n, T, tuple(np.shape(Rs))))
    if not (-1 <= int(model) < engine.K):
        raise ValueError("model = %r is neither -1 (ensemble mean) nor a head below K = %d" % (model, engine.K))
    r = model_error(engine, Os, None, Rs, ts, model=model)
    errors = {'timesteps': tuple(ts), 'l2_sum': [], 'l1_sum': [], 'l1_state_cost': [],
              'state_diff': {k: [] for k in _STAT_KEYS}, 'cost_diff': {k: [] for k in _STAT_KEYS}, 'dropped': []}
    sums = r['sums'].cpu().numpy()                                                  # synchronises
    for p, h in enumerate(ts):
        cnt = sums[p, 0]
        if cnt < 1:
            raise RuntimeError("evaluate_model_predictions: every window was dropped at horizon %d (done before the horizon)" % h)
        errors['l1_sum'].append(sums[p, 1] / cnt)                                   # :162
        errors['l2_sum'].append(sums[p, 1] / cnt)                                   # :163
        errors['l1_state_cost'].append(sums[p, 2] / cnt)                            # :164
        m = r['valid'][p].bool()
        _write_stats(errors['state_diff'], r['state_diff'][p][m])                   # :165
        _write_stats(errors['cost_diff'], r['cost_diff'][p][m])                     # :166
        errors['dropped'].append(int(n * (T + 1 - h) - int(cnt)))
    if log_dir is not None:
        write_to_csv(errors['state_diff'], ts, os.path.join(log_dir, 'state_diff_%d.csv' % count))     # :168-169
        write_to_csv(errors['cost_diff'], ts, os.path.join(log_dir, 'cost_diff_%d.csv' % count))       # :170-171
    return errors


def get_error_distribution(engine, initial_states, actions, real_costs, real_final_states, horizon, model=0, known_actions=False):
    """env_helpers.py:214-233 on the results of its real-simulator half (:195-212): initial_states [n, ns], actions [n, horizon, na] as recorded
    (clipped here, :216; read with known_actions only), real_costs [n], real_final_states [n, ns].
    -> (e_cost [n], e_state [n, ns]) float32 NumPy: estimated minus real total cost (:232), final-state difference (:233).  An env whose rollout
    reported `done` before the horizon (Ant) has NaN in both.  model: a head (the call site's training_models[0], :638) or -1 for the mean."""
    init = np.asarray(initial_states, np.float32)
    if init.ndim != 2 or init.shape[1] != engine.ns:
        raise ValueError("initial_states: expected [n, %d], got %s" % (engine.ns, init.shape))
    n, horizon = init.shape[0], int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be positive")
    if not (-1 <= int(model) < engine.K):
        raise ValueError("model = %r is neither -1 (ensemble mean) nor a head below K = %d" % (model, engine.K))
    fin = np.asarray(real_final_states, np.float32)
    rc = np.asarray(real_costs, np.float32)
    if fin.shape != init.shape or rc.shape != (n,):
        raise ValueError("real_final_states / real_costs: expected %s and (%d,), got %s and %s" % (init.shape, n, fin.shape, rc.shape))
    As = None
    if known_actions:
        As = np.asarray(actions, np.float32)
        if As.shape != (n, horizon, engine.na):
            raise ValueError("actions: expected [%d, %d, %d], got %s" % (n, horizon, engine.na, As.shape))
    # the one window per trajectory starts at Os[:, 0] and is compared with Os[:, horizon]; the real total cost enters as the first "reward"
    Os = np.zeros((n, horizon + 1, engine.ns), np.float32); Os[:, 0] = init; Os[:, horizon] = fin
    Rs = np.zeros((n, horizon), np.float32); Rs[:, 0] = -rc
    r = model_error(engine, Os, As, Rs, [horizon], model=model, known_actions=known_actions, t0_only=True, signed_diff=True)
    keep = r['valid'][0].bool().cpu().numpy()
    e_cost = r['cost_diff'][0].cpu().numpy(); e_state = r['state_diff'][0].cpu().numpy()
    e_cost[~keep] = np.nan; e_state[~keep] = np.nan
    return e_cost, e_state
