#!/usr/bin/env python3
"""Time the model diagnostic metrpo_model_error (csrc/model_error.hip; env_helpers.py:96-172) at the size of the reference's commented-out call
(model_based_rl.py:619-635): swimmer, C1 nets (K = 5, 2x64 dynamics, 2x32 policy), n = 50 recorded trajectories of T = 100 steps, the reference's
ten horizons (1, 3, 5, 7, 10, 12, 15, 18, 20, 100) -> W = 5000 windows rolled out for hmax = 100 steps.

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up):
  whole        metrpo_model_error, policy actions, ensemble mean (window gather + two fills + the fused rollout + k_pred_error)
  compare      the same call on a caller-made trajectory: k_pred_error alone
  gather       metrpo_model_error_windows alone
  rollout      the yardstick for the rollout's share: metrpo_rollout of THIS library at B = n T, T = hmax with the call's settings (deterministic,
               model_mean, resumed from the window starts, H = hmax + 1) -- the parent's kernels, untouched by the diagnostic
  known        the whole call with known_actions = 1 (hmax launches of the action gather + metrpo_step's thread-per-env kernel): the slow mode
'whole - compare - gather' must agree with 'rollout' within the round-to-round spread of the pair.  k_pred_error is reported as achieved GB/s over
the bytes it must read (rewards, done flags, recorded rewards, and per horizon the predicted and the recorded state of every serving window).
The CPU figure is the float64 NumPy restatement tests/model_error_ref.py on the host this runs on, one process, labelled as such.
Usage: model_error_time.py [--out FILE] [--reps N] [--rounds R] [--n 50] [--T 100]"""
import sys, os, argparse, time, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import metrpo_amd
from metrpo_amd import _lib, model_error as M
from oracle import metrpo_oracle as O
import model_error_ref as R


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--T', type=int, default=100)
    a = ap.parse_args()
    env, K, n, T = 'swimmer', 5, a.n, a.T
    hs = [h for h in M.TIMESTEPS if h <= T]
    hmax, n_h, W = hs[-1], len(hs), n * T
    dm, theta, pdims, pool = O.make_problem(env, K=K, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=0, n_pool=max(n, 64))
    dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
    eng = metrpo_amd.Engine(env, K, (64, 64), (32, 32))
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_policy(theta)
    Os, As, Rs = R.recorded_trajectories(dm, theta, pdims, env, pool, n, T, seed=0)
    dev, ns, na = eng.device, eng.ns, eng.na
    d = lambda x: torch.as_tensor(x, device=dev).contiguous()
    dOs, dAs, dRs = d(Os), d(As), d(Rs)
    sd = torch.empty(n_h, W, ns, dtype=torch.float32, device=dev); cd = torch.empty(n_h, W, dtype=torch.float32, device=dev)
    va = torch.empty(n_h, W, dtype=torch.uint8, device=dev); sums = torch.empty(n_h, 4, dtype=torch.float64, device=dev)
    h_arr = (C.c_int32 * n_h)(*hs)

    def args(known=0, traj=None):
        x = _lib.ModelErrorArgs()
        x.d_Os, x.d_As, x.d_Rs, x.n, x.T, x.hs, x.n_h, x.model, x.known_actions = dOs.data_ptr(), dAs.data_ptr(), dRs.data_ptr(), n, T, h_arr, n_h, -1, known
        x.d_state_diff, x.d_cost_diff, x.d_valid, x.d_sums = sd.data_ptr(), cd.data_ptr(), va.data_ptr(), sums.data_ptr()
        if traj is not None:
            x.d_dbg_obs, x.d_dbg_rew, x.d_dbg_done, x.d_dbg_last_obs = traj.obs.data_ptr(), traj.rew.data_ptr(), traj.done.data_ptr(), traj.last_obs.data_ptr()
        return x

    st = eng._stream()
    call = lambda x: _lib.check(_lib.lib.metrpo_model_error(eng._ctx, C.byref(x), st), eng._ctx)
    # the yardstick rollout, and the trajectory the comparison is timed on
    init = M.model_error_windows(eng, dOs)
    ts0 = torch.zeros(W, dtype=torch.int32, device=dev); md0 = torch.zeros(W, dtype=torch.int32, device=dev)
    traj = eng.alloc_trajectory(W, hmax, hmax + 1)
    roll = lambda: eng.rollout(W, hmax, hmax + 1, 'model_mean', init, determ=True, eval_all_heads=True, out=traj, resume=(init, ts0, md0))
    roll(); torch.cuda.synchronize()
    a_whole, a_cmp, a_known = args(), args(traj=traj), args(known=1)
    sides = (('whole', lambda: call(a_whole)), ('compare', lambda: call(a_cmp)), ('rollout', roll),
             ('gather', lambda: _lib.check(_lib.lib.metrpo_model_error_windows(eng._ctx, C.c_void_p(dOs.data_ptr()), n, T, C.c_void_p(init.data_ptr()), st), eng._ctx)),
             ('known', lambda: call(a_known)))
    call(a_whole); torch.cuda.synchronize()
    family = eng.last_rollout_kernel()
    whole_sums = sums.cpu().numpy().copy()
    # the call's rollout is the yardstick's: same bits out of the comparison on either trajectory
    call(a_cmp); torch.cuda.synchronize()
    same = bool(np.array_equal(whole_sums, sums.cpu().numpy()))
    for _, fn in sides: fn(); fn()
    t = {k: [] for k, _ in sides}
    for _ in range(a.rounds):                                  # interleaved rounds: drift of the clock hits all sides alike
        for k, fn in sides:
            t[k].append(timed(fn, a.reps if k != 'known' else max(1, a.reps // 5)))
    t = {k: np.array(v) for k, v in t.items()}
    md = {k: float(np.median(v)) for k, v in t.items()}
    counts = whole_sums[:, 0]
    read_b = hmax * W * 5 + n * T * 4 + float(np.sum(counts)) * ns * 4 * 2
    write_b = n_h * W * (ns * 4 + 4 + 1)
    t0 = time.perf_counter()
    ref = R.evaluate_model_predictions(dm, theta, pdims, env, Os, Rs, timesteps=hs, model=-1)
    cpu_s = time.perf_counter() - t0
    l1 = whole_sums[:, 1] / counts
    agree = float(np.max(np.abs(l1 - np.array(ref['l1_sum'])) / np.array(ref['l1_sum'])))
    share = md['whole'] - md['compare'] - md['gather']
    spread = max(t['whole'].max() - t['whole'].min(), t['rollout'].max() - t['rollout'].min())
    fmt = lambda k: "%9.1f us [%.1f, %.1f]" % (md[k], t[k].min(), t[k].max())
    lines = [
        "# metrpo_model_error at the reference's commented-out call size: %s, K = %d, 2x64 dynamics, 2x32 policy, n = %d, T = %d, horizons %s" % (env, K, n, T, tuple(hs)),
        "# W = %d windows x hmax = %d steps; rollout family: %s.  %d interleaved rounds of %d back-to-back calls (known: %d), CUDA events, 2 warm-up calls each;" % (
            W, hmax, family, a.rounds, a.reps, max(1, a.reps // 5)),
        "# medians and [min, max] over the rounds.  Device: %s" % torch.cuda.get_device_name(0),
        "whole call (policy actions, ensemble mean)      %s" % fmt('whole'),
        "  k_pred_error alone (caller-made trajectory)   %s   reads %.2f MB -> %.0f GB/s; with its %.2f MB of stores %.0f GB/s" % (
            fmt('compare'), read_b / 1e6, read_b / md['compare'] / 1e3, write_b / 1e6, (read_b + write_b) / md['compare'] / 1e3),
        "  window gather alone                           %s" % fmt('gather'),
        "  rollout share = whole - compare - gather      %9.1f us" % share,
        "yardstick: metrpo_rollout, B = %d, T = %d, same settings   %s   share / yardstick %.3f; difference %.1f us, spread of the pair %.1f us" % (
            W, hmax, fmt('rollout'), share / md['rollout'], share - md['rollout'], spread),
        "k_pred_error on the call's own trajectory and on the yardstick's: sums %s" % ('bit-identical' if same else 'DIFFER'),
        "known_actions = 1 (%d x (action gather + metrpo_step))   %s   %.1f x the policy mode" % (hmax, fmt('known'), md['known'] / md['whole']),
        "CPU: float64 NumPy restatement (tests/model_error_ref.py) of the same call on this host, one process: %.2f s = %.0f x the device call;"
        " l1_sum agrees within %.2g relative" % (cpu_s, cpu_s * 1e6 / md['whole'], agree),
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
