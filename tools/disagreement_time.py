#!/usr/bin/env python3
"""Time metrpo_ensemble_disagreement (csrc/disagreement.hip) on the rows of one C1 rollout: swimmer, K = 5, 2x64 dynamics, 2x32 policy, T = 100 steps of
B = 5000 imagined envs -> N = 500 000 (s, a) rows, want = (score, sums) with one group per step.

Sides, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after 2 warm-up calls each), [min, max] over the rounds:
  fused     the fused kernel + the sums launch
  generic   force_generic: metrpo_step's kernel with d_next_all into the workspace + the reduction kernel + the sums launch
  step      the route a caller had before this entry point: Engine.step(want_all=True), then torch: std over the heads (unbiased=False), the norm over
            the dims, per-step sum / sum of squares / max.  Works on any build of the package: `--root DIR --sides step` imports metrpo_amd from another
            checkout (the parent commit's, built), so the figure is the parent's own.
Also printed for the fused side: its share of the f32 matrix peak (useful FLOPs 2 K N (nin 64 + 64 64 + 64 ns) over the measured time, against
Engine.probe_peaks()), and the agreement of fused and generic scores.
Usage: disagreement_time.py [--out FILE] [--root DIR] [--sides fused,generic,step] [--reps 10] [--rounds 7] [--T 100] [--B 5000]"""
import sys, os, argparse
ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--sides', default='fused,generic,step')
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--T', type=int, default=100)
ap.add_argument('--B', type=int, default=5000)
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import metrpo_amd
from oracle import metrpo_oracle as O


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


def main():
    env, K, hidden, T, B = 'swimmer', 5, (64, 64), a.T, a.B
    N = T * B
    dm, theta, pdims, pool = O.make_problem(env, K=K, dyn_hidden=hidden, pol_hidden=(32, 32), seed=0, n_pool=256)
    dm = dm.astype(np.float32).astype(np.float64)
    eng = metrpo_amd.Engine(env, K, hidden, (32, 32))
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_policy(theta)
    dev = eng.device
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(pool[rng.randint(len(pool), size=N)].astype(np.float32), device=dev)
    act = torch.as_tensor((1.5 * rng.randn(N, dm.na)).astype(np.float32), device=dev)
    sides, names = [], a.sides.split(',')
    if 'fused' in names or 'generic' in names:
        out = dict(score=torch.empty(N, dtype=torch.float32, device=dev), sums=torch.empty(T, 4, dtype=torch.float64, device=dev))
        out_g = {k: torch.empty_like(v) for k, v in out.items()}
    if 'fused' in names:
        sides.append(('fused', lambda: eng.ensemble_disagreement(obs, act, rows_per_group=B, want=('score', 'sums'), out=out)))
    if 'generic' in names:
        sides.append(('generic', lambda: eng.ensemble_disagreement(obs, act, rows_per_group=B, want=('score', 'sums'), force_generic=True, out=out_g)))

    def step_route():
        nall = eng.step(obs, act, 'one_model', want_all=True)[3]
        score = nall.std(dim=0, unbiased=False).norm(dim=1)
        s = score.view(T, B).double()
        return score, s.sum(1), (s * s).sum(1), s.max(1).values
    if 'step' in names:
        sides.append(('step', step_route))
    for _, fn in sides: fn(); fn()
    paths = {}
    if 'fused' in names:
        sides[0][1](); paths['fused'] = eng.last_disagreement_kernel()
    t = {k: [] for k, _ in sides}
    for _ in range(a.rounds):                                  # interleaved rounds: drift of the clock hits all sides alike
        for k, fn in sides:
            t[k].append(timed(fn, a.reps))
    t = {k: np.array(v) for k, v in t.items()}
    lines = ["# metrpo_ensemble_disagreement at the rows of one C1 rollout: %s, K = %d, 2x64 dynamics, N = %d x %d = %d rows, want = (score, sums), one group per step" % (env, K, T, B, N),
             "# package from %s; %d interleaved rounds of %d back-to-back calls, CUDA events, 2 warm-up calls each; medians and [min, max] over the rounds.  Device: %s" % (
                 ROOT, a.rounds, a.reps, torch.cuda.get_device_name(0))]
    label = dict(fused="fused kernel + sums launch", generic="generic path (force_generic)", step="Engine.step(want_all) + torch std / norm / per-step sums")
    for k, _ in sides:
        lines.append("%-58s %9.1f us [%.1f, %.1f]" % (label[k], float(np.median(t[k])), t[k].min(), t[k].max()))
    if 'fused' in names:
        flop = 2.0 * K * N * ((dm.ns + dm.na - dm.n_drop) * 64 + 64 * 64 + 64 * dm.ns)
        peak_tf, _ = eng.probe_peaks()
        us = float(np.median(t['fused']))
        lines.append("fused path ran as: %s; useful %.2f GFLOP -> %.1f TFLOP/s = %.1f %% of the measured f32 matrix peak (%.1f TFLOP/s; the sums launch is inside the time)" % (
            paths['fused'], flop / 1e9, flop / us / 1e6, 100.0 * flop / us / 1e6 / peak_tf, peak_tf))
    if 'fused' in names and 'generic' in names:
        torch.cuda.synchronize()
        d = (out['score'] - out_g['score']).abs().max().item()
        lines.append("fused vs generic: max |score difference| %.3g (scores up to %.3g); sums relative difference %.3g" % (
            d, out['score'].max().item(), ((out['sums'] - out_g['sums']).abs() / out_g['sums'].abs().clamp_min(1e-300)).max().item()))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
