#!/usr/bin/env python3
"""Time metrpo_svg_update (csrc/svg.hip) at the shapes of the 'svg' branch: swimmer at its params-file nets (2x512, n = 15 recorded rollouts of T = 200
steps), swimmer at the C1 nets (2x64, same rollouts), humanoid (2x1024, n = 60, T = 100); K = 2 heads (only head `model` is read).

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up), [min, max] over the rounds:
  update/auto      the whole metrpo_svg_update on the path the library picks (GEMM on all three shapes)
  update/generic   the same call with path = 1 (thread per (sample, output row)); on humanoid 2x1024 one call per round, it is the slow cross-check
  grad/auto        metrpo_svg_grad: the update without its SGD step (same launches: the step rides in the closing kernel)
and once, on the host: the float64 NumPy restatement tests/svg_ref.py of the same gradient (wall clock; --no-numpy skips it).
The split of a call into its parts (Jacobian stage, scan, policy VJP) comes from a kernel trace of this tool run with --trace-run (one shape, a few
calls, no timing): rocprofv3 --kernel-trace --stats -- python tools/svg_time.py --trace-run swimmer512
Usage: svg_time.py [--out FILE] [--reps N] [--rounds R] [--no-numpy] [--trace-run SHAPE]"""
import sys, os, argparse, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import metrpo_amd
from oracle import metrpo_oracle as O

SHAPES = {'swimmer512': ('swimmer', (512, 512), (32, 32), 15, 200), 'swimmer64': ('swimmer', (64, 64), (32, 32), 15, 200),
          'humanoid1024': ('humanoid', (1024, 1024), (100, 50, 25), 60, 100)}


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


def setup(name):
    env, dh, ph, n, T = SHAPES[name]
    dm, theta, pdims, pool = O.make_problem(env, K=2, dyn_hidden=dh, pol_hidden=ph, seed=0, n_pool=max(n, 64))
    dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
    eng = metrpo_amd.Engine(env, 2, dh, ph)
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_policy(theta)
    rng = np.random.RandomState(0)
    obs = np.zeros((n, T, dm.ns), np.float32); act = np.zeros((n, T, dm.na), np.float32)
    s = pool[:n].copy()
    for t in range(T):                                         # recorded rollouts: head 0 under the noisy policy mean
        a = O.policy_mean(theta, pdims, s) + 0.3 * rng.randn(n, dm.na)
        obs[:, t], act[:, t] = s, a
        s = O.dynamics_forward(dm, 0, s, np.clip(a, -1, 1)) + 0.01 * rng.randn(n, dm.ns)
    lens = np.full(n, T, np.int32); lens[1::3] = T - 1; lens[2::3] = max(1, T // 2)
    dev = eng.device
    return eng, dm, theta, pdims, env, obs, act, lens, tuple(torch.as_tensor(x, device=dev) for x in (obs, act, lens))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--trace-run', default=None)
    a = ap.parse_args()
    if a.trace_run:
        eng, _, _, _, _, _, _, _, (o, c, l) = setup(a.trace_run)
        for _ in range(5):
            eng.svg_update(o, c, 0.0, l)
        torch.cuda.synchronize()
        print('trace run: %s, 5 x svg_update on path %s' % (a.trace_run, eng.last_svg_path()))
        return
    lines = ["# metrpo_svg_update: %d interleaved rounds of %d back-to-back calls, CUDA events, 2 warm-up calls each; medians and [min, max] over the rounds." % (a.rounds, a.reps),
             "# ragged lengths (T, T - 1, T / 2, ...), gamma = 1, head 0, lr = 0 (theta stays put over the repetitions).  Device: %s" % torch.cuda.get_device_name(0)]
    for name in ('swimmer512', 'swimmer64', 'humanoid1024'):
        eng, dm, theta, pdims, env, obs, act, lens, (o, c, l) = setup(name)
        slow = name == 'humanoid1024'
        sides = [('update/auto', lambda: eng.svg_update(o, c, 0.0, l), 1), ('grad/auto', lambda: eng.svg_grad(o, c, l), 1),
                 ('update/generic', lambda: eng.svg_update(o, c, 0.0, l, path='generic'), a.reps if slow else 1)]
        for _, fn, _ in sides: fn(); fn()
        eng.svg_update(o, c, 0.0, l); auto = eng.last_svg_path()
        t = {k: [] for k, _, _ in sides}
        for _ in range(a.rounds):
            for k, fn, div in sides:
                t[k].append(timed(fn, max(1, a.reps // div)))
        t = {k: np.array(v) for k, v in t.items()}
        fmt = lambda k: "%11.1f us [%.1f, %.1f]" % (float(np.median(t[k])), t[k].min(), t[k].max())
        env_, dh, ph, n, T = SHAPES[name]
        lines += ["%s: %s, dynamics %s, policy %s, n = %d, T = %d (N = %d samples); auto path: %s" % (name, env_, 'x'.join(map(str, dh)), 'x'.join(map(str, ph)), n, T, n * T, auto),
                  "  svg_update, auto path      %s" % fmt('update/auto'),
                  "  svg_grad, auto path        %s" % fmt('grad/auto'),
                  "  svg_update, generic path   %s   generic / auto %.1f x" % (fmt('update/generic'), float(np.median(t['update/generic'])) / float(np.median(t['update/auto'])))]
        if not a.no_numpy and not slow:
            import svg_ref as R
            t0 = time.perf_counter()
            R.svg_gradient(dm, theta, pdims, env, obs.astype(np.float64), act.astype(np.float64), lens)
            lines += ["  float64 NumPy restatement on this host (one call, wall clock)   %.1f ms" % ((time.perf_counter() - t0) * 1e3)]
        del eng
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
