#!/usr/bin/env python3
"""Time metrpo_score_actions (csrc/score_actions.hip) at a candidate-ranking size and at a planner's size: swimmer, C1 nets (K = 5, 2x64 dynamics),
T = 30, B = 4096 and B = 512 candidates from S = 8 start states, gamma = 0.99.

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up), [min, max] over the rounds:
  fused      (a) Engine.score_actions, the one-launch kernel (+ nothing else: ret only)
  replay     (b) what the library offered before for the same numbers: K calls of Engine.rollout_actions(eps_rand, model=k), each writing its
                 [T+1, B, ns] trajectory, then the discount-and-sum in torch (float64, mask included) -- same process, same rounds
  replay-k   the K rollout_actions calls of (b) alone (no torch)
  generic    (c) Engine.score_actions(force_generic=True): per head the step loop, then the reduction kernel
  fused+agg  (a) with ret_mean / ret_std (the second small launch)
Parity printed with the times: (a) against (b) in fp32 ulps of the return (the step arithmetic is shared: <= 1), (a) against (c) relative.
Usage: score_actions_time.py [--out FILE] [--reps N] [--rounds R] [--T 30] [--sizes 4096,512] [--S 8] [--terminal-value | --terminal-mlp]
--terminal-value: with a terminal value set (metrpo_set_terminal_value: w1 ~ 0.5 N(0, 1), w2 ~ 0.1 N(0, 1), one bias ~ N(0, 1) for every candidate: the sides of this tool differ in S).
--terminal-mlp: with the value's MLP form set instead (metrpo_set_terminal_value_mlp: a 32 x 32 tanh net, W0 ~ N(0, 1) / sqrt(ns), W1 ~ N(0, 1) / sqrt(32),
W2 ~ 2 N(0, 1) / sqrt(32), biases 0.1 N(0, 1), one bias ~ N(0, 1) for every candidate)."""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def rounds_of(sides, rounds, reps):
    for _, fn, _ in sides: fn(); fn()
    t = {k: [] for k, _, _ in sides}
    for _ in range(rounds):                                    # interleaved rounds: drift of the clock hits all sides alike
        for k, fn, div in sides:
            t[k].append(timed(fn, max(1, reps // div)))
    return {k: np.array(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--T', type=int, default=30)
    ap.add_argument('--S', type=int, default=8)
    ap.add_argument('--sizes', default='4096,512')
    ap.add_argument('--terminal-value', action='store_true')
    ap.add_argument('--terminal-mlp', action='store_true')
    a = ap.parse_args()
    env, K, T, S, gamma = 'swimmer', 5, a.T, a.S, 0.99
    dm, theta, pdims, pool = O.make_problem(env, K=K, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=0, n_pool=64)
    eng = metrpo_amd.Engine(env, K, (64, 64), (32, 32))
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    dev = eng.device
    rng = np.random.RandomState(0)
    if a.terminal_value:                                       # draws of its own: the candidates below are the same with and without
        tvr = np.random.RandomState(1)
        eng.set_terminal_value(0.5 * tvr.randn(dm.ns), 0.1 * tvr.randn(dm.ns), tvr.randn(1))
    if a.terminal_mlp:
        if a.terminal_value:
            ap.error('--terminal-value and --terminal-mlp: one form at a time')
        tvr, h = np.random.RandomState(1), 32
        net = [tvr.randn(dm.ns, h) / np.sqrt(dm.ns), 0.1 * tvr.randn(h), tvr.randn(h, h) / np.sqrt(h), 0.1 * tvr.randn(h), 2.0 * tvr.randn(h) / np.sqrt(h), 0.1 * tvr.randn(1)]
        eng.set_terminal_value_mlp(np.concatenate([x.reshape(-1) for x in net]), (h, h), tvr.randn(1))
    lines = ["# metrpo_score_actions%s: %s, K = %d, 2x64 dynamics, T = %d, S = %d start states, gamma = %g.  %d interleaved rounds of %d back-to-back calls"
             % (" with a terminal value" if a.terminal_value else (" with an MLP terminal value" if a.terminal_mlp else ""), env, K, T, S, gamma, a.rounds, a.reps),
             "# (replay and generic: %d), CUDA events, 2 warm-up calls each; medians and [min, max] over the rounds.  Device: %s" % (max(1, a.reps // 4), torch.cuda.get_device_name(0))]
    for B in [int(x) for x in a.sizes.split(',')]:
        init = torch.as_tensor(pool[rng.randint(len(pool), size=S)].astype(np.float32), device=dev)
        starts = init[torch.arange(B, device=dev) // (B // S)].contiguous()
        acts = torch.as_tensor((1.5 * rng.randn(T, B, dm.na)).astype(np.float32), device=dev)
        out_a = {'ret': torch.empty(K, B, dtype=torch.float32, device=dev)}
        out_g = {'ret': torch.empty(K, B, dtype=torch.float32, device=dev)}
        out_m = {w: torch.empty((K, B) if w == 'ret' else (B,), dtype=torch.float32, device=dev) for w in ('ret', 'ret_mean', 'ret_std')}
        traj = [(torch.empty(T + 1, B, eng.ns, dtype=torch.float32, device=dev), torch.empty(T, B, dtype=torch.float32, device=dev),
                 torch.empty(T, B, dtype=torch.uint8, device=dev)) for _ in range(K)]
        disc = (gamma ** torch.arange(T, dtype=torch.float64, device=dev)).view(T, 1)
        ret_b = torch.empty(K, B, dtype=torch.float32, device=dev)

        def replay_k():
            for k in range(K):
                eng.rollout_actions(starts, acts, 'eps_rand', model=k, out=traj[k])

        def replay():
            replay_k()
            for k in range(K):
                _, rew, done = traj[k]
                alive = torch.ones(T, B, dtype=torch.float64, device=dev)
                alive[1:] = torch.cumprod(1.0 - done[:-1].double(), dim=0)
                ret_b[k] = (disc * alive * rew.double()).sum(dim=0).float()

        fused = lambda: eng.score_actions(init, acts, gamma=gamma, out=out_a)
        generic = lambda: eng.score_actions(init, acts, gamma=gamma, force_generic=True, out=out_g)
        fused_agg = lambda: eng.score_actions(init, acts, gamma=gamma, want=('ret', 'ret_mean', 'ret_std'), out=out_m)
        fused(); path_a = eng.last_score_actions_kernel()
        generic(); path_c = eng.last_score_actions_kernel()
        replay(); path_b = eng.last_rollout_actions_kernel()
        torch.cuda.synchronize()
        ra, rb, rc = out_a['ret'].double().cpu().numpy(), ret_b.double().cpu().numpy(), out_g['ret'].double().cpu().numpy()
        ulps = float((np.abs(ra - rb) / np.spacing(np.abs(rb).astype(np.float32)).astype(np.float64)).max())
        rel = float((np.abs(ra - rc) / np.maximum(np.abs(rc), 1e-3)).max())
        r = rounds_of([('fused', fused, 1), ('replay', replay, 4), ('replay-k', replay_k, 4), ('generic', generic, 4), ('fused+agg', fused_agg, 1)], a.rounds, a.reps)
        md = {k: float(np.median(v)) for k, v in r.items()}
        fmt = lambda k: "%9.1f us [%.1f, %.1f]" % (md[k], r[k].min(), r[k].max())
        lines += ["B = %d (%d tiles x %d heads = %d waves):" % (B, (B + 15) // 16, K, (B + 15) // 16 * K),
                  "  (a) score_actions, %-7s                         %s" % (path_a, fmt('fused')),
                  "      ... with ret_mean / ret_std                   %s" % fmt('fused+agg'),
                  "  (b) %d x rollout_actions (%s) + torch sum       %s   (b) / (a) %.2f x; the %d calls alone %s" % (K, path_b, fmt('replay'), md['replay'] / md['fused'], K, fmt('replay-k')),
                  "  (c) score_actions, %-7s                         %s   (c) / (a) %.2f x" % (path_c, fmt('generic'), md['generic'] / md['fused']),
                  "  parity: (a) against (b) %.2f fp32 ulp of the return at worst; (a) against (c) %.3g relative at worst" % (ulps, rel)]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
