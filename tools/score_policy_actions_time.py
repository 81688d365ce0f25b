#!/usr/bin/env python3
"""Time metrpo_score_policy_actions (csrc/score_policy_actions.hip) at a candidate-ranking size and at a planner's size: swimmer, C1 nets (K = 5,
2x64 dynamics, 2x32 policy), T = 30, B = 4096 and B = 512 noise sequences from S = 8 start states, gamma = 0.99.

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up), [min, max] over the rounds:
  fused        (a) Engine.score_policy_actions, the one-launch kernel (ret only), with noise
  fused-none   (a) with noise=None (the deterministic policy, B start states: no global load in the step loop)
  fused+act    (a) with act_out (the variant that stores the action of every step)
  open-loop    Engine.score_actions on the same shapes in the same run (the kernel without the policy chain): the ratio (a) / open-loop stands next
               to the matrix-instruction estimate (92 + 30) / 92 = 1.33 for swimmer
  generic      (c) Engine.score_policy_actions(force_generic=True): per head and step the policy launch, the add, the step launch; then the reduction
  host         (d) the host loop the call replaces: per head and step Engine.policy_actions + add + Engine.step, then the discount-and-sum in torch
Parity printed with the times: (a) against (c) and (a) against (d), relative.
Usage: score_policy_actions_time.py [--out FILE] [--reps N] [--rounds R] [--T 30] [--sizes 4096,512] [--S 8] [--terminal-value | --terminal-mlp]
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
    eng.set_policy(theta)
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
    slow = 10                                                  # the launch-per-step sides run reps / slow calls per round
    lines = ["# metrpo_score_policy_actions%s: %s, K = %d, 2x64 dynamics, 2x32 policy, T = %d, S = %d start states, gamma = %g.  %d interleaved rounds of %d"
             % (" with a terminal value" if a.terminal_value else (" with an MLP terminal value" if a.terminal_mlp else ""), env, K, T, S, gamma, a.rounds, a.reps),
             "# back-to-back calls (generic and host: %d), CUDA events, 2 warm-up calls each; medians and [min, max] over the rounds.  Device: %s"
             % (max(1, a.reps // slow), torch.cuda.get_device_name(0))]
    for B in [int(x) for x in a.sizes.split(',')]:
        init = torch.as_tensor(pool[rng.randint(len(pool), size=S)].astype(np.float32), device=dev)
        starts = init[torch.arange(B, device=dev) // (B // S)].contiguous()
        noise = torch.as_tensor((0.5 * rng.randn(T, B, dm.na)).astype(np.float32), device=dev)
        mk = lambda: {'ret': torch.empty(K, B, dtype=torch.float32, device=dev)}
        out_a, out_n, out_g, out_o = mk(), mk(), mk(), mk()
        out_x = dict(mk(), act_out=torch.empty(K, T, B, dm.na, dtype=torch.float32, device=dev))
        disc = (gamma ** torch.arange(T, dtype=torch.float64, device=dev)).view(T, 1)
        ret_h = torch.empty(K, B, dtype=torch.float32, device=dev)
        models = [torch.full((B,), k, dtype=torch.int32, device=dev) for k in range(K)]

        def host():
            for k in range(K):
                s, rews, dones = starts, [], []
                for t in range(T):
                    act = eng.policy_actions(s)[0] + noise[t]
                    s, r, d = eng.step(s, act, 'eps_rand', model_idx=models[k])
                    rews.append(r); dones.append(d)
                rew, done = torch.stack(rews), torch.stack(dones)
                alive = torch.ones(T, B, dtype=torch.float64, device=dev)
                alive[1:] = torch.cumprod(1.0 - done[:-1].double(), dim=0)
                ret_h[k] = (disc * alive * rew.double()).sum(dim=0).float()

        fused = lambda: eng.score_policy_actions(init, noise, gamma=gamma, out=out_a)
        fused_none = lambda: eng.score_policy_actions(starts, None, T=T, gamma=gamma, out=out_n)
        fused_act = lambda: eng.score_policy_actions(init, noise, gamma=gamma, want=('ret', 'act_out'), out=out_x)
        generic = lambda: eng.score_policy_actions(init, noise, gamma=gamma, force_generic=True, out=out_g)
        open_loop = lambda: eng.score_actions(init, noise, gamma=gamma, out=out_o)
        fused(); path_a = eng.last_score_policy_actions_kernel()
        generic(); path_c = eng.last_score_policy_actions_kernel()
        open_loop(); path_o = eng.last_score_actions_kernel()
        host()
        torch.cuda.synchronize()
        ra, rc, rh = out_a['ret'].double().cpu().numpy(), out_g['ret'].double().cpu().numpy(), ret_h.double().cpu().numpy()
        rel_c = float((np.abs(ra - rc) / np.maximum(np.abs(rc), 1e-3)).max())
        rel_h = float((np.abs(ra - rh) / np.maximum(np.abs(rh), 1e-3)).max())
        # two groups of interleaved rounds: the one-launch sides among themselves (the launch-bound sides leave the clocks low for whoever follows
        # them), then the launch-per-step sides, 300 x slower, with the fused call riding along as the common yardstick
        r = rounds_of([('open-loop', open_loop, 1), ('fused', fused, 1), ('fused-none', fused_none, 1), ('fused+act', fused_act, 1)], a.rounds, a.reps)
        r.update({k: v for k, v in rounds_of([('fused-slow-group', fused, 1), ('generic', generic, slow), ('host', host, slow)], a.rounds, a.reps).items()})
        md = {k: float(np.median(v)) for k, v in r.items()}
        fmt = lambda k: "%9.1f us [%.1f, %.1f]" % (md[k], r[k].min(), r[k].max())
        lines += ["B = %d (%d tiles x %d heads = %d waves):" % (B, (B + 15) // 16, K, (B + 15) // 16 * K),
                  "  (a) score_policy_actions, %-7s, with noise        %s" % (path_a, fmt('fused')),
                  "      ... noise=None (B start states)                 %s" % fmt('fused-none'),
                  "      ... with act_out [K, T, B, na]                  %s" % fmt('fused+act'),
                  "  (b) score_actions, %-7s, the same shapes         %s   (a) / (b) %.2f x (matrix-instruction estimate 1.33)" % (path_o, fmt('open-loop'), md['fused'] / md['open-loop']),
                  "  (c) score_policy_actions, %-7s                   %s   (c) / (a) %.1f x" % (path_c, fmt('generic'), md['generic'] / md['fused']),
                  "  (d) host loop: %d x (policy_actions + add + step) + torch sum  %s   (d) / (a) %.1f x" % (K * T, fmt('host'), md['host'] / md['fused']),
                  "      (a) timed among (c) and (d), behind their launch-bound loops:   %s" % fmt('fused-slow-group'),
                  "  parity: (a) against (c) %.3g relative at worst; (a) against (d) %.3g relative at worst" % (rel_c, rel_h)]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
