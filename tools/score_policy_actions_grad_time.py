#!/usr/bin/env python3
"""Time metrpo_score_policy_actions_grad (csrc/score_policy_actions_grad.hip) at tools/score_actions_grad_time.py's sizes: swimmer, C1 nets (K = 5, 2x64
dynamics, 2x32 policy), T = 30, B = 4096 and B = 512 noise candidates from S = 8 start states, gamma = 0.99.

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up), [min, max] over the rounds:
  pgrad      Engine.score_policy_actions_grad, the fused path (grad and ret: a forward and a reverse launch)
  grad       Engine.score_actions_grad on the same number of candidates in the same run: the yardstick, the open-loop gradient
  pscore     Engine.score_policy_actions in the same run (the forward sweep without its stores)
  generic    Engine.score_policy_actions_grad(force_generic=True)
  pgrad+all  the fused path with grad_mean (the third small launch), lam0 and act_out
Expected pgrad / grad from the matrix-instruction counts per step and tile (swimmer, counted off the source): forward 92 + 30 (policy), reverse
76 + 112 + 22 (the policy's hidden layers) + 28 (its adjoint: 2 x 2 + 8 x 2 + 8) = 360 against 92 + 76 + 112 = 280: 1.29.
Parity printed with the times: fused against generic, rel-L2 of the gradient per head at worst; ret against score_policy_actions in bits.
Usage: score_policy_actions_grad_time.py [--out FILE] [--reps N] [--rounds R] [--T 30] [--sizes 4096,512] [--S 8] [--terminal-value | --terminal-mlp]
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


# matrix instructions per step of one 16-candidate tile, counted off the source for swimmer (NS_KS = 3, NIN_KS = 3, OUT_CB = 1, RK = 2)
MFMA_SWIMMER = dict(dyn_fwd=3 * 4 + 16 * 4 + 16, pol_fwd=3 * 2 + 8 * 2 + 8, dyn_recompute=3 * 4 + 16 * 4, dyn_adjoint=4 * 4 + 16 * 4 + 16 * 2,
                    pol_hidden=3 * 2 + 8 * 2, pol_adjoint=2 * 2 + 8 * 2 + 8)


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
    m = MFMA_SWIMMER
    mine = m['dyn_fwd'] + m['pol_fwd'] + m['dyn_recompute'] + m['dyn_adjoint'] + m['pol_hidden'] + m['pol_adjoint']
    theirs = m['dyn_fwd'] + m['dyn_recompute'] + m['dyn_adjoint']
    lines = ["# metrpo_score_policy_actions_grad%s: %s, K = %d, 2x64 dynamics, 2x32 policy, T = %d, S = %d start states, gamma = %g.  %d interleaved rounds of %d"
             % (" with a terminal value" if a.terminal_value else (" with an MLP terminal value" if a.terminal_mlp else ""), env, K, T, S, gamma, a.rounds, a.reps),
             "# back-to-back calls (generic: %d), CUDA events, 2 warm-up calls each; medians and [min, max] over the rounds.  Device: %s"
             % (max(1, a.reps // 4), torch.cuda.get_device_name(0)),
             "# matrix instructions per step and tile, from the source: %d (forward %d + %d policy; reverse %d + %d + %d policy hidden + %d policy adjoint) against"
             % (mine, m['dyn_fwd'], m['pol_fwd'], m['dyn_recompute'], m['dyn_adjoint'], m['pol_hidden'], m['pol_adjoint']),
             "# %d of metrpo_score_actions_grad: expected ratio %.2f" % (theirs, mine / float(theirs))]
    for B in [int(x) for x in a.sizes.split(',')]:
        init = torch.as_tensor(pool[rng.randint(len(pool), size=S)].astype(np.float32), device=dev)
        noise = torch.as_tensor((0.8 * rng.randn(T, B, dm.na)).astype(np.float32), device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out_f = {'grad': f32(K, T, B, dm.na), 'ret': f32(K, B)}
        out_g = {'grad': f32(K, T, B, dm.na), 'ret': f32(K, B)}
        out_o = {'grad': f32(K, T, B, dm.na), 'ret': f32(K, B)}
        out_m = {'grad': f32(K, T, B, dm.na), 'ret': f32(K, B), 'grad_mean': f32(T, B, dm.na), 'lam0': f32(K, B, dm.ns), 'act_out': f32(K, T, B, dm.na)}
        out_s = {'ret': f32(K, B)}
        pgrad = lambda: eng.score_policy_actions_grad(init, noise, gamma=gamma, out=out_f)
        generic = lambda: eng.score_policy_actions_grad(init, noise, gamma=gamma, force_generic=True, out=out_g)
        pgrad_all = lambda: eng.score_policy_actions_grad(init, noise, gamma=gamma, want=('grad', 'ret', 'grad_mean', 'lam0', 'act_out'), out=out_m)
        grad = lambda: eng.score_actions_grad(init, noise, gamma=gamma, out=out_o)
        pscore = lambda: eng.score_policy_actions(init, noise, gamma=gamma, out=out_s)
        pgrad(); path_f = eng.last_score_policy_actions_grad_kernel()
        generic(); path_g = eng.last_score_policy_actions_grad_kernel()
        grad(); path_o = eng.last_score_actions_grad_kernel()
        pscore(); path_s = eng.last_score_policy_actions_kernel()
        torch.cuda.synchronize()
        gf, gg = out_f['grad'].double().cpu().numpy(), out_g['grad'].double().cpu().numpy()
        rel = max(float(np.linalg.norm(gf[k] - gg[k]) / max(np.linalg.norm(gg[k]), 1e-300)) for k in range(K))
        same = bool(torch.equal(out_f['ret'], out_s['ret']))
        r = rounds_of([('pgrad', pgrad, 1), ('grad', grad, 1), ('pscore', pscore, 1), ('generic', generic, 4), ('pgrad+all', pgrad_all, 1)], a.rounds, a.reps)
        md = {k: float(np.median(v)) for k, v in r.items()}
        fmt = lambda k: "%9.1f us [%.1f, %.1f]" % (md[k], r[k].min(), r[k].max())
        lines += ["B = %d (%d tiles x %d heads):" % (B, (B + 15) // 16, K),
                  "  score_policy_actions_grad, %-7s (grad, ret)       %s   / score_actions_grad %.2f x" % (path_f, fmt('pgrad'), md['pgrad'] / md['grad']),
                  "      ... with grad_mean, lam0 and act_out              %s" % fmt('pgrad+all'),
                  "  score_actions_grad, %-7s (the yardstick)          %s" % (path_o, fmt('grad')),
                  "  score_policy_actions, %-7s                        %s" % (path_s, fmt('pscore')),
                  "  score_policy_actions_grad, %-7s                   %s   generic / fused %.2f x" % (path_g, fmt('generic'), md['generic'] / md['pgrad']),
                  "  parity: fused against generic %.3g rel-L2 of a head's gradient at worst; ret %s score_policy_actions' bits"
                  % (rel, 'is' if same else 'is NOT')]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
