#!/usr/bin/env python3
"""Time one epoch of the 'ppo' update (Engine.ppo_update(n_epochs=1): the OP_PPO gradient kernel + the reduction carrying the entropy term and
the Adam step) against the two-call form it replaces, Engine.loss_grad followed by Engine.policy_adam_step (the TRPO surrogate's gradient,
its reduction, and the stand-alone Adam kernel: three launches), and against one Engine.vpg_update, on the same batch: C1's shape (Swimmer,
policy 2x32, N = 5000 x 100, MFMA family), the humanoid params-file shape (100-50-25, N = 50 000, fused3) and one GEMM-path shape.  The
gradient kernels of the pair and k_policy_adam are the parent commit's instruction for instruction and its reduction differs in kernarg offsets
only, so the pair is timed in this library (the output says so), interleaved with the PPO epoch; its own round-to-round spread is the margin.
theta is moved off theta_old so that the gate is in both states (the gated gradient's distance from the ungated one is printed).
Usage: ppo_time.py [--out FILE] [--reps N] [--rounds R]"""
import sys, os, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import metrpo_amd


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


def run(label, env, ph, N, path, reps, rounds, clip=0.1):
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    assert eng.set_update_path(path) == path
    family = {'gemm': 'GEMM', False: 'generic', True: 'fused3' if len(ph) == 3 else 'MFMA'}[path]
    th = metrpo_amd.xavier_policy_theta(eng.ns, ph, eng.na, 1.0, seed=0)
    eng.set_policy(th)
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(rng.randn(N, eng.ns).astype(np.float32) * 0.5, device='cuda')
    eps = torch.as_tensor(rng.randn(N, eng.na).astype(np.float32), device='cuda')
    act, mean = eng.policy_actions(obs, eps)
    adv = torch.as_tensor(rng.randn(N).astype(np.float32), device='cuda')
    ls = torch.as_tensor(th[-eng.na:].astype(np.float32), device='cuda')
    b = eng.make_batch(obs, act, adv, mean, ls)
    moved = (th + 0.01 * rng.randn(th.size)).astype(np.float32)
    eng.set_policy(moved)
    lk = eng.loss_grad(b)
    full, gated = eng.ppo_loss_grad(b, 1e9, 0.0), eng.ppo_loss_grad(b, clip, 0.0)
    share = float(((full[1:] - gated[1:]).norm() / full[1:].norm()).item())      # the gated gradient's distance from the ungated one (sums of signed terms: it may exceed 1)
    # lr = 0: every call sees the same theta (the Adam moments still move; they cost nothing more or less for that)
    ppo = lambda: eng.ppo_update(b, n_epochs=1, clip_lr=clip, entropy_bonus_coeff=0.01, lr=0.0, want_losses=False)
    pair = lambda: eng.policy_adam_step(eng.loss_grad(b)[1:], 0.0, clip_val=None)
    vpg = lambda: eng.vpg_update(b, lr=0.0, want_loss=False)
    for _ in range(2): ppo(); pair(); vpg()
    p, q, v = [], [], []
    for _ in range(rounds):                                   # interleaved rounds: drift of the clock hits all sides alike
        p.append(timed(ppo, reps)); q.append(timed(pair, reps)); v.append(timed(vpg, reps))
    p, q, v = np.array(p), np.array(q), np.array(v)
    return ("%-7s %-15s pol=%-13s N=%7d  ppo epoch %8.1f us [%.1f, %.1f]  loss_grad+adam_step %8.1f us [%.1f, %.1f]  ppo/pair %.3f  "
            "vpg_update %8.1f us  ppo/vpg %.3f  (|g_unclipped - g_ppo| / |g_unclipped| = %.2f: the gate is active)" % (
                family, label, ph, N, np.median(p), p.min(), p.max(), np.median(q), q.min(), q.max(), np.median(p) / np.median(q),
                np.median(v), np.median(p) / np.median(v), share))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    lines = ["# one PPO epoch (ppo_update, n_epochs = 1: 2 launches) vs loss_grad + policy_adam_step (3 launches + the host's tensor slice) vs one vpg_update,",
             "# same batch, all stream-ordered without synchronisation.  Each round times %d back-to-back calls of each side (CUDA events) after 2"
             % a.reps,
             "# warm-up calls; %d interleaved rounds; medians and [min, max] over the rounds.  Device: %s" % (a.rounds, torch.cuda.get_device_name(0)),
             "# The loss_grad + policy_adam_step side is THIS library's OP_GRAD path, not a second library built from the parent commit: its gradient",
             "# kernels and k_policy_adam are the parent's instruction for instruction, its reduction k_finalize<false, false> differs from the",
             "# parent's k_finalize<false> in the kernarg offsets of the hidden arguments only (the disassembly check is not this tool's output: in profiles/r08_ppo.txt it is appended by hand below the timing lines).",
             "# Margin for 'not slower': the [min, max] spread of the loss_grad + policy_adam_step side over the rounds of the same job."]
    print("\n".join(lines), flush=True)
    for args in [('C1', 'swimmer', (32, 32), 500000, True), ('params-humanoid', 'humanoid', (100, 50, 25), 50000, True),
                 ('C1 (GEMM path)', 'swimmer', (32, 32), 500000, 'gemm'), ('humanoid (GEMM)', 'humanoid', (100, 50, 25), 50000, 'gemm')]:
        lines.append(run(*args, reps=a.reps, rounds=a.rounds))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")
