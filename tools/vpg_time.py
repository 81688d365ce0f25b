#!/usr/bin/env python3
"""Time one 'vpg' update (Engine.vpg_update: the gradient kernel + the reduction carrying the Adam step) against one TRPO update
(Engine.trpo_update: gradient, 10 CG products, line search) on the same batch, one row per update family, at C1 (Swimmer, policy 2x32,
N = 5000 x 100) and at the swimmer / humanoid params-file shapes (policy_opt_params.vpg.batch_size = 50 000 samples).
Usage: vpg_time.py [--out FILE] [--reps N] [--rounds R]"""
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
    return e0.elapsed_time(e1) / reps


def run(label, env, ph, N, path, reps, rounds):
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
    vpg = lambda: eng.vpg_update(b, want_loss=False)
    trpo = lambda: eng.trpo_update(b)
    for _ in range(2): vpg(); trpo()
    v, t = [], []
    for _ in range(rounds):                                   # interleaved rounds: drift of the clock hits both sides alike
        v.append(timed(vpg, reps)); t.append(timed(trpo, reps))
    v, t = np.array(v), np.array(t)
    return "%-7s %-14s pol=%-13s N=%7d  vpg_update %8.3f ms  trpo_update %8.3f ms  vpg/trpo %.3f  [vpg min %.3f, max %.3f]" % (
        family, label, ph, N, np.median(v), np.median(t), np.median(v) / np.median(t), v.min(), v.max())


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    lines = ["# one vpg_update (stream-ordered, no synchronisation) vs one trpo_update (synchronises on every line-search trial) on the same batch.",
             "# Each round times %d back-to-back calls of each side (CUDA events) after 2 warm-up calls; %d interleaved rounds; medians.  Device: %s"
             % (a.reps, a.rounds, torch.cuda.get_device_name(0))]
    print("\n".join(lines), flush=True)
    for args in [('C1', 'swimmer', (32, 32), 500000, True), ('C1', 'swimmer', (32, 32), 500000, 'gemm'),
                 ('C1', 'swimmer', (32, 32), 500000, False),
                 ('params-swimmer', 'swimmer', (32, 32), 50000, True), ('params-swimmer', 'swimmer', (32, 32), 50000, 'gemm'),
                 ('params-swimmer', 'swimmer', (32, 32), 50000, False),
                 ('params-humanoid', 'humanoid', (100, 50, 25), 50000, True), ('params-humanoid', 'humanoid', (100, 50, 25), 50000, 'gemm')]:
        lines.append(run(*args, reps=a.reps, rounds=a.rounds))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")
