#!/usr/bin/env python3
"""Time the 'bptt-stochastic' gradient (Philox draws and n_saturates, as BPTT(stochastic=True).step calls it) against the deterministic
'bptt' gradient on the MFMA, GEMM-path (k_dg_pre_mfma / k_dg_pre_mfma3) and generic sweeps.
Usage: bptt_stochastic_time.py [--out FILE] [--reps N] [--rounds R]"""
import sys, os, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import metrpo_amd
from metrpo_amd import synthetic

PATHS = {0: 'generic', 1: 'MFMA', 2: 'GEMM'}


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(env, K, dh, ph, B, T, reps, rounds, generic=False):
    eng = metrpo_amd.Engine(env, K, dh, ph)
    Ws, bs, norm = synthetic.make_dynamics(env, K, dh, seed=0)
    eng.set_dynamics_layers(Ws, bs, norm['in_mean'], norm['in_std'], norm['diff_mean'], norm['diff_std'])
    eng.set_policy(metrpo_amd.xavier_policy_theta(eng.ns, ph, eng.na))
    path = PATHS[eng.set_det_path(not generic)]
    x0 = torch.as_tensor(synthetic.make_pool(env)[:B].astype(np.float32), device='cuda')
    seed = [0]
    def det():
        eng.bptt_grad(x0, T, 1.0)
    def sto():
        seed[0] += 1
        eng.bptt_grad_stochastic(x0, T, 1.0, seed=seed[0], n_saturates=True)
    for _ in range(2): det(); sto()
    d, s = [], []
    for _ in range(rounds):                                   # interleaved rounds: drift of the clock hits both sides alike
        d.append(timed(det, reps)); s.append(timed(sto, reps))
    d, s = np.array(d), np.array(s)
    r = s / d
    return "%-7s %-8s K=%d dyn=%-12s pol=%-13s B=%4d T=%4d  bptt %9.3f ms  stochastic %9.3f ms  ratio median %.3f  [min %.3f, max %.3f]" % (
        path, env, K, dh, ph, B, T, np.median(d), np.median(s), np.median(r), r.min(), r.max())


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    lines = ["# one BPTT gradient: forward sweep, reverse sweep, parameter reduction; stochastic adds the Philox draws in both sweeps, the",
             "# n_saturates count and the log_std reduction.  Each round times %d back-to-back calls of each side (CUDA events) after 2 warm-up"
             % a.reps,
             "# calls; %d interleaved rounds; medians, and the ratio's median and range over the rounds.  Device: %s"
             % (a.rounds, torch.cuda.get_device_name(0))]
    print("\n".join(lines), flush=True)
    for shape, generic in [(('swimmer', 5, (64, 64), (32, 32), 500, 200), False), (('swimmer', 5, (512, 512), (32, 32), 100, 200), False),
                           (('humanoid', 5, (1024, 1024), (100, 50, 25), 32, 100), False),
                           (('swimmer', 5, (64, 64), (16, 16), 500, 200), True)]:
        lines.append(run(*shape, reps=a.reps, rounds=a.rounds, generic=generic))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")
