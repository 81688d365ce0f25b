#!/usr/bin/env python3
"""Time the 'l-bfgs' policy update: one metrpo_lbfgs_policy minimisation per round (ms per evaluation, against one bptt_grad alone: the
step kernel's and the host loop's share), and the same minimisation driven from the host through tests/lbfgs_ref.py calling
engine.bptt_grad and synchronising on every evaluation (what running scipy on the host would cost).
Usage: lbfgs_time.py [--out FILE] [--rounds R] [--maxiter N]"""
import sys, os, argparse, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
import numpy as np, torch
import metrpo_amd
from metrpo_amd import synthetic
import lbfgs_ref as L

PATHS = {0: 'generic', 1: 'MFMA', 2: 'GEMM'}


def timed(fn, reps=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(env, K, dh, ph, B, T, rounds, maxiter):
    eng = metrpo_amd.Engine(env, K, dh, ph)
    Ws, bs, norm = synthetic.make_dynamics(env, K, dh, seed=0)
    eng.set_dynamics_layers(Ws, bs, norm['in_mean'], norm['in_std'], norm['diff_mean'], norm['diff_std'])
    th0 = metrpo_amd.xavier_policy_theta(eng.ns, ph, eng.na)
    path = PATHS[eng.set_det_path(True)]
    x0 = torch.as_tensor(synthetic.make_pool(env)[:B].astype(np.float32), device='cuda')
    eng.set_policy(th0)
    opts = eng.lbfgs_opts(maxiter=maxiter)
    res = {}

    def dev():
        eng.set_policy(th0)
        res['d'] = eng.lbfgs_policy(x0, T, 1.0, opts)

    def grad():
        eng.bptt_grad(x0, T, 1.0)

    def host():
        eng.set_policy(th0)
        def fg(x):
            eng.set_policy(np.asarray(x).astype(np.float32))
            c, g = eng.bptt_grad(x0, T, 1.0)
            c = c.cpu().numpy()
            return float(np.float32(sum(c.tolist()) / len(c))), g.cpu().numpy().astype(np.float32).astype(np.float64)
        res['h'] = L.minimize(fg, th0.astype(np.float64), maxiter=maxiter)
    dev(); host(); grad()
    d, h, g = [], [], []
    for _ in range(rounds):                                   # interleaved rounds
        d.append(timed(dev) / res['d']['nfev']); g.append(timed(grad, 5)); h.append(timed(host) / res['h'].nfev)
    d, h, g = np.median(d), np.median(h), np.median(g)
    return ("%-7s %-8s K=%d dyn=%-10s pol=%-9s B=%4d T=%4d P=%5d  nfev %3d/%3d  bptt_grad %7.3f ms  lbfgs_policy %7.3f ms/eval (step share %+.3f ms)"
            "  host-driven %7.3f ms/eval  (%.2fx)" % (path, env, K, dh, ph, B, T, eng.P, res['d']['nfev'], res['h'].nfev, g, d, d - g, h, h / d))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--maxiter', type=int, default=30)
    a = ap.parse_args()
    lines = ["# 'l-bfgs' minimisation of the BPTT cost (maxiter %d, scipy's other defaults, lookahead 2): milliseconds per evaluation of one"
             " metrpo_lbfgs_policy call," % a.maxiter,
             "# against one bptt_grad alone (5 back-to-back calls) and the same minimisation driven from the host (lbfgs_ref + bptt_grad + one"
             " synchronisation per evaluation).",
             "# CUDA events, %d interleaved rounds, medians.  Device: %s" % (a.rounds, torch.cuda.get_device_name(0))]
    print("\n".join(lines), flush=True)
    for shape in [('swimmer', 5, (64, 64), (32, 32), 500, 200), ('swimmer', 5, (512, 512), (32, 32), 100, 200)]:
        lines.append(run(*shape, rounds=a.rounds, maxiter=a.maxiter)); print(lines[-1], flush=True)
    if a.out:
        open(a.out, 'w').write("\n".join(lines) + "\n")
