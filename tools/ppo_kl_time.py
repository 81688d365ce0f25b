#!/usr/bin/env python3
"""Time one epoch of the 'ppo' update with the KL penalty (Engine.ppo_kl_update(n_epochs=1): the loss + KL launch and its reduction, the OP_PPOKL
gradient kernel, the reduction with the entropy term and the Adam step) against what it is made of, one epoch of Engine.ppo_update plus one
Engine.loss_kl on the same batch: C1's update shape (Swimmer, policy 2x32, N = 5000 x 100, MFMA family) and the humanoid params-file shape
(100-50-25, N = 50 000, fused3).  The OP_PPO and OP_LOSSKL kernels of this library are the parent commit's instruction streams up to kernarg
offsets (the disassembly note in profiles/r09_ppo_kl.txt), so the sum is timed in this library, interleaved with the new epoch; its own
round-to-round spread is the margin.  theta is moved off theta_old and step_size is half the mean KL there: the gate is open (the closed gate is
timed too).  lr = 0: every call sees the same theta.
Usage: ppo_kl_time.py [--out FILE] [--reps N] [--rounds R]"""
import sys, os, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import metrpo_amd
from ppo_time import timed


def run(label, env, ph, N, reps, rounds, clip=0.1, beta=3.0):
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    assert eng.set_update_path(True) is True
    family = 'fused3' if len(ph) == 3 else 'MFMA'
    th = metrpo_amd.xavier_policy_theta(eng.ns, ph, eng.na, 1.0, seed=0)
    eng.set_policy(th)
    rng = np.random.RandomState(0)
    obs = torch.as_tensor(rng.randn(N, eng.ns).astype(np.float32) * 0.5, device='cuda')
    eps = torch.as_tensor(rng.randn(N, eng.na).astype(np.float32), device='cuda')
    act, mean = eng.policy_actions(obs, eps)
    adv = torch.as_tensor(rng.randn(N).astype(np.float32), device='cuda')
    ls = torch.as_tensor(th[-eng.na:].astype(np.float32), device='cuda')
    b = eng.make_batch(obs, act, adv, mean, ls)
    eng.set_policy((th + 0.01 * rng.randn(th.size)).astype(np.float32))
    mkl = float(eng.loss_kl(b)[1].item())
    g0, g1 = eng.ppo_loss_grad(b, clip, 0.01), eng.ppo_kl_loss_grad(b, clip, 0.01, beta, 0.5 * mkl)
    share = float(((g1[1:] - g0[1:]).norm() / g0[1:].norm()).item())
    kw = dict(n_epochs=1, clip_lr=clip, entropy_bonus_coeff=0.01, lr=0.0, want_losses=False)
    new_open = lambda: eng.ppo_kl_update(b, kl_penalty=beta, step_size=0.5 * mkl, **kw)
    new_closed = lambda: eng.ppo_kl_update(b, kl_penalty=beta, step_size=2.0 * mkl, **kw)
    ppo = lambda: eng.ppo_update(b, **kw)
    lkl = lambda: eng.loss_kl(b)
    both = lambda: (eng.loss_kl(b), eng.ppo_update(b, **kw))
    for _ in range(2): new_open(); new_closed(); ppo(); lkl(); both()
    t = {k: [] for k in ('open', 'closed', 'ppo', 'lkl', 'both')}
    for _ in range(rounds):                                   # interleaved rounds: drift of the clock hits all sides alike
        for k, fn in (('open', new_open), ('closed', new_closed), ('ppo', ppo), ('lkl', lkl), ('both', both)):
            t[k].append(timed(fn, reps))
    t = {k: np.array(v) for k, v in t.items()}
    md = {k: float(np.median(v)) for k, v in t.items()}
    return ("%-7s %-15s pol=%-13s N=%7d  ppo_kl epoch (gate open) %8.1f us [%.1f, %.1f]  (gate closed %8.1f us)  ppo epoch %8.1f us [%.1f, %.1f]  "
            "loss_kl %8.1f us [%.1f, %.1f]  sum %8.1f us  back-to-back %8.1f us [%.1f, %.1f]  ppo_kl/sum %.3f  ppo_kl/back-to-back %.3f  "
            "(mean_kl %.3g, |g_ppo_kl - g_ppo| / |g_ppo| = %.2f: the penalty is active)" % (
                family, label, ph, N, md['open'], t['open'].min(), t['open'].max(), md['closed'], md['ppo'], t['ppo'].min(), t['ppo'].max(),
                md['lkl'], t['lkl'].min(), t['lkl'].max(), md['ppo'] + md['lkl'], md['both'], t['both'].min(), t['both'].max(),
                md['open'] / (md['ppo'] + md['lkl']), md['open'] / md['both'], mkl, share))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    lines = ["# one PPO epoch with the KL penalty (ppo_kl_update, n_epochs = 1: 4 launches) vs one ppo_update epoch (2 launches) + one loss_kl (2 launches + its",
             "# output tensor) on the same batch, all stream-ordered without synchronisation.  'sum' adds the two medians timed apart, 'back-to-back' times the",
             "# two calls issued together.  Each round times %d back-to-back calls of each side (CUDA events) after 2 warm-up calls; %d interleaved" % (a.reps, a.rounds),
             "# rounds; medians and [min, max] over the rounds.  Device: %s" % torch.cuda.get_device_name(0),
             "# Margin for 'no more than the sum': the [min, max] spread of the sides over the rounds of the same job."]
    print("\n".join(lines), flush=True)
    for args in [('C1', 'swimmer', (32, 32), 500000), ('params-humanoid', 'humanoid', (100, 50, 25), 50000)]:
        lines.append(run(*args, reps=a.reps, rounds=a.rounds))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")
