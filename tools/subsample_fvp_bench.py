"""Timings of the subsampled-FVP TRPO update for profiles/r10_subsample_fvp.txt: at C1 (2 x 32, N = 500 000) and params-humanoid (100-50-25,
N = 50 000), per subsample factor f: the Fisher-vector-product kernel uncached on the gathered sub-batch against the cached product of a whole
solve on a compact batch of the same rows (HIP events around the kernel, option TIME_FVP), the gather (us, bytes moved, GB/s), the update
(Engine.trpo_update) and the whole ConjugateGradientOptimizer.optimize (draw + gather + update).  Interleaved rounds, medians with [min, max].

    python tools/subsample_fvp_bench.py [--rounds 7] [--only-f1]     # --only-f1: the f = 1.0 update alone (to time another checkout in the same session)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.environ.get('METRPO_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metrpo_amd                                              # noqa: E402
from metrpo_amd.engine import xavier_policy_theta             # noqa: E402
from metrpo_amd.optimizer import ConjugateGradientOptimizer    # noqa: E402

SHAPES = {'C1': ('swimmer', (32, 32), 500000), 'humanoid': ('humanoid', (100, 50, 25), 50000)}
FACTORS = (1.0, 0.5, 0.2, 0.1)


def problem(env, ph, N, seed=0):
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    theta = xavier_policy_theta(eng.ns, ph, eng.na, init_std=1.0, seed=seed)
    g = torch.Generator(device='cuda'); g.manual_seed(seed)
    obs = torch.randn(N, eng.ns, generator=g, device='cuda') * 0.5
    eng.set_policy(theta)
    mean = eng.policy_actions(obs)[1].clone()
    act = mean + torch.randn(N, eng.na, generator=g, device='cuda')
    adv = torch.randn(N, generator=g, device='cuda'); adv = (adv - adv.mean()) / adv.std()
    ls = torch.zeros(eng.na, device='cuda')
    return eng, theta, (obs, act, adv, mean, ls)


def timed(fn, reps):
    """us per call: events around `reps` back-to-back calls (the calls synchronise themselves where the update does)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def med(xs):
    return '%8.1f [%8.1f, %8.1f]' % (float(np.median(xs)), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--only-f1', action='store_true')
    a = ap.parse_args()
    for name, (env, ph, N) in SHAPES.items():
        eng, theta, (obs, act, adv, mean, ls) = problem(env, ph, N)
        batch = eng.make_batch(obs, act, adv, mean, ls)
        th = torch.as_tensor(theta, device='cuda')

        def update(fvp=None):
            eng.set_policy(th)
            return eng.trpo_update(batch, fvp_batch=fvp) if fvp is not None else eng.trpo_update(batch)
        update()                                               # warm-up: workspaces, code objects
        if a.only_f1:
            xs = [timed(update, 5) for _ in range(a.rounds)]
            print('%-9s update f=1.0 (set_policy + trpo_update) us: %s' % (name, med(xs)))
            continue
        rows = {}
        subs = {}
        for f in FACTORS:
            m = int(N * f)
            idx = torch.randperm(N, device='cuda')[:m].to(torch.int32)
            subs[f] = (m, idx)
            eng.trpo_update(batch, fvp_batch=eng.subsample_batch(batch, idx)); update()
        for r in range(a.rounds):                              # interleaved: every quantity once per round
            for f in FACTORS:
                m, idx = subs[f]
                row = rows.setdefault(f, dict(gather=[], upd=[], opt=[], fvp_unc=[], fvp_cached=[]))
                row['gather'].append(timed(lambda: eng.subsample_batch(batch, idx, n_global_sub=m), 20))
                sub = eng.subsample_batch(batch, idx, n_global_sub=m)
                row['upd'].append(timed((lambda: update(sub)) if f < 1.0 else update, 5))
                opt = ConjugateGradientOptimizer(subsample_factor=f, seed=r); opt.update_opt(leq_constraint=(None, 0.01))
                row['opt'].append(timed(lambda: (eng.set_policy(th), opt.optimize(eng, batch)), 5))
                # kernel-only: the uncached product on the gathered rows ...
                eng.set_option('TIME_FVP', '1'); eng.fvp_kernel_us()
                update(sub); row['fvp_unc'].append(eng.fvp_kernel_us()[0])
                # ... and the cached product of a whole solve on a compact batch of the same rows
                il = idx.long()
                compact = eng.make_batch(obs[il], act[il], adv[il], mean[il], ls)
                eng.set_policy(th); eng.trpo_update(compact); row['fvp_cached'].append(eng.fvp_kernel_us()[0])
                eng.set_option('TIME_FVP', None)
        base = float(np.median(rows[1.0]['upd']))
        print('%s  (%s, policy %s, N = %d; %d interleaved rounds, medians [min, max], us)' % (name, env, 'x'.join(map(str, ph)), N, a.rounds))
        for f in FACTORS:
            m, row = subs[f][0], rows[f]
            bytes_moved = m * (4 + 2 * 4 * (eng.ns + eng.na))             # index + read and write of obs and old_mean rows (broadcast log_std, no mask)
            gus = float(np.median(row['gather']))
            print('  f=%.1f m=%7d  FVP kernel uncached(sub) %s  cached(compact) %s' % (f, m, med(row['fvp_unc']), med(row['fvp_cached'])))
            print('             gather %s  %.1f MB -> %.0f GB/s' % (med(row['gather']), bytes_moved / 1e6, bytes_moved / gus / 1e3))
            print('             update %s  ratio to f=1.0: %.3f   optimize (draw + gather + update) %s' % (med(row['upd']), float(np.median(row['upd'])) / base, med(row['opt'])))


if __name__ == '__main__':
    main()
