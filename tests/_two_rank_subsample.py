"""Helper of tests/test_gpu_subsample_fvp.py::test_two_ranks_subsample_their_own_shares: 2 processes (gloo) on cuda:0 attach the one-shot direct
all-reduce (comm.hip); each takes half of a fixed all-valid batch, gathers its OWN rows of that half (metrpo_subsample_batch) and runs one fused
TRPO update whose Fisher-vector products see the sub-batch (metrpo_trpo_update_fvp).  Every rank asserts that all ranks ended with bit-identical
theta; rank 0 writes it with the update's diagnostics."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
import test_gpu_subsample_fvp as T          # noqa: E402


def same_on_all_ranks(a, world):
    got = [None] * world
    dist.all_gather_object(got, np.ascontiguousarray(a).tobytes())
    return all(g == got[0] for g in got)


def main(out_path):
    import metrpo_amd
    from metrpo_amd.optimizer import ConjugateGradientOptimizer
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    env, ph, path, name, N, seed = T.FAMILIES['mfma']
    d = T.data_of('mfma')
    N -= 1
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    eng.set_policy(d['th'])
    assert eng.set_update_path(path) == path
    comm = metrpo_amd.Comm()
    assert comm.attach_engine(eng, transport='one-shot') == 'one-shot'
    lo, hi = rank * N // world, (rank + 1) * N // world
    batch = eng.make_batch(d['obs'][lo:hi], d['act'][lo:hi], d['adv'][lo:hi], d['om'][lo:hi], d['ols'][0], n_global=N)
    opt = ConjugateGradientOptimizer()
    opt.update_opt(leq_constraint=(None, 0.01))
    out = opt.optimize(eng, batch, comm=comm, subsample_indices=T.rank_indices(N, rank))
    torch.cuda.synchronize()
    eng.comm_check()
    theta = eng.get_policy().double().cpu().numpy()
    assert same_on_all_ranks(theta, world), "ranks ended with different theta"
    assert same_on_all_ranks(np.array([out['beta'], out['kl'], out['loss']]), world)
    if rank == 0:
        np.savez(out_path, theta=theta, beta=out['beta'], n_backtrack=out['n_backtrack'], accepted=out['accepted'], kl=out['kl'])
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
