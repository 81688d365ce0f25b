"""Helper of tests/test_gpu_vpg.py::test_two_ranks_on_one_gpu_equal_one_rank: 2 processes (gloo) on cuda:0 attach the one-shot direct
all-reduce (comm.hip) and run two fused VPG updates (metrpo_vpg_update) on half of a fixed batch each.  Every rank asserts that all ranks
ended with bit-identical theta and Adam state; rank 0 writes them."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
from test_gpu_engine import _update_problem          # noqa: E402


def same_on_all_ranks(a, world):
    got = [None] * world
    dist.all_gather_object(got, np.ascontiguousarray(a).tobytes())
    return all(g == got[0] for g in got)


def main(out_path, path):
    import metrpo_amd
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    eng, th, pdims, obs, act, adv, om, ols = _update_problem(N=6000, seed=29)
    eng.set_update_path({'mfma': True, 'gemm': 'gemm'}[path])
    comm = metrpo_amd.Comm()
    assert comm.attach_engine(eng, transport='one-shot') == 'one-shot'
    rng = np.random.RandomState(4)                                     # test_gpu_vpg._adam_state(eng, 4)
    m0 = (rng.randn(eng.P) * 1e-3).astype(np.float32)
    v0 = (rng.rand(eng.P) * 1e-5 + 1e-6).astype(np.float32)
    eng.set_policy_adam(m0, v0, 5)
    N = len(obs)
    lo, hi = rank * N // world, (rank + 1) * N // world
    batch = eng.make_batch(obs[lo:hi], act[lo:hi], adv[lo:hi], None, None, n_global=N)
    losses = [eng.vpg_update(batch, lr=1e-2) for _ in range(2)]
    torch.cuda.synchronize()
    eng.comm_check()
    theta = eng.get_policy().double().cpu().numpy()
    m, v, t = eng.get_policy_adam()
    m, v = m.double().cpu().numpy(), v.double().cpu().numpy()
    loss = torch.cat(losses).cpu().numpy()
    for a in (theta, m, v, loss):
        assert same_on_all_ranks(a, world), "ranks ended with different vectors"
    if rank == 0:
        np.savez(out_path, theta=theta, m=m, v=v, t=t, loss=loss)
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
