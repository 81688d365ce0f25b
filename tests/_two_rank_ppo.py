"""Helper of tests/test_gpu_ppo.py::test_two_ranks_on_one_gpu_equal_one_rank: 2 processes (gloo) on cuda:0 attach the one-shot direct
all-reduce (comm.hip) and run one fused PPO update of three epochs (metrpo_ppo_update) on half of a fixed batch each.  Every rank asserts
that all ranks ended with bit-identical theta, Adam state and losses; rank 0 writes them."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
import test_gpu_ppo as T          # noqa: E402


def same_on_all_ranks(a, world):
    got = [None] * world
    dist.all_gather_object(got, np.ascontiguousarray(a).tobytes())
    return all(g == got[0] for g in got)


def main(out_path):
    import metrpo_amd
    dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    cs = T.case('mfma', epochs=3, ent=0.02, lr=1e-3)
    env, ph, path, N, expect = T.FAMILIES['mfma']
    eng = metrpo_amd.Engine(env, 2, (64, 64), ph)
    eng.set_policy(cs['theta'])
    eng.set_update_path(path)
    comm = metrpo_amd.Comm()
    assert comm.attach_engine(eng, transport='one-shot') == 'one-shot'
    m0, v0, t0 = T._adam_state(eng.P, 2)
    eng.set_policy_adam(m0, v0, t0)
    lo, hi = rank * N // world, (rank + 1) * N // world
    batch = eng.make_batch(cs['obs'][lo:hi], cs['act'][lo:hi], cs['adv'][lo:hi], cs['old_mean'][lo:hi], cs['old_ls'][0],
                           valid=cs['valid'][lo:hi], n_global=int(cs['valid'].sum()))
    losses = eng.ppo_update(batch, n_epochs=3, clip_lr=cs['clip'], entropy_bonus_coeff=0.02, lr=1e-3)
    torch.cuda.synchronize()
    eng.comm_check()
    theta = eng.get_policy().double().cpu().numpy()
    m, v, t = eng.get_policy_adam()
    m, v = m.double().cpu().numpy(), v.double().cpu().numpy()
    loss = losses.cpu().numpy()
    for a in (theta, m, v, loss):
        assert same_on_all_ranks(a, world), "ranks ended with different vectors"
    if rank == 0:
        np.savez(out_path, theta=theta, m=m, v=v, t=t, loss=loss)
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1])
