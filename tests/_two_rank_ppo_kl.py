"""Helper of tests/test_gpu_ppo_kl.py::test_two_ranks_on_one_gpu_equal_one_rank: 2 processes (gloo) on cuda:0 attach the one-shot direct
all-reduce (comm.hip) and run one fused PPO update with the KL penalty, three epochs (metrpo_ppo_kl_update), on half of a fixed batch each.
argv: output file, step_size, kl_penalty.  Every rank asserts that its own share of the mean KL at entry (loss_kl, not summed) lies below
step_size and the ranks' sum above it -- the gate is open only on the global mean -- and that all ranks ended with bit-identical theta, Adam
state, losses and mean KLs; rank 0 writes them."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, 'tests'))
import test_gpu_ppo as T          # noqa: E402
from _two_rank_ppo import same_on_all_ranks          # noqa: E402


def main(out_path, step, beta):
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
    share = eng.loss_kl(batch)[1:2].cpu()                     # this rank's share of the mean KL (a plain call: no exchange)
    total = share.clone()
    dist.all_reduce(total)
    assert float(share) < step < float(total), (float(share), step, float(total))
    losses, kls = eng.ppo_kl_update(batch, n_epochs=3, clip_lr=cs['clip'], entropy_bonus_coeff=0.02, kl_penalty=beta, step_size=step, lr=1e-3,
                                    want_mean_kls=True)
    torch.cuda.synchronize()
    eng.comm_check()
    theta = eng.get_policy().double().cpu().numpy()
    m, v, t = eng.get_policy_adam()
    m, v = m.double().cpu().numpy(), v.double().cpu().numpy()
    loss, kl = losses.cpu().numpy(), kls.cpu().numpy()
    assert abs(kl[0] - float(total)) <= 1e-12 + 1e-9 * float(total)      # the device summed the same two shares
    for a in (theta, m, v, loss, kl):
        assert same_on_all_ranks(a, world), "ranks ended with different vectors"
    if rank == 0:
        np.savez(out_path, theta=theta, m=m, v=v, t=t, loss=loss, kl=kl)
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1], float(sys.argv[2]), float(sys.argv[3]))
