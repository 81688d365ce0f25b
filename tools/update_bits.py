"""SHA-256 of every output of the fused 2 x 32 policy-update kernels (csrc/policy_mfma.hip) on seeded inputs: the record a change of those
kernels that promises the same bits is held to (tests/test_gpu_update_bits.py, fixture tests/golden/update_bits_gfx950.json).

Per environment of tests/update_cases.py::FUSED_ENVS and N in {1, 17, 261} (swimmer also N = 300007, where the tile deal walks its rounds):
  grad/<ols form>/<mask>   surrogate loss + gradient, old log_std per sample ('rows') and broadcast ('bcast'), with and without `valid`
                           (masks: 'none' = no pointer, 'seven' = valid[::7] = 0, at N = 1 'ones' = the one sample valid, through the pointer; every output below too)
  fvp/<mask>               Fisher-vector product as a call of its own (OP_FVP)
  losskl/<theta>/<mask>    loss + mean KL at theta and at a trial theta
  vpg, ppo, ppokl-open, ppokl-closed   the other heads of the gradient kernel (the penalty's gate open and closed)
  trpo                     one TRPO update (gradient, cached solve of 10 products = OP_FVPC, line search): g, step direction, new theta
  vjp/B<b>                 bptt_grad on b initial states, T = 3: the gradient kernel with the mean-adjoint supplied (policy_vjp), 8 b rows
Every hash is of the bytes of the float64 (theta: float32) array the call returns.

  python tools/update_bits.py --out tests/golden/update_bits_gfx950.json      # on the commit whose bits are the record
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = (1, 17, 261)
BIG = {'swimmer': 300007}
VJP_B = (1, 5, 33)
TRIAL_SCALE = 0.02


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(a.tobytes()).hexdigest()


def masks(N):
    """name -> `valid` array (None: no pointer).  valid[::7] = 0 leaves nothing of N = 1, whose launch through the `valid` pointer keeps its one sample."""
    out = {'none': None}
    v = np.ones(N, np.uint8)
    if N >= 2:
        v[::7] = 0
        out['seven'] = v
    else:
        out['ones'] = v
    return out


def env_hashes(env, sizes=None):
    """{key: sha256} of one environment; one engine, every size."""
    import torch
    import helpers as Hh
    from update_cases import FUSED_ENVS
    out = {}
    eng = None
    for N in (sizes or SIZES + ((BIG[env],) if env in BIG else ())):
        seed = 4000 + 97 * FUSED_ENVS.index(env) + (N % 1009)
        dm, th, pdims, obs, act, adv, om, ols = Hh.update_data(env, N, seed=seed)
        rng = np.random.RandomState(seed + 7)
        if N == 1:
            adv = rng.randn(1).astype(np.float32).astype(np.float64)
        th2 = (th + TRIAL_SCALE * rng.randn(th.size)).astype(np.float32).astype(np.float64)
        v = rng.randn(th.size)
        if eng is None:
            eng = Hh.engine_of(env, 2, (64, 64), (32, 32), dm, th)
            assert eng.set_update_path(True) is True
        assert eng.update_path(N) == 'mfma', (env, N, eng.update_path(N))
        pre = '%s/N%d/' % (env, N)
        for mname, valid in masks(N).items():
            for form, ls in (('rows', ols), ('bcast', ols[0])):
                b = eng.make_batch(obs, act, adv, om, ls, valid=valid)
                eng.set_policy(th)
                out[pre + 'grad/%s/%s' % (form, mname)] = sha(eng.loss_grad(b))
                assert eng.last_update_launch()['family'] == 'mfma'
                out[pre + 'losskl/old/%s/%s' % (form, mname)] = sha(eng.loss_kl(b))
                out[pre + 'losskl/trial/%s/%s' % (form, mname)] = sha(eng.loss_kl(b, th2))
                eng.set_policy(th2)
                out[pre + 'ppo/%s/%s' % (form, mname)] = sha(eng.ppo_loss_grad(b, 0.3, 0.01))
                out[pre + 'ppokl-open/%s/%s' % (form, mname)] = sha(eng.ppo_kl_loss_grad(b, 0.3, 0.01, 2.0, 0.01, mean_kl=torch.tensor([0.5], dtype=torch.float64)))
                out[pre + 'ppokl-closed/%s/%s' % (form, mname)] = sha(eng.ppo_kl_loss_grad(b, 0.3, 0.01, 2.0, 0.01, mean_kl=torch.tensor([0.0], dtype=torch.float64)))
                if form == 'rows':
                    eng.set_policy(th)
                    out[pre + 'vpg/%s' % mname] = sha(eng.vpg_loss_grad(b))
                    out[pre + 'fvp/%s' % mname] = sha(eng.fvp(b, v))
                    assert eng.last_update_launch()['op'] == 1
            # the cached products: one whole update (its solve runs OP_FVPC on the gradient launch's activations)
            eng.set_policy(th)
            b = eng.make_batch(obs, act, adv, om, ols[0], valid=valid)
            r = eng.trpo_update(b, want_vectors=True)
            out[pre + 'trpo/g/%s' % mname] = sha(r['g'])
            out[pre + 'trpo/d/%s' % mname] = sha(r['d'])
            out[pre + 'trpo/theta/%s' % mname] = sha(eng.get_policy())
            out[pre + 'trpo/cg_iters/%s' % mname] = int(r['cg_iters_run'])
    eng.set_policy(th)
    rng = np.random.RandomState(977 + FUSED_ENVS.index(env))
    for B in VJP_B:
        x0 = (rng.randn(B, eng.ns) * 0.1).astype(np.float32)
        costs, grad = eng.bptt_grad(x0, 3, 0.99)
        out['%s/vjp/B%d' % (env, B)] = sha(grad)
        out['%s/vjp/B%d/family' % (env, B)] = eng.last_update_launch()['family']
    torch.cuda.synchronize()
    return out


def all_hashes(envs=None):
    from update_cases import FUSED_ENVS
    out = {}
    for env in (envs or FUSED_ENVS):
        out.update(env_hashes(env))
    return out


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]
    rec = {'arch': arch, 'hashes': all_hashes()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d hashes (%s) -> %s' % (len(rec['hashes']), arch, a.out))


if __name__ == '__main__':
    main()
