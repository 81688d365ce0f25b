"""Reference checkpoints on the engine (formats.load / save_policy_and_models, policy.ckpt, <scope>_<i>.ckpt) and the optimizer
state entry points (metrpo_get / set_dyn_adam, metrpo_get / set_policy_adam): a run saved and loaded into a fresh engine
continues bit for bit as the uninterrupted one."""
import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu

SHAPES = [('swimmer', 5, (64, 64), (32, 32)), ('ant', 5, (64, 64), (32, 32))]


def _rms_pair(eng, rng):
    """RunningMeanStd objects whose sums are float32 values (what a TF checkpoint holds) and the normalisers they give."""
    from metrpo_amd import dynamics_training as DT, formats
    ns, na = eng.ns, eng.na
    rin, rdiff = DT.RunningMeanStd(eng, epsilon=0.0, shape=(ns + na,)), DT.RunningMeanStd(eng, epsilon=0.0, shape=(ns,))
    rin.update(torch.as_tensor(rng.randn(300, ns + na) * 0.5 + 0.1, dtype=torch.float32, device=eng.device))
    rdiff.update(torch.as_tensor(rng.randn(300, ns) * 0.05, dtype=torch.float32, device=eng.device))
    torch.cuda.synchronize()
    for r in (rin, rdiff):
        r._sum = r._sum.float().double(); r._sumsq = r._sumsq.float().double()
    stats = [formats.rms_mean_std(r._sum.cpu().numpy().astype(np.float32), r._sumsq.cpu().numpy().astype(np.float32), np.float32(r._count))
             for r in (rin, rdiff)]
    eng.set_normalizers(stats[0][0], stats[0][1], stats[1][0], stats[1][1])
    return rin, rdiff


def _steps(eng, rng_seed, n):
    rng = np.random.RandomState(rng_seed)
    for _ in range(n):
        bs = 64
        x = torch.as_tensor(rng.randn(bs * eng.K, eng.ns + eng.na) * 0.5, dtype=torch.float32, device=eng.device)
        y = x[:, :eng.ns] + torch.as_tensor(rng.randn(bs * eng.K, eng.ns) * 0.01, dtype=torch.float32, device=eng.device)
        eng.train_step(x, y, bs, 1e-3, reg_constant=1e-4)
        x0 = torch.as_tensor(rng.randn(32, eng.ns) * 0.1, dtype=torch.float32, device=eng.device)
        _, grad = eng.bptt_grad(x0, 10, 0.99)
        eng.policy_adam_step(grad, 1e-3, clip_val=10.0)
    torch.cuda.synchronize()


def _same(a, b, what):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b), what


def _state(eng):
    m, v, t = eng.get_train_adam()
    pm, pv, pt = eng.get_policy_adam()
    torch.cuda.synchronize()
    return dict(dyn=eng.get_dynamics().cpu(), theta=eng.get_policy().cpu(), m=m.cpu(), v=v.cpu(), t=t, pm=pm.cpu(), pv=pv.cpu(), pt=pt)


@pytest.mark.parametrize('env,K,dh,ph', SHAPES)
def test_policy_and_models_round_trip_continues_bitwise(tmp_path, env, K, dh, ph):
    import metrpo_amd
    from metrpo_amd import dynamics_training as DT, formats
    src, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, ph, seed=3)
    rin, rdiff = _rms_pair(src, np.random.RandomState(4))
    _steps(src, 10, 3)
    prefix = formats.save_policy_and_models(str(tmp_path), 3, src, rin, rdiff)
    assert prefix.endswith('policy-and-models-3.ckpt')
    assert metrpo_amd.tf_checkpoint.latest_checkpoint(str(tmp_path)) == prefix

    dst = metrpo_amd.Engine(env, K, dh, ph)
    rin2, rdiff2 = DT.RunningMeanStd(dst, 0.0, (dst.ns + dst.na,)), DT.RunningMeanStd(dst, 0.0, (dst.ns,))
    rep = formats.load_policy_and_models(prefix, dst, rin2, rdiff2)
    assert rep['missing'] == [] and rep['unmapped'] == []
    assert len(rep['mapped']) == K * 2 * 3 * 3 + 6 + 7 + 6 * 2 + 4
    a, b = _state(src), _state(dst)
    assert a['t'] == b['t'] == 3 and a['pt'] == b['pt'] == 3
    for k in ('dyn', 'theta', 'm', 'v', 'pm', 'pv'):
        _same(a[k], b[k], k)
    assert float(a['m'].abs().sum()) > 0 and float(a['pm'].abs().sum()) > 0
    for r1, r2 in ((rin, rin2), (rdiff, rdiff2)):
        _same(r1._sum, r2._sum, 'rms sum'); _same(r1._sumsq, r2._sumsq, 'rms sumsq'); assert r1._count == r2._count

    _steps(src, 11, 1)
    _steps(dst, 11, 1)
    a, b = _state(src), _state(dst)
    for k in ('dyn', 'theta', 'm', 'v', 'pm', 'pv'):
        _same(a[k], b[k], 'after one more step: ' + k)
    assert a['t'] == b['t'] == 4

    B, T = 1000, 50
    tr = [e.rollout(B, T, 25, 'step_rand', pool, seed=7) for e in (src, dst)]
    torch.cuda.synchronize()
    for f in ('obs', 'act', 'rew', 'done'):
        _same(getattr(tr[0], f), getattr(tr[1], f), 'rollout ' + f)


def test_model_checkpoint_restores_one_model_only(tmp_path):
    from metrpo_amd import formats
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 5, (64, 64), (32, 32), seed=5)
    before = eng.get_dynamics().cpu().clone()
    prefix = formats.save_model_checkpoint(str(tmp_path), eng, 2)
    assert prefix.endswith('training_dynamics_2.ckpt')
    names = list(formats.tf_checkpoint.list_checkpoint(prefix))
    assert all(n.startswith('training_dynamics/model2/') for n in names) and len(names) == 6
    eng.set_dynamics_model(2, np.random.RandomState(0).randn(eng.dyn_param_count))
    torch.cuda.synchronize()
    assert not torch.equal(eng.get_dynamics().cpu()[2], before[2])
    rep = formats.load_model_checkpoint(prefix, eng, 2)
    torch.cuda.synchronize()
    assert len(rep['mapped']) == 6 and rep['unmapped'] == []
    _same(eng.get_dynamics().cpu(), before, 'all models after the restore')


def test_policy_checkpoint_round_trip(tmp_path):
    import metrpo_amd
    from metrpo_amd import formats
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 5, (64, 64), (32, 32), seed=6)
    prefix = formats.save_policy_checkpoint(str(tmp_path), eng)
    assert prefix.endswith('policy.ckpt')
    names = list(formats.tf_checkpoint.list_checkpoint(prefix))
    assert names == sorted(['training_policy/mean_network/hidden_0/W', 'training_policy/mean_network/hidden_0/b',
                            'training_policy/mean_network/hidden_1/W', 'training_policy/mean_network/hidden_1/b',
                            'training_policy/mean_network/output/W', 'training_policy/mean_network/output/b',
                            'training_policy/output_std_param/param'])
    other = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    other.set_policy(np.zeros(other.P, np.float32))
    rep = formats.load_policy_checkpoint(prefix, other)
    assert len(rep['mapped']) == 7
    _same(other.get_policy(), eng.get_policy(), 'theta')
    pol = metrpo_amd.GaussianMLPPolicy(other)
    pol.set_param_values(theta)
    _same(other.get_policy(), torch.as_tensor(theta, dtype=torch.float32), 'set_param_values')
    with pytest.raises(ValueError, match='parameters'):
        pol.set_param_values(theta[:-1])


def test_adam_state_before_any_step_is_zero_and_settable():
    import metrpo_amd
    eng = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    m, v, t = eng.get_train_adam()
    pm, pv, pt = eng.get_policy_adam()
    torch.cuda.synchronize()
    assert t == 0 and pt == 0
    assert m.shape == (5, eng.dyn_param_count) and pm.shape == (eng.P,)
    for x in (m, v, pm, pv):
        assert float(x.abs().sum()) == 0.0
    rng = np.random.RandomState(1)
    m1, v1 = rng.rand(5, eng.dyn_param_count).astype(np.float32), rng.rand(5, eng.dyn_param_count).astype(np.float32)
    eng.set_train_adam(m1, v1, 9)
    p1, q1 = rng.rand(eng.P).astype(np.float32), rng.rand(eng.P).astype(np.float32)
    eng.set_policy_adam(p1, q1, 4)
    m, v, t = eng.get_train_adam()
    pm, pv, pt = eng.get_policy_adam()
    torch.cuda.synchronize()
    assert t == 9 and pt == 4
    _same(m, torch.as_tensor(m1), 'm'); _same(v, torch.as_tensor(v1), 'v'); _same(pm, torch.as_tensor(p1), 'pm'); _same(pv, torch.as_tensor(q1), 'pv')
    from metrpo_amd._lib import MetrpoError
    with pytest.raises(MetrpoError):
        eng.set_train_adam(m1, v1, -1)
