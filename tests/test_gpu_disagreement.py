"""GPU tests of metrpo_ensemble_disagreement (csrc/disagreement.hip): the spread of the K heads' next states at supplied (s, a) rows, against the float64
restatement tests/disagreement_ref.py, against the kernels it shares code with (bit for bit), on both paths, at the tile edges and at a size where a
workgroup strides over many tiles.

Bounds (disagreement_ref.bounds, from tests/tolerances.py, none new): next_all and mean to STEP; std[d] to atol + rtol (max_k |s'_k[d]| + std[d]) -- the
population std is 1-Lipschitz in the heads' errors; score to the 2-norm over the dims of the std bounds; maxdev to twice that; rew_std the same with REWARD at
max_k |r_k|; the generic path on wide nets with wide_or_step(hidden) in place of STEP.  d_sums: count exact, max the max of the returned scores bit for bit,
sums 1e-12 relative of a float64 sum of the returned fp32 scores.  Actions are 1.5 * randn, so the clip acts."""
import numpy as np
import pytest
import torch

import helpers as Hh
import tolerances as TOL
import disagreement_ref as DR

pytestmark = pytest.mark.gpu
ALL = ('score', 'maxdev', 'std', 'mean', 'next_all', 'rew_std', 'sums')
_engines = {}
_worst = {}


def cpu(t):
    return t.detach().cpu().numpy()


def engine(shape):
    if shape not in _engines:
        env, K, hidden, _ = DR.SHAPES[shape]
        dm, theta, _, _ = DR.problem(shape)
        _engines[shape] = Hh.engine_of(env, K, hidden, DR.POL_HIDDEN.get(shape, (32, 32)), dm, theta)
    return _engines[shape]


def assert_follows(tag, got, ref, row):
    """every output of a device result against the restatement; the worst share of each bound is printed first"""
    sh = DR.shares(got, ref, row)
    for k, v in sh.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    print("%s: share of the bounds %s (suite so far %s)" % (tag, {k: round(v, 4) for k, v in sh.items()}, {k: round(v, 4) for k, v in _worst.items()}))
    for k, v in sh.items():
        assert v <= 1.0, "%s: %s is at %.3g of its bound" % (tag, k, v)


def assert_sums(sums, score, valid, rpg):
    want = DR.group_sums(score, np.ones(len(score), bool) if valid is None else valid, rpg)
    assert sums.shape == want.shape
    assert np.array_equal(sums[:, 0], want[:, 0])                                          # the count is exact
    assert np.array_equal(sums[:, 3], want[:, 3])                                          # the max of the returned fp32 scores, bit for bit
    np.testing.assert_allclose(sums[:, 1:3], want[:, 1:3], rtol=1e-12, atol=0)


def run(shape, obs, actions, valid=None, rpg=0, force_generic=False, want=ALL):
    eng = engine(shape)
    a_dev = torch.as_tensor(actions, device=eng.device)
    a_before = a_dev.clone()
    r = eng.ensemble_disagreement(obs, a_dev, valid=valid, rows_per_group=rpg, want=want, force_generic=force_generic)
    kernel = eng.last_disagreement_kernel()
    assert torch.equal(a_dev, a_before)                                                    # d_actions is never written
    return {k: cpu(v) for k, v in r.items()}, kernel


# ---- 1. the fused kernel against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,N,rpg', DR.FUSED_CASES)
def test_fused_against_the_restatement(shape, N, rpg):
    env, K, hidden, _ = DR.SHAPES[shape]
    dm = DR.problem(shape)[0]
    obs, actions = DR.inputs(shape, N)
    ref = DR.reference(shape, N)
    got, kernel = run(shape, obs, actions, rpg=rpg)
    assert kernel == 'fused'
    assert got['score'].shape == (N,) and got['std'].shape == (N, dm.ns) and got['next_all'].shape == (K, N, dm.ns) and got['sums'].dtype == np.float64
    assert_follows("%s N=%d" % (shape, N), got, ref, TOL.STEP)
    assert_sums(got['sums'], got['score'], None, rpg)
    if K == 1:
        assert not got['std'].any() and not got['score'].any() and not got['maxdev'].any() and not got['rew_std'].any()      # exact zeros
    else:
        assert (got['score'] > 0).all()


def test_time_major_input_groups_by_step():
    eng, dm = engine('swimmer'), DR.problem('swimmer')[0]
    obs, actions = DR.inputs('swimmer', 33)
    flat = eng.ensemble_disagreement(obs[:30], actions[:30], rows_per_group=5, want=('score', 'sums'))
    tm = eng.ensemble_disagreement(obs[:30].reshape(6, 5, dm.ns), actions[:30].reshape(6, 5, dm.na), want=('score', 'sums', 'next_all'))
    assert tm['score'].shape == (6, 5) and tm['sums'].shape == (6, 4) and tm['next_all'].shape == (5, 6, 5, dm.ns)
    assert torch.equal(tm['score'].reshape(-1), flat['score']) and torch.equal(tm['sums'], flat['sums'])
    only_sums = eng.ensemble_disagreement(obs[:30], actions[:30], rows_per_group=5, want=('sums',))           # the scores go to a ctx workspace
    assert list(only_sums) == ['sums'] and torch.equal(only_sums['sums'], flat['sums'])
    with pytest.raises(ValueError, match='none of'):
        eng.ensemble_disagreement(obs, actions, want=('variance',))
    with pytest.raises(ValueError, match='actions: expected'):
        eng.ensemble_disagreement(obs, actions[:, :1])


# ---- 2. the offset case: |s'| >> spread, both paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
def test_offset_case(force):
    dm, obs, actions = DR.offset_problem()
    eng = Hh.engine_of('swimmer', dm.K, (64, 64), (32, 32), dm, DR.problem('swimmer')[1])
    ref = DR.disagreement(dm, 'swimmer', obs, actions)
    r = eng.ensemble_disagreement(obs, actions, want=ALL, force_generic=force)
    assert eng.last_disagreement_kernel() == ('generic' if force else 'fused')
    assert_follows("offset %s" % ('generic' if force else 'fused'), {k: cpu(v) for k, v in r.items()}, ref, TOL.STEP)


# ---- 3. the same bits as the kernels it shares code with ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', DR.FUSED)
def test_same_bits_as_rollout_actions_and_step(shape):
    N = 17
    eng = engine(shape)
    K = DR.SHAPES[shape][1]
    obs, actions = DR.inputs(shape, N)
    r = eng.ensemble_disagreement(obs, actions, want=('next_all', 'mean'))
    assert eng.last_disagreement_kernel() == 'fused'
    for k in range(K):
        o, _, _ = eng.rollout_actions(obs, actions[None], 'eps_rand', model=k)
        assert eng.last_rollout_actions_kernel() == 'fused'
        assert torch.equal(r['next_all'][k], o[1]), "head %d differs from rollout_actions" % k
    o, _, _ = eng.rollout_actions(obs, actions[None], 'model_mean')
    assert torch.equal(r['mean'], o[1])
    g = eng.ensemble_disagreement(obs, actions, want=('next_all',), force_generic=True)
    assert eng.last_disagreement_kernel() == 'generic'
    _, _, _, nall = eng.step(obs, actions, 'one_model', want_all=True)
    assert torch.equal(g['next_all'], nall)


# ---- 4. the generic path ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,force', [('wide', False), ('k9', False), ('humanoid', False), ('half_cheetah', True)])
def test_generic_path(shape, force):
    N = 17
    env, K, hidden, _ = DR.SHAPES[shape]
    row = TOL.wide_or_step(hidden)
    obs, actions = DR.inputs(shape, N)
    ref = DR.reference(shape, N)
    got, kernel = run(shape, obs, actions, rpg=5, force_generic=force)
    assert kernel == 'generic'
    assert_follows("%s generic" % shape, got, ref, row)
    assert_sums(got['sums'], got['score'], None, 5)
    nall = engine(shape).step(obs, actions, 'one_model', want_all=True)[3]
    assert np.array_equal(got['next_all'], cpu(nall))
    if force:                                                                              # the two paths agree within the sum of their two bounds
        fused, kernel = run(shape, obs, actions, rpg=5)
        assert kernel == 'fused'
        b = DR.bounds(ref, TOL.STEP)['score'] + DR.bounds(ref, row)['score']
        print("%s fused vs generic score: %.3g of the two bounds" % (shape, np.max(np.abs(fused['score'] - got['score']) / b)))
        assert np.all(np.abs(fused['score'] - got['score']) <= b)


# ---- 5. no write beyond N, skipped rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('shape', ['swimmer', 'ant'])
@pytest.mark.parametrize('N', [17, 1])
def test_no_write_beyond_N(shape, N, force):
    """Each output is the front of a larger allocation whose tail holds a sentinel."""
    eng, dm = engine(shape), DR.problem(shape)[0]
    K, ns, dev = dm.K, dm.ns, eng.device
    obs, actions = DR.inputs(shape, N)
    sizes = dict(score=N, maxdev=N, rew_std=N, std=N * ns, mean=N * ns, next_all=K * N * ns, sums=4 * 4)
    rpg = 5
    guard = {k: torch.full((n + 64,), 777.0, dtype=torch.float64 if k == 'sums' else torch.float32, device=dev) for k, n in sizes.items()}
    r = eng.ensemble_disagreement(obs, actions, rows_per_group=rpg, want=ALL, force_generic=force, out=guard)
    assert eng.last_disagreement_kernel() == ('generic' if force else 'fused')
    plain = eng.ensemble_disagreement(obs, actions, rows_per_group=rpg, want=ALL, force_generic=force)
    torch.cuda.synchronize()
    G = -(-N // rpg)
    for k, n in sizes.items():
        n = 4 * G if k == 'sums' else n
        assert torch.all(guard[k][n:] == 777.0), "%s: written behind its end" % k
        assert not torch.any(guard[k][:n] == 777.0), "%s: a cell in front of its end was not written" % k
        assert torch.equal(guard[k][:n], plain[k].reshape(-1)), k


@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('shape,N', [('swimmer', 33), ('half_cheetah', 17)])
def test_skipped_rows(shape, N, force):
    eng = engine(shape)
    obs, actions = DR.inputs(shape, N)
    valid = np.arange(N) % 3 != 1                                                          # a third of the rows skipped
    obs_nan = obs.copy(); obs_nan[~valid] = np.nan                                         # what a skipped row holds enters no result
    act_nan = actions.copy(); act_nan[~valid] = np.nan
    full = eng.ensemble_disagreement(obs, actions, rows_per_group=5, want=ALL, force_generic=force)
    part = eng.ensemble_disagreement(obs_nan, act_nan, valid=valid, rows_per_group=5, want=ALL, force_generic=force)
    assert eng.last_disagreement_kernel() == ('generic' if force else 'fused')
    v = torch.as_tensor(valid, device=eng.device)
    for k in ('score', 'maxdev', 'rew_std', 'std', 'mean'):
        assert torch.equal(part[k][v], full[k][v]), k                                     # the other rows: the unmasked call, bit for bit
        assert not part[k][~v].any(), k                                                    # skipped rows read 0
    assert torch.equal(part['next_all'][:, v], full['next_all'][:, v]) and not part['next_all'][:, ~v].any()
    assert_sums(cpu(part['sums']), cpu(part['score']), valid, 5)
    assert cpu(part['sums'])[:, 0].sum() == valid.sum()


# ---- 6. nothing else changes ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_else():
    """tests/test_gpu_rollout_actions.py::test_a_known_actions_call_changes_nothing_else for this entry point."""
    dm, theta, _, pool = DR.problem('swimmer')
    eng = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)
    rng = np.random.RandomState(0)
    x = rng.randn(5 * 16, dm.ns + dm.na).astype(np.float32); y = rng.randn(5 * 16, dm.ns).astype(np.float32)
    eng.train_step(x, y, 16, 1e-3)
    eng.policy_adam_step(torch.as_tensor(rng.randn(eng.P), dtype=torch.float64, device=eng.device), 1e-3)
    state = lambda: [eng.get_policy().clone(), eng.get_dynamics().clone()] + [t.clone() if torch.is_tensor(t) else t for t in eng.get_train_adam()] + \
        [t.clone() if torch.is_tensor(t) else t for t in eng.get_policy_adam()]
    before = state()
    roll = lambda: eng.rollout(128, 6, 4, 'step_rand', pool.astype(np.float32), seed=5)
    t1 = roll()
    o1, r1, a1 = t1.obs.clone(), t1.rew.clone(), t1.act.clone()
    eng.rollout_actions(pool[:8].astype(np.float32), np.zeros((2, 8, dm.na), np.float32), 'model_mean')
    kernel, note, ract = eng.last_rollout_kernel(), eng.rollout_note(), eng.last_rollout_actions_kernel()
    assert eng.last_disagreement_kernel() is None
    obs, actions = DR.inputs('swimmer', 33)
    res = []
    for force in (False, True):
        for _ in range(2):                                                                 # two identical calls: identical bits in every output
            res.append(eng.ensemble_disagreement(obs, actions, rows_per_group=5, want=ALL, force_generic=force))
        assert eng.last_disagreement_kernel() == ('generic' if force else 'fused')
        for k in ALL:
            assert torch.equal(res[-1][k], res[-2][k]), k
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note and eng.last_rollout_actions_kernel() == ract
    t2 = roll()                                                                            # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


def test_abi_argument_errors():
    import ctypes as C
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    eng, dm = engine('swimmer'), DR.problem('swimmer')[0]
    dev = eng.device
    obs, act = torch.zeros(4, dm.ns, device=dev), torch.zeros(4, dm.na, device=dev)
    score = torch.full((4,), 555.0, device=dev)

    def args(**kw):
        a = _lib.DisagreementArgs()
        a.N, a.d_obs, a.d_actions, a.d_score = 4, obs.data_ptr(), act.data_ptr(), score.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    call = lambda a: lib.metrpo_ensemble_disagreement(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_ensemble_disagreement(eng._ctx, None, eng._stream()) == -2 and b'args NULL' in err()
    for name in ('d_obs', 'd_actions'):
        assert call(args(**{name: None})) == -2 and b'are required' in err()
    assert call(args(N=-1)) == -1 and call(args(N=2 ** 31)) == -1 and call(args(rows_per_group=-1)) == -1
    assert call(args(N=0)) == 0 and call(args(N=0, d_obs=None)) == 0                        # N == 0: OK, nothing written
    torch.cuda.synchronize()
    assert torch.all(score == 555.0)
    assert call(args()) == 0
    torch.cuda.synchronize()
    assert not torch.any(score == 555.0)
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))                              # before metrpo_set_dynamics: the other diagnostics' error
    assert lib.metrpo_ensemble_disagreement(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_disagreement_kernel() is None


# ---- 7. the host function ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_function_on_a_sampler_rollout():
    import metrpo_amd
    B, H = 32, 6
    eng, dm, theta, pdims, pool = Hh.make_engine('ant', 5, (64, 64), (32, 32), seed=2)
    pool[::3, 2] = 0.21; dm.diff_mean[2] = -0.02                                           # a third of the envs leaves 0.2 <= z <= 1.0 at once: resets
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    policy = metrpo_amd.GaussianMLPPolicy(eng, init_std=1.0, seed=2)
    eng.set_policy(theta)
    nne = metrpo_amd.NeuralNetEnv(env=metrpo_amd.InitStatePool(pool, dm.na), inner_env=None, cost_np='ant', dynamics_in=None, dynamics_outs=eng, sam_mode='step_rand')
    algo = metrpo_amd.TRPO(env=nne, policy=policy, baseline=metrpo_amd.LinearFeatureBaseline(), batch_size=B * H, max_path_length=H, discount=0.99, gae_lambda=0.95,
                           step_size=0.01, sampler_args=dict(n_envs=B))
    algo.start_worker()
    paths = algo.obtain_samples(0)
    tr = paths.traj
    T = tr.obs.shape[0]
    tpath = cpu(tr.tpath)
    assert (cpu(tr.done)[:-1].any(axis=0)).any() and tpath.max() < H and (tpath[1:] == 0).any()              # it resets
    r = metrpo_amd.ensemble_disagreement(eng, paths)
    assert eng.last_disagreement_kernel() == 'fused'
    score = r['score']
    assert score.shape == (T, tr.obs.shape[1]) and r['sums'].shape == (T, 4)
    direct = eng.ensemble_disagreement(tr.obs.reshape(-1, dm.ns), tr.act.reshape(-1, dm.na), want=('score',))
    assert torch.equal(direct['score'], score.reshape(-1))
    np.testing.assert_allclose(cpu(r['by_step']), cpu(score.double().mean(1)), rtol=1e-12, atol=0)
    s64 = cpu(score).astype(np.float64)
    want = np.array([s64[tpath == l].mean() for l in range(tpath.max() + 1)])
    np.testing.assert_allclose(cpu(r['by_path_step']), want, rtol=1e-12, atol=0)
    assert np.array_equal(cpu(r['path_step_count']), np.bincount(tpath.reshape(-1)))
    same = metrpo_amd.ensemble_disagreement(eng, tr)                                       # a Trajectory works as well
    assert torch.equal(same['score'], score)
