"""GPU parity of the ensemble dynamics training path vs oracle/dynamics_oracle.py."""
import numpy as np
import pytest
import torch
from conftest import load_golden
from oracle import metrpo_oracle as O
from oracle import dynamics_oracle as D
import helpers as Hh
import tolerances as TOL

pytestmark = pytest.mark.gpu


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def flat_to_layers(flat, dm):
    """[K][Pd] -> Ws, bs lists (W0,b0,W1,b1,... per model)."""
    Ws, bs, o = [], [], 0
    for W, b in zip(dm.Ws, dm.bs):
        n = W.shape[1] * W.shape[2]
        Ws.append(flat[:, o:o + n].reshape(W.shape)); o += n
        bs.append(flat[:, o:o + b.shape[1]]); o += b.shape[1]
    return Ws, bs


def data(dm, n, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, dm.ns + dm.na) * 0.5).astype(np.float32).astype(np.float64)
    x[:, dm.ns:] = np.clip(x[:, dm.ns:], -1, 1)
    y = (x[:, :dm.ns] + rng.randn(n, dm.ns) * 0.1).astype(np.float32).astype(np.float64)
    return x, y


SHAPES = [('swimmer', 5, (64, 64), 1000), ('half_cheetah', 3, (128, 96), 200), ('ant', 4, (512, 512), 256),
          ('humanoid', 2, (256, 128, 64), 100), ('hopper', 5, (16, 8), 37)]


@pytest.mark.parametrize('env,K,dh,bs', SHAPES)
@pytest.mark.parametrize('reg', [0.0, 1e-3])
def test_train_steps_match_oracle(env, K, dh, bs, reg):
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, (32, 32), seed=71)
    for l in range(len(dm.Ws)):     # the engine holds float32 copies: start the oracle from exactly those values
        dm.Ws[l] = dm.Ws[l].astype(np.float32).astype(np.float64); dm.bs[l] = dm.bs[l].astype(np.float32).astype(np.float64)
    for a in ('in_mean', 'in_std', 'diff_mean', 'diff_std'):
        setattr(dm, a, getattr(dm, a).astype(np.float32).astype(np.float64))
    adam = D.AdamState(dm)
    eng.train_reset()
    x, y = data(dm, 4000, 3)
    rng = np.random.RandomState(4)
    for it in range(4):
        idx = rng.randint(len(x), size=bs * K)
        xb, yb = x[idx], y[idx]
        xs, ys = D.split_batch(xb, yb, bs, K)
        ref_losses = D.prediction_losses(dm, xs, ys) + np.array([D.regularizer_loss(dm, k, reg) for k in range(K)])
        got = cpu(eng.train_step(xb, yb, bs, 1e-3, reg))
        np.testing.assert_allclose(got, ref_losses, **TOL.DYN_LOSS)
        D.train_step(dm, adam, xb, yb, bs, 1e-3, reg_constant=reg)
    Ws, bs_ = flat_to_layers(cpu(eng.get_dynamics()), dm)
    for l in range(len(dm.Ws)):
        # Adam moves every weight by ~lr per step whatever the gradient's scale, so a weight whose gradient is at fp32
        # rounding level (|g| ~ 1e-9) can step the other way: demand a fraction of lr for 99.9 % of the entries and the
        # hard bound 4 steps x lr for the rest
        for got_, ref_ in ((Ws[l], dm.Ws[l]), (bs_[l], dm.bs[l])):
            err = np.abs(got_ - ref_)
            assert (err > 5e-5).mean() < 1e-3 and err.max() <= 4.4e-3
    xv, yv = data(dm, 777, 9)
    np.testing.assert_allclose(cpu(eng.eval_losses(xv, yv, reg)), D.validation_losses(dm, xv, yv, reg), **TOL.DYN_EVAL_LOSS)


def test_single_step_gradient_direction():
    """After ONE Adam step from zero moments the update is -lr * sign(g) (|g| >> eps): checks the gradient sign of every weight."""
    env, K, dh, bs = 'swimmer', 3, (64, 64), 500
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, (32, 32), seed=72)
    for l in range(len(dm.Ws)):
        dm.Ws[l] = dm.Ws[l].astype(np.float32).astype(np.float64); dm.bs[l] = dm.bs[l].astype(np.float32).astype(np.float64)
    for a in ('in_mean', 'in_std', 'diff_mean', 'diff_std'):
        setattr(dm, a, getattr(dm, a).astype(np.float32).astype(np.float64))
    x, y = data(dm, bs * K, 5)
    before = cpu(eng.get_dynamics())
    eng.train_reset()
    eng.train_step(x, y, bs, 1e-3)
    delta = cpu(eng.get_dynamics()) - before
    xs, ys = D.split_batch(x, y, bs, K)
    for k in range(K):
        gW, gb = D.model_gradients(dm, k, xs[k], ys[k])
        g = np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in zip(gW, gb)])
        big = np.abs(g) > 1e-5
        assert big.mean() > 0.2
        # first TF-Adam step: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001)/0.1  ->  -lr sqrt(.001) g / (sqrt(.001)|g| + eps)
        expect = -1e-3 * np.sqrt(1e-3) * g[big] / (np.sqrt(1e-3) * np.abs(g[big]) + 1e-8)
        np.testing.assert_allclose(delta[k][big], expect, rtol=5e-3, atol=2e-7)


def test_eval_losses_chunking_and_model_restore():
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 3, (64, 64), (32, 32), seed=73)
    xv, yv = data(dm, 20000, 11)                       # > one 8192-row pass
    np.testing.assert_allclose(cpu(eng.eval_losses(xv, yv)), D.validation_losses(dm, xv, yv), **TOL.DYN_LOSS)   # untrained: no drift
    snap = eng.get_dynamics().clone()
    eng.train_reset()
    for _ in range(3):
        eng.train_step(xv[:300], yv[:300], 100, 1e-2)
    assert not torch.equal(eng.get_dynamics(), snap)
    eng.set_dynamics_model(1, snap[1])
    cur = eng.get_dynamics()
    assert torch.equal(cur[1], snap[1]) and not torch.equal(cur[0], snap[0])


@pytest.mark.parametrize('n', [1, 8193])
def test_eval_losses_params_file_shape(n):
    """eval_losses at the params files' 2 x 1024, K = 5: a single row, and 8193 rows (the second 8192-row pass holds one row)."""
    eng, dm, theta, pdims, pool = Hh.make_engine('half_cheetah', 5, (1024, 1024), (32, 32), seed=76)
    for l in range(len(dm.Ws)):
        dm.Ws[l] = dm.Ws[l].astype(np.float32).astype(np.float64); dm.bs[l] = dm.bs[l].astype(np.float32).astype(np.float64)
    for a in ('in_mean', 'in_std', 'diff_mean', 'diff_std'):
        setattr(dm, a, getattr(dm, a).astype(np.float32).astype(np.float64))
    xv, yv = data(dm, n, 12)
    for reg in (0.0, 1e-3):
        np.testing.assert_allclose(cpu(eng.eval_losses(xv, yv, reg)), D.validation_losses(dm, xv, yv, reg), **TOL.DYN_LOSS)


@pytest.mark.parametrize('dim', [76, 111])
@pytest.mark.parametrize('n', [1, 3, 1001])
def test_rms_accumulate_two_column_blocks(dim, n):
    """k_rms_accumulate with two 64-column blocks (the second one partial), two calls into the same sums: float64 sums of the fp32 rows"""
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 2, (64, 64), (32, 32), seed=78)
    rng = np.random.RandomState(dim + n)
    chunks = [(rng.randn(n, dim) * 1.0 + 2.0).astype(np.float32), (rng.randn(n, dim) * 3.0 + 1.0).astype(np.float32)]
    rsum = torch.full((dim,), 0.25, dtype=torch.float64, device='cuda'); rsumsq = torch.full((dim,), 0.5, dtype=torch.float64, device='cuda')
    for c in chunks:
        eng.rms_accumulate(c, rsum, rsumsq)
    z = np.concatenate(chunks).astype(np.float64)
    np.testing.assert_allclose(cpu(rsum), 0.25 + np.sum(z, axis=0), rtol=1e-12, atol=1e-12 * np.abs(z).sum(0).max())
    np.testing.assert_allclose(cpu(rsumsq), 0.5 + np.sum(z * z, axis=0), rtol=1e-12)


def test_replay_buffer_and_normalizers_match_reference_semantics():
    import metrpo_amd
    from metrpo_amd.dynamics_training import data_collection, RunningMeanStd, push_normalizers
    d = load_golden('dyn_data')
    dc = data_collection(max_size=50, device='cuda')
    np.random.seed(int(d['seed']))
    ai = 0
    for i, (op, n) in enumerate(zip(d['ops'], d['ns'])):
        if op == 0:
            dc.add_data(d['addx%d' % ai], d['addy%d' % ai]); ai += 1
            xb, yb = dc.x, dc.y
        elif op == 1:
            xb, yb = dc.get_next_batch(int(n))
        else:
            xb, yb = dc.sample(int(n))
        np.testing.assert_array_equal(cpu(xb), d['x%d' % i].astype(np.float32)); np.testing.assert_array_equal(cpu(yb), d['y%d' % i].astype(np.float32))
        assert dc.n_data == int(d['n_data'][i]) and dc.cur_idx == int(d['cur_idx'][i])
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 2, (64, 64), (32, 32), seed=74)
    rng = np.random.RandomState(0)
    xa, xb_ = rng.randn(1000, 12) + 2.0, rng.randn(500, 12) * 3.0 + 1.0
    r_in = RunningMeanStd(eng, shape=(12,)); ref = D.RunningMeanStdOracle((12,))
    for chunk in (xa, xb_):
        r_in.update(chunk.astype(np.float32)); ref.update(chunk.astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(cpu(r_in.mean), ref.mean, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(cpu(r_in.std), ref.std, rtol=1e-6, atol=1e-6)
    r_diff = RunningMeanStd(eng, shape=(10,))
    assert np.allclose(cpu(r_diff.std), 1.0)           # epsilon 1e-2 / count 1e-2 -> unit std before any data
    push_normalizers(eng, r_in, r_diff)                # the rollout / training kernels now normalise with the new statistics
    dm.in_mean, dm.in_std = cpu(r_in.mean), cpu(r_in.std)
    dm.diff_mean, dm.diff_std = np.zeros(10), np.ones(10)
    s = pool[:64].astype(np.float32); a = np.zeros((64, 2), np.float32)
    nxt = eng.step(s, a, 'one_model', None, None)[0]
    np.testing.assert_allclose(cpu(nxt), O.dynamics_forward(dm, 0, s.astype(np.float64), a.astype(np.float64)), **TOL.STEP)


def test_add_rollouts_matches_reference_collect_data():
    """product add_rollouts / trajectories_to_pairs vs the reference's collect_data golden (tests/golden/collect_split.npz)."""
    import metrpo_amd
    from collections import OrderedDict
    from metrpo_amd.dynamics_training import data_collection, add_rollouts, trajectories_to_pairs
    from test_oracle_dynamics import collect_split_cases, _Rec
    for d, ci, Os, As, c in collect_split_cases():
        x_all, y_all = trajectories_to_pairs(Os, As)
        scopes = ['s%d' % i for i in range(c['n_scopes'])]
        data = OrderedDict((sc, data_collection(1000, device='cuda')) for sc in scopes)
        val = OrderedDict((sc, data_collection(1000, device='cuda')) for sc in scopes)
        irms, orms = _Rec(), _Rec()
        np.random.seed(c['seed'])
        add_rollouts(x_all, y_all, data, val, c['mode'], c['same'], c['ratio'], irms, orms)
        for si, sc in enumerate(scopes):
            for got, key in ((data[sc].x, 'tx'), (data[sc].y, 'ty'), (val[sc].x, 'vx'), (val[sc].y, 'vy')):
                np.testing.assert_array_equal(cpu(got), d['c%d_s%d_%s' % (ci, si, key)].astype(np.float32))
        assert len(irms.calls) == int(d['c%d_n_rms' % ci])
        for k in range(len(irms.calls)):
            np.testing.assert_array_equal(irms.calls[k], d['c%d_rms_in%d' % (ci, k)]); np.testing.assert_array_equal(orms.calls[k], d['c%d_rms_out%d' % (ci, k)])


def test_running_mean_std_known_answer():
    """the reference's own test for this path (running_mean_std.py:44-62): with epsilon 0 the statistics after two updates
    equal np.mean / np.std of the concatenation (sizes and moments as in the reference test)."""
    import metrpo_amd
    from metrpo_amd.dynamics_training import RunningMeanStd
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 2, (64, 64), (32, 32), seed=75)
    rng = np.random.RandomState(5)
    x = (rng.randn(1000, 3) * 1.0 + 2.0).astype(np.float32); y = (rng.randn(1000, 3) * 3.0 + 1.0).astype(np.float32)
    z = np.concatenate([x, y], axis=0).astype(np.float64)
    rms = RunningMeanStd(eng, epsilon=0.0, shape=[3])
    rms.update(x); rms.update(y)
    assert np.allclose(cpu(rms.mean), z.mean(0)) and np.allclose(cpu(rms.std), z.std(0))


def test_optimize_models_loop_fits_and_restores_best():
    import metrpo_amd
    from metrpo_amd.dynamics_training import data_collection, optimize_models
    env, K = 'swimmer', 5
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, (64, 64), (32, 32), seed=75)
    true, _, _, _ = O.make_problem(env, K=1, dyn_hidden=(32, 32), pol_hidden=(8, 8), seed=99)
    rng = np.random.RandomState(0)

    def gen(n):
        x = rng.randn(n, dm.ns + dm.na) * 0.5; x[:, dm.ns:] = np.clip(x[:, dm.ns:], -1, 1)
        return x.astype(np.float32), O.dynamics_forward(true, 0, x[:, :dm.ns], x[:, dm.ns:]).astype(np.float32)
    dat, val = data_collection(10 ** 6, device='cuda'), data_collection(10 ** 6, device='cuda')
    dat.add_data(*gen(4000)); val.add_data(*gen(1000))
    before = cpu(eng.eval_losses(val.x, val.y))
    np.random.seed(0)
    out = optimize_models(eng, dat, val, {"scratch": 3e-3, "refine": 1e-3}, batch_size=200, max_passes=40, log_every=1,
                          num_passes_threshold=5, reinitialize=True, init_seed=1)
    after = cpu(eng.eval_losses(val.x, val.y))
    assert (after < 0.2 * before).all() and out['n_model_updates'] > 0
    np.testing.assert_allclose(after, out['min_validation_losses'], rtol=1e-5)      # recover_weights: each model at its own best
    # the refreshed ensemble is what the rollout kernels now use
    traj = eng.rollout(64, 5, 5, 'step_rand', pool, seed=1)
    assert torch.isfinite(traj.obs).all()


def test_dynamics_npz_round_trip(tmp_path):
    """formats.save_dynamics_npz / load_dynamics_npz: weights AND running-normaliser sums under the reference's TF variable names
    (model_based_rl.py:728 checkpoint payload); restoring into a FRESH engine reproduces the predictions."""
    import metrpo_amd
    from metrpo_amd import formats
    from metrpo_amd.dynamics_training import RunningMeanStd, push_normalizers
    eng, dm, theta, pdims, pool = Hh.make_engine('swimmer', 3, (24, 16), (8, 8), seed=77)
    rng = np.random.RandomState(1)
    r_in, r_diff = RunningMeanStd(eng, epsilon=0.0, shape=(12,)), RunningMeanStd(eng, epsilon=0.0, shape=(10,))
    r_in.update((rng.randn(300, 12) * 1.7 + 0.4).astype(np.float32)); r_diff.update((rng.randn(300, 10) * 0.3).astype(np.float32))
    push_normalizers(eng, r_in, r_diff)
    p = str(tmp_path / 'policy-and-models-0.npz')
    formats.save_dynamics_npz(p, eng, r_in, r_diff)
    z = np.load(p)
    assert 'training_dynamics/model0/layer0/weights' in z.files and 'input_rms/runningsum' in z.files and 'diff_rms/count' in z.files
    np.testing.assert_array_equal(z['training_dynamics/model2/layer1/weights'], dm.Ws[1][2].astype(np.float32))
    s, a = pool[:32].astype(np.float32), (rng.rand(32, 2) * 2 - 1).astype(np.float32)
    want = eng.step(s, a, 'one_model', None, None, want_all=True)[3].clone()
    fresh = metrpo_amd.Engine('swimmer', 3, (24, 16), (8, 8))                  # never saw set_dynamics
    f_in, f_diff = RunningMeanStd(fresh, epsilon=0.0, shape=(12,)), RunningMeanStd(fresh, epsilon=0.0, shape=(10,))
    formats.load_dynamics_npz(p, fresh, f_in, f_diff)
    fresh.set_policy(theta)
    assert torch.equal(fresh.get_dynamics(), eng.get_dynamics())
    assert torch.equal(fresh.step(s, a, 'one_model', None, None, want_all=True)[3], want)
    assert torch.equal(f_in._sum, r_in._sum) and f_in._count == r_in._count and torch.equal(f_diff.std, r_diff.std)


def test_reference_own_buffer_tests_on_the_device_collection():
    """utils.test_data_collection / test_combine_data_collection (the reference's own tests of this row) on the GPU-resident buffer."""
    import metrpo_amd
    from metrpo_amd.dynamics_training import data_collection, combine_data_collections
    from test_oracle_dynamics import run_reference_buffer_tests
    run_reference_buffer_tests(lambda m: data_collection(m, device='cuda'), combine_data_collections, to_np=cpu)
