"""tests/process_ref.py (the float64 time-major restatement the GPU process kernels are held to) against the oracle's per-path
process_samples and LinearFeatureBaselineOracle on small ragged batches, every done pattern; and the oracle's lstsq cut-off.  CPU only."""
import numpy as np
import pytest
from oracle import metrpo_oracle as O
import helpers as Hh
import process_ref as R


def _batch(pattern, T, B, ns, seed, rscale=1.0):
    rng = np.random.RandomState(seed)
    done, tpath = R.make_done(pattern, T, B, rng, nw=4)
    obs = (rng.randn(T, B, ns) * 4.0).astype(np.float32)                  # some entries beyond the +-10 clip
    rew = (rng.randn(T, B) * rscale).astype(np.float32)
    return obs, rew, done, tpath


@pytest.mark.parametrize('pattern', R.DONE_PATTERNS)
@pytest.mark.parametrize('gamma,lam', [(1.0, 1.0), (0.99, 0.95), (0.995, 1.0), (0.9, 0.0)])
@pytest.mark.parametrize('use_coeffs', [False, True])
def test_gae_matches_oracle_process_samples(pattern, gamma, lam, use_coeffs):
    T, B, ns = 23, 7, 5
    obs, rew, done, tpath = _batch(pattern, T, B, ns, seed=R.DONE_PATTERNS.index(pattern) * 10 + int(lam * 7), rscale=1e3 if lam == 0.0 else 1.0)
    coeffs = np.random.RandomState(3).randn(2 * ns + 4) * 0.3 if use_coeffs else None
    V = R.baseline_values(obs, tpath, coeffs) if use_coeffs else None
    adv, ret, valid = R.gae(rew, done, gamma, lam, V)
    tr = dict(obs=obs.astype(np.float64), act=np.zeros((T, B, 1)), rew=rew.astype(np.float64), mean=np.zeros((T, B, 1)),
              done=done.astype(bool), tpath=tpath)
    paths = Hh.paths_from_timemajor(tr)
    tb = [x for p in paths for x in p['_tb']]
    assert int(valid.sum()) == len(tb)
    if not tb:                                                             # 'none': nothing completes, nothing is valid
        assert pattern == 'none' and not valid.any()
        np.testing.assert_array_equal(R.stats(adv, valid), [0.0, 0.0, 0.0])
        return
    tt, bb = np.array(tb).T
    assert valid[tt, bb].all()
    base = O.LinearFeatureBaselineOracle(); base._coeffs = coeffs
    samples = O.process_samples(paths, base, gamma, lam, center_adv=False)
    a = samples['advantages']
    np.testing.assert_allclose(adv[tt, bb], a, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(a).max()))
    np.testing.assert_allclose(ret[tt, bb], samples['returns'], rtol=1e-12, atol=1e-12 * max(1.0, np.abs(samples['returns']).max()))
    st = R.stats(adv, valid)
    assert st[2] == len(a)
    np.testing.assert_allclose(st[:2], [a.sum(), (a * a).sum()], rtol=1e-12, atol=1e-12 * np.abs(a).sum())
    np.testing.assert_allclose(R.center(adv, valid)[tt, bb], O.center_advantages(a), rtol=1e-12, atol=1e-12)
    assert (R.center(adv, valid)[~valid] == 0).all()
    # the refit (samplers/base.py:164-167) sees the same normal equations
    F = np.concatenate([O.LinearFeatureBaselineOracle.features(p) for p in paths])
    AtA, Aty = R.normal_equations(obs, ret.astype(np.float32), tpath, valid, chunk=17)
    Fr = R.features(obs, tpath)[tt, bb]
    np.testing.assert_allclose(Fr, F, rtol=1e-15, atol=0)
    np.testing.assert_allclose(AtA, F.T @ F, rtol=1e-12, atol=1e-12 * np.abs(F.T @ F).max())
    np.testing.assert_allclose(Aty, F.T @ ret.astype(np.float32)[tt, bb].astype(np.float64), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('T,B,t0,batch', [(12, 5, 0, 20), (12, 5, 30, 1e9), (9, 4, 3, 0)])
def test_stop_step_is_the_sampler_loop_condition(T, B, t0, batch):
    """obtain_samples (vectorized_sampler.py:60,104): n_samples grows by the length of every path completed at a step, the loop ends
    after the first step at which n_samples >= batch_size -- restated as a Python loop over steps and envs."""
    done, tpath = R.make_done('t0', T, B, np.random.RandomState(T + B))
    n, stop = 0, None
    for t in range(T):
        for b in range(B):
            if done[t, b]:
                n += int(tpath[t, b]) + 1
        if n >= batch:
            stop = t0 + t
            break
    cum, s = R.stop_step(done, tpath, t0, batch)
    assert s == stop and cum == n


def _rank_deficient_paths(seed=11, n_paths=40, L=60, ns=6):
    """Paths whose feature matrix has an exact null space: a saturated observation column (o_1 = 0.75 and o_1^2 = 0.5625 are multiples
    of the constant feature), as every clipped, saturated state dimension gives."""
    rng = np.random.RandomState(seed)
    paths = []
    for _ in range(n_paths):
        o = np.clip(rng.randn(L, ns) * 2.0, -10, 10)
        o[:, 1] = 0.75
        r = rng.randn(L) + o[:, 0]
        paths.append(dict(observations=o, rewards=r, returns=O.discount_cumsum(r, 0.99)))
    return paths


def test_oracle_lstsq_cutoff_is_numpy_1_12s():
    """The reference ran NumPy 1.12.1, whose lstsq default is rcond = -1 (singular values below eps * s_max are cut); rcond=None (NumPy
    >= 1.14's new default) cuts below eps * max(M, N) * s_max.  With reg_coeff at 3e-15 of the largest eigenvalue of F^T F, the regularised
    system's s_min / s_max is ~3e-15: between the two cut-offs.  The old default keeps that direction, the new one drops it -- the
    oracle's fit (and the host solve of me-trpo_amd/baseline.py) must keep it, as the reference did and as the device's elimination does."""
    import metrpo_amd.baseline as MB
    paths = _rank_deficient_paths()
    Fm = np.concatenate([O.LinearFeatureBaselineOracle.features(p) for p in paths])
    y = np.concatenate([p['returns'] for p in paths])
    G = Fm.T @ Fm
    reg = 3e-15 * np.linalg.eigvalsh(G).max()
    A, b = G + reg * np.identity(G.shape[0]), Fm.T @ y
    s = np.linalg.svd(A, compute_uv=False)
    F = A.shape[0]
    assert np.finfo(float).eps < s[-1] / s[0] < np.finfo(float).eps * F                 # between the -1 and the None cut-offs
    keep = np.linalg.lstsq(A, b, rcond=-1)[0]
    drop = np.linalg.lstsq(A, b, rcond=None)[0]
    assert np.linalg.norm(keep - drop) > 1e-5 * np.linalg.norm(drop)                    # the two cut-offs give different coefficients (~4e-4 here)
    base = O.LinearFeatureBaselineOracle(reg_coeff=reg)
    base.fit(paths)
    np.testing.assert_array_equal(base._coeffs, keep)
    host = MB.LinearFeatureBaseline(reg_coeff=reg)
    np.testing.assert_array_equal(host.solve(G, b), keep)
