"""CPU tests of tests/disagreement_ref.py, the restatement tests/test_gpu_disagreement.py holds metrpo_ensemble_disagreement to: it is np.std / np.linalg.norm
written out; its float32 mode in the device's order stays inside the GPU test's bounds on every GPU case's inputs (so the bounds can be met by correct fp32
code); and on the offset case the one-pass variance E[x^2] - mean^2 in float32 leaves them (so that case catches that mistake)."""
import numpy as np
import pytest

from oracle import metrpo_oracle as O
import tolerances as TOL
import disagreement_ref as DR


def test_restatement_is_np_std_and_norm():
    dm = DR.problem('half_cheetah')[0]
    obs, actions = DR.inputs('half_cheetah', 33)
    valid = np.arange(33) % 3 != 1
    r = DR.disagreement(dm, 'half_cheetah', obs, actions, valid=valid, rows_per_group=5)
    a = np.clip(actions.astype(np.float64), -1, 1)
    for n in range(33):
        heads = np.stack([O.dynamics_forward(dm, k, obs[n:n + 1].astype(np.float64), a[n:n + 1])[0] for k in range(dm.K)])
        if not valid[n]:
            assert not r['next_all'][:, n].any() and not r['std'][n].any() and r['score'][n] == 0 and r['maxdev'][n] == 0 and r['rew_std'][n] == 0
            continue
        np.testing.assert_allclose(r['next_all'][:, n], heads, rtol=1e-13, atol=0)
        np.testing.assert_allclose(r['mean'][n], heads.mean(axis=0), rtol=1e-13, atol=1e-15)
        sd = np.sqrt(((heads - heads.mean(axis=0)) ** 2).sum(axis=0) / dm.K)                       # ddof = 0
        np.testing.assert_allclose(r['std'][n], sd, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(r['score'][n], np.sqrt((sd ** 2).sum()), rtol=1e-12)
        np.testing.assert_allclose(r['maxdev'][n], max(np.linalg.norm(h - heads.mean(axis=0)) for h in heads), rtol=1e-12)
        rk = np.array([-O.cost_np_vec('half_cheetah', obs[n:n + 1].astype(np.float64), a[n:n + 1], h[None])[0] for h in heads])
        np.testing.assert_allclose(r['rew_std'][n], np.std(rk), rtol=1e-10, atol=1e-15)
    assert r['sums'].shape == (7, 4)
    for g in range(7):
        rows = [n for n in range(5 * g, min(33, 5 * g + 5)) if valid[n]]
        sc = r['score'][rows]
        np.testing.assert_allclose(r['sums'][g], [len(rows), sc.sum(), (sc ** 2).sum(), sc.max()], rtol=1e-14)
    assert (actions > 1).any() and (actions < -1).any()                                            # the clip acts
    # rows_per_group = 0: one group
    one = DR.disagreement(dm, 'half_cheetah', obs, actions, valid=valid)
    assert one['sums'].shape == (1, 4) and one['sums'][0, 0] == valid.sum()


def test_one_head_gives_exact_zeros():
    dm = DR.problem('swimmer_k1')[0]
    obs, actions = DR.inputs('swimmer_k1', 17)
    for mode in ('f64', 'f32'):
        r = DR.disagreement(dm, 'swimmer', obs, actions, mode=mode)
        assert not r['std'].any() and not r['score'].any() and not r['maxdev'].any() and not r['rew_std'].any()


def test_float32_two_pass_stays_inside_the_bounds_on_every_gpu_case():
    worst = {}
    cases = sorted(set((sh, N) for sh, N, _ in DR.FUSED_CASES if N <= 64)) + [(sh, 17) for sh in DR.GENERIC]
    for sh, N in cases:
        env, _, hidden, _ = DR.SHAPES[sh]
        dm = DR.problem(sh)[0]
        obs, actions = DR.inputs(sh, N)
        ref = DR.reference(sh, N)
        got = DR.disagreement(dm, env, obs, actions, mode='f32')
        for k, v in DR.shares(got, ref, TOL.wide_or_step(hidden)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("float32 restatement, worst share of each bound over %d cases: %s" % (len(cases), {k: round(v, 4) for k, v in worst.items()}))
    assert all(v < 1.0 for v in worst.values()), worst


def test_offset_case_catches_the_one_pass_variance():
    dm, obs, actions = DR.offset_problem()
    ref = DR.disagreement(dm, 'swimmer', obs, actions)
    assert np.abs(ref['next_all'][:, :, 0]).min() > 900 and ref['std'][:, 0].max() < 1e-2               # |s'| >> spread
    two = DR.shares(DR.disagreement(dm, 'swimmer', obs, actions, mode='f32'), ref, TOL.STEP)
    one = DR.shares(DR.disagreement(dm, 'swimmer', obs, actions, mode='f32_onepass'), ref, TOL.STEP)
    print("offset case, share of the bounds: two-pass %s, one-pass %s" % ({k: round(v, 4) for k, v in two.items()}, {k: round(v, 2) for k, v in one.items()}))
    assert all(v < 1.0 for v in two.values()), two
    assert one['std'] > 1.0 and one['score'] > 1.0, one
