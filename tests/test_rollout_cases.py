"""tests/rollout_cases.py held to its own promises, without the library: the table reaches every compiled 2 x 64 rollout instantiation in every form, every
sampling mode meets every tile edge at both K parities, the Ant cases are clear of the done thresholds and mix early and horizon terminations -- and the
check that tests/test_gpu_rollout_edges.py applies to the device fails a wrong kernel: a float64 trajectory with one of rollout_cases.MUTATIONS built in, put
in the device's place, must break the check on at least one case of every pair the mutation applies to, while the unmutated trajectory passes every case."""
import numpy as np
import pytest
from conftest import load_golden
from oracle import metrpo_oracle as O
import rollout_cases as RC
import rollout_check as CK

_PROBLEMS = {}


def _problem(env, K):
    """One problem per pair at a time (its draws are cached on it)."""
    if (env, K) not in _PROBLEMS:
        _PROBLEMS.clear()
        _PROBLEMS[(env, K)] = RC.Problem(env, K)
    return _PROBLEMS[(env, K)]


def _distinct_cases(env, K):
    """The cases of every form of a pair, one per distinct (shape, mode, draws): the forms differ only in the rotation of the modes."""
    seen, out = set(), []
    for form in RC.forms(env, K):
        for c in RC.cases(env, K, form):
            key = (c.B, c.T, c.H, c.mode, c.determ, c.philox)
            if key not in seen:
                seen.add(key); out.append(c)
    return out


def test_the_table_is_the_compiled_table():
    assert len(RC.TABLE) == 47 and len(set(RC.TABLE)) == 47 and len(RC.PAIRS) == 50 and not set(RC.TABLE) & set(RC.OFF_TABLE)
    assert {K for e, K in RC.TABLE if e == 'ant'} == set(range(1, 9)) and {K for e, K in RC.TABLE if e == 'half_cheetah'} == set(range(1, 10))
    for env, K in RC.TABLE:
        f = RC.forms(env, K)
        assert f[0] == 'coop-one' and ('coop-two' in f) == (K <= 5) and ('head-per-wave' in f) == (K <= 8)
        assert ('coop-one-4wave' in f) == (env in ('swimmer', 'hopper', 'snake') and 2 <= K <= 5) == (RC.launch_of(env, K, 'coop-one')[4] == 8)
        assert ('generic' in f) == (K in (1, 5, 10) or K == RC.K_MAX[env])
    for env, K in RC.OFF_TABLE:
        assert RC.forms(env, K)[0] == 'gemm-stepwise' and K > RC.K_MAX[env]
    # 8-wave head-split instantiations: three envs at K = 2 ... 5
    assert sum(RC.launch_of(e, K, 'coop-one')[4] == 8 for e, K in RC.TABLE) == 12


def test_every_form_holds_every_case_class_and_at_most_three_tiles():
    n = 0
    for env, K in RC.PAIRS:
        for form in RC.forms(env, K):
            cs = RC.cases(env, K, form)
            n += len(cs)
            names = [c.name for c in cs]
            assert [c.mode for c in cs if c.name == 'all-modes'] == list(O.SAM_MODES)
            assert sorted((c.B, c.T, c.H) for c in cs if c.name == 'edges') == sorted(RC.EDGES)
            assert sorted((c.B, c.T, c.H) for c in cs if c.name == 'horizon') == sorted(RC.HORIZON)
            assert names.count('chunked') == 1 and names.count('determ') == 1 and names.count('philox') == (1 if form.startswith('coop') else 0)
            assert [c.mode for c in cs if c.name == 'selected-head-only'] == (['step_rand', 'eps_rand', 'one_model'] if form == 'generic' else [])
            for c in cs:
                assert (c.B + 15) // 16 <= 3 and c.mode in O.SAM_MODES and (c.chunks is None or sum(c.chunks) == c.T)
                assert c.eval_all == (c.name != 'selected-head-only') and c.determ == (c.name == 'determ') and c.philox == (c.name == 'philox')
            ch = [c for c in cs if c.name == 'chunked'][0]
            assert (ch.B, ch.T, ch.H) == RC.FULL and ch.chunks[0] == ch.H        # the chunk boundary sits exactly behind the horizon reset
    print('%d cases over %d (pair, form) entries' % (n, sum(len(RC.forms(e, K)) for e, K in RC.PAIRS)))


def test_every_mode_meets_every_tile_edge_at_both_parities_of_K():
    met, horizon, philox, determ = set(), set(), set(), set()
    for env, K in RC.PAIRS:
        for form in RC.forms(env, K):
            for c in RC.cases(env, K, form):
                if c.eval_all and not c.philox and not c.determ and c.chunks is None:
                    met.add((c.mode, c.B, K % 2))
                if c.name == 'horizon':
                    horizon.add((c.mode, c.T, c.H))
                if c.philox:
                    philox.add((c.mode, K % 2))
                if c.determ:
                    determ.add(c.mode)
    assert met >= {(m, B, par) for m in O.SAM_MODES for B in (1, 15, 16, 17, 33) for par in (0, 1)}
    assert horizon == {(m, T, H) for m in O.SAM_MODES for (B, T, H) in RC.HORIZON}
    assert philox == {(m, par) for m in O.SAM_MODES for par in (0, 1)} and determ == set(O.SAM_MODES)
    # the modes that read all heads, on the instantiations nothing held against float64 before: the two-middle-heads median at K = 6, 8, 10
    for K in (6, 8, 10):
        assert any(c.mode == 'model_med' and c.B == B for c in RC.cases('swimmer', K, 'coop-one') for B in (33,))


def test_ant_cases_are_clear_of_the_thresholds_and_mix_both_terminations():
    closest, early, total = np.inf, 0, 0
    for env, K in RC.PAIRS:
        if env != 'ant':
            continue
        p = _problem(env, K)
        for c in _distinct_cases(env, K):
            dr, rad, seed = p.draws(c)
            free = RC.reference(p, dr, c.B, c.T, c.H, c.mode, c.determ)
            z = free['next'][:, :, 2]
            gap = float(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)).min())
            assert gap >= RC.ANT_MARGIN, (K, c, gap)
            closest = min(closest, gap)
            if c.name == 'all-modes':
                e, h = free['done'] & (free['tpath'] < c.H - 1), free['done'] & (free['tpath'] == c.H - 1)
                assert e.any() and h.any(), (K, c.mode, int(e.sum()), int(h.sum()))
                assert (free['last_ts'] != 0).any()                                 # the call ends mid-path
                early += int(e.sum()); total += int(free['done'].sum())
    print('closest z to a threshold %.3g; %d of %d dones of the all-modes cases are early' % (closest, early, total))


def test_ant_bound_mutation_shows_on_the_identity_vectors():
    """The rollout cases stay clear of 0.2 / 1.0 by construction; the exact boundaries go through every K's epilogue in the identity pass (ant_done.npz)."""
    d = load_golden('ant_done')
    xn = d['x_next']
    assert np.array_equal(~RC.ant_not_done(xn), d['done'])
    assert not np.array_equal(~RC.ant_not_done(xn, 'ant_bound_gt'), d['done'])
    assert ((xn[:, 2] == 0.2) & ~d['done']).any() and ((xn[:, 2] == 1.0) & ~d['done']).any()
    # the fixture's boundary values are fp32 numbers' neighbours too: rounding to the device's storage type keeps them on their side
    assert np.array_equal(~RC.ant_not_done(xn.astype(np.float32)), d['done'])


def _passes(p, c, dev, form=None):
    try:
        RC.check_case(p, c, dev, 'cpu', form=form)
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize('env,K', RC.PAIRS, ids=['%s-K%d' % pk for pk in RC.PAIRS])
def test_check_passes_the_reference_and_fails_every_mutation(env, K):
    p = _problem(env, K)
    cs = _distinct_cases(env, K)
    CK.REPORT.clear()
    for c in cs:                                                       # two float64 restatements (reference(), helpers.oracle_rollout) agree on every case
        dr, rad, seed = p.draws(c)
        RC.check_case(p, c, RC.reference(p, dr, c.B, c.T, c.H, c.mode, c.determ), 'float64 %s' % c.name, form='cpu')
    assert max(CK.REPORT.values()) < 1e-6, CK.REPORT                   # ... to float64 rounding: 1e-6 of the fp32 bounds
    CK.REPORT.clear()
    for mut in RC.MUTATIONS:
        if not RC.mutation_applies(mut, env, K):
            continue
        caught = [c for c in cs if not _passes(p, c, RC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ, mut=mut))]
        print('%s: caught by %d of %d cases' % (mut, len(caught), len(cs)))
        assert caught, mut
        if mut in ('upper_median', 'std_ddof1'):                       # value faults: it is the tolerance row itself that they exceed, and by what factor
            worst = 0.0
            for c in caught:
                ok, bad = (RC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ, mut=m)['next'][0] for m in (None, mut))   # step 0: same state
                worst = max(worst, float((np.abs(bad - ok) / (p.tol['atol'] + p.tol['rtol'] * np.abs(ok))).max()))
            print('    %s exceeds STEP on the next state by %.3g x' % (mut, worst))
            assert worst > 1.0, (mut, worst)
        # not by one lucky case class: the tile-edge cases see it too wherever they can
        if mut in ('tpath_off_by_one', 'reset_row_t'):
            assert {'edges', 'horizon', 'all-modes'} <= {c.name for c in caught}, (mut, {c.name for c in caught})
