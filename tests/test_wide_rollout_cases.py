"""tests/wide_rollout_cases.py held to its own promises, without the library: the table reaches every instantiation of the wide-net rollout paths it names (by the
dispatch rules restated in wide_rollout_cases.expect), every sampling mode meets every B edge, every family sees K = 1, an even K under model_med and K >= 3
under model_mean_std, chunks take the sub-form of the one call, the Ant cases are clear of the done thresholds and mix early and horizon terminations, no Philox
radius is small enough to be excluded -- and the check that tests/test_gpu_wide_rollout_edges.py applies to the device fails a wrong kernel: a float64 trajectory
with one of wide_rollout_cases.MUTATIONS built in, put in the device's place, must break the check on at least one case of every form the mutation applies to,
while the unmutated trajectory passes every case to 1e-6 of the bounds."""
import numpy as np
import pytest
from oracle import metrpo_oracle as O
import rollout_check as CK
import wide_rollout_cases as WC

_PROBLEMS = {}
KEYS = sorted({WC.problem_key(f) for f in WC.FORMS}, key=str)
FIVE = ('swimmer', 'half_cheetah', 'hopper', 'snake', 'ant')


def _problem(key):
    """One problem at a time (its draws are cached on it)."""
    if key not in _PROBLEMS:
        _PROBLEMS.clear()
        _PROBLEMS[key] = WC.Problem(*key)
    return _PROBLEMS[key]


def _ckey(c):
    return (c.B, c.T, c.H, c.mode, c.determ, c.philox)


def _launches():
    """(form, case, expectation of each of its launches) over the table."""
    for f in WC.FORMS:
        for c in WC.cases(f):
            yield f, c, WC.expect_chunks(f, c)


def test_every_named_instantiation_is_reached():
    seen = dict(pre=set(), post=set(), sk1=set(), sk_modes=set(), mode3_l0=set(), late=set(), place=set(), persist=set(), resident=set(), tile=set(), rounds=set(), rot=set())
    S0 = lambda env: (sum(O.ENV_SPECS[env][:2]) - O.ENV_SPECS[env][2] + 1 + 3) // 4
    OT = lambda env: 1 if O.ENV_SPECS[env][0] <= 16 else 2 if O.ENV_SPECS[env][0] <= 32 else 4
    for f, c, es in _launches():
        for e in es:
            if e['family'] == 'resident':
                seen['resident'].add((f.env, f.hidden[0], e['res_ws'], e['res_threads']))
                if e['res_rot']:
                    seen['rot'].add(f.env)
                assert e['pre'] is None and e['post_width'] == 0
                continue
            seen['pre'].add((e['pre'], f.env) if e['pre'] in ('mfma', 'mfma-merged') else e['pre'])
            seen['post'].add(e['post_width'])
            seen['rounds'].add((e['family'], e['rounds']))
            if e['family'] == 'gemm-stepwise':
                seen['tile'].add((f.hidden, e['fuse_tile'], e['out_splits']))
            if e['family'] == 'gemm-streamk':
                seen['sk_modes'].add(e['sk_mode'])
                if e['sk_mode'] == 1:
                    seen['sk1'].add((S0(f.env), OT(f.env)))
                if e['sk_mode'] == 3:
                    seen['mode3_l0'].add(e['l0'])
                if f.hidden == (1024, 1024):
                    seen['late'].add((OT(f.env), e['late']))
                if 'STREAMK_PLACE' in f.opts:
                    seen['place'].add(f.opts['STREAMK_PLACE'])
            if e['family'] == 'streamk-persistent':
                seen['persist'].add((f.env, S0(f.env), OT(f.env), e['persist_wide']))
                assert e['post_width'] == 0 and e['pre'] == 'mfma' and e['l0'] == 'producer'
    assert seen['pre'] >= {(k, env) for k in ('mfma', 'mfma-merged') for env in FIVE} | {'mfma3', 'mfma3-split', 'mfma3-merged', 'valu', 'gemm-chain'}, seen['pre']
    assert seen['post'] == {0, 32, 64}
    assert seen['tile'] >= {((96, 96), 0, 0), ((256, 256), 1, 4), ((256, 256), 0, 2), ((128, 128, 128), 1, 2), ((72, 72), 0, 0)}, seen['tile']
    assert seen['sk_modes'] == {1, 2, 3} and seen['sk1'] == {(3, 1), (4, 1), (5, 1), (6, 2), (9, 2)} and seen['mode3_l0'] == {'rows', 'gemm'}
    assert seen['late'] == {(ot, late) for ot in (1, 2, 4) for late in (0, 1)} and seen['place'] == {'flat', 'xcd'}
    assert seen['persist'] == {(env, S0(env), OT(env), w) for env in FIVE for w in (0, 1)}
    assert seen['resident'] == {('swimmer', 512, 16, 512), ('swimmer', 512, 32, 512), ('hopper', 512, 32, 512), ('snake', 512, 32, 512), ('half_cheetah', 512, 32, 512),
                                ('hopper', 1024, 64, 256), ('snake', 1024, 64, 256), ('half_cheetah', 1024, 64, 256), ('swimmer', 1024, 64, 256), ('ant', 1024, 64, 256)}
    assert seen['rot'] == set(FIVE)                                    # k_rollout_resident_wide<ENV, 1024, 64, true>
    assert seen['rounds'] >= {(fam, r) for fam in ('gemm-stepwise', 'gemm-streamk') for r in ('single', 'merged', 'parallel')}


def test_every_form_runs_its_family_and_chunks_keep_the_sub_form():
    n = 0
    for f in WC.FORMS:
        cs = WC.cases(f)
        n += len(cs)
        names = [c.name for c in cs]
        B, T, H = WC.full_shape(f)
        assert [c.mode for c in cs if c.name == 'all-modes'] == list(O.SAM_MODES) and all((c.B, c.T, c.H) == (B, T, H) for c in cs if c.name in ('all-modes', 'chunked'))
        assert sorted(c.B for c in cs if c.name == 'edges') == sorted(WC.edge_batches(f)) and all((c.T, c.H) == (6, 4) for c in cs if c.name == 'edges')
        assert sorted((c.B, c.T, c.H) for c in cs if c.name == 'horizon') == sorted(WC.HORIZON)
        assert names.count('chunked') == names.count('determ') == names.count('philox') == 1
        assert names.count('philox-rounds') == (2 if f.env != 'ant' and f.group in ('gemm', 'streamk') else 0)
        assert all(c.B <= 129 and c.T <= 8 and f.K <= 5 and f.K in (1, 2, 3, 5) for c in cs) and (not WC.is_1024(f) or all(c.B <= 33 or c.name == 'rotating' for c in cs))
        fam = WC.FAMILY_OF_GROUP[f.group]
        hit = 0
        for c in cs:
            es = WC.expect_chunks(f, c)
            if c.chunks:                                               # same family, same sub-form as the one call: the chunked result must be bitwise the one call's
                one = WC.expect(f, c.B, c.T, c.H, c.mode, c.philox, c.opts)
                assert all(e == one for e in es), (f.name, es, one)
            hit += all(e['family'] == fam for e in es)
            if f.group == 'resident':
                assert {e['family'] for e in es} == ({'resident'} if c.mode in WC.RESIDENT_MODES and c.B <= 128 else {'gemm-stepwise'}), (f.name, c)
            elif f.group == 'persist':
                assert {e['family'] for e in es} == ({'streamk-persistent'} if c.T >= 2 and c.name != 'philox-rounds' else {'gemm-streamk'}), (f.name, c)
            else:
                assert {e['family'] for e in es} == {fam}, (f.name, c)
            if c.name == 'philox-rounds':
                assert [e['rounds'] for e in es] == ['parallel' if 'NO_MERGED_ROUNDS' in c.opts else 'merged']
        assert hit >= 10, (f.name, hit)
        if f.group == 'resident':                                  # the resident kernel itself meets every edge (B <= 128) and, where B <= 128 on the full shape, all its modes
            assert {c.B for c in cs if c.name == 'edges' and c.mode in WC.RESIDENT_MODES} == set(WC.edge_batches(f))
            full = [c for c in cs if c.name in ('all-modes', 'resident-modes') and c.B <= 128]
            assert {c.mode for c in full if WC.expect_chunks(f, c)[0]['family'] == 'resident'} == set(WC.RESIDENT_MODES)
            other = [c for c in cs if c.name == 'all-modes' and c.mode not in WC.RESIDENT_MODES]
            assert len(other) == 3 and all(WC.expect_chunks(f, c)[0]['family'] == 'gemm-stepwise' for c in other)
    print('%d cases over %d forms, %d distinct problems' % (n, len(WC.FORMS), len(KEYS)))


def test_every_mode_meets_every_edge_and_every_family_its_K():
    met, k1, med_even, std3 = set(), set(), set(), set()
    for f, c, es in _launches():
        fam = es[0]['family']
        if not c.philox and not c.determ and c.chunks is None:
            met.add((c.mode, c.B))
        if f.K == 1:
            k1.add(fam)
        if f.K % 2 == 0 and c.mode == 'model_med':
            med_even.add(fam)
        if f.K >= 3 and c.mode == 'model_mean_std':
            std3.add(fam)
    assert met >= {(m, B) for m in O.SAM_MODES for B in (1, 15, 16, 17, 33, 63, 64, 65, 127, 128, 129)}
    fams = {'gemm-stepwise', 'gemm-streamk', 'streamk-persistent', 'resident'}
    assert k1 == fams, k1
    assert med_even == std3 == fams - {'resident'}                     # (the resident kernel takes step_rand, eps_rand and one_model only)


def test_ant_cases_are_clear_of_the_thresholds_and_mix_both_terminations():
    closest, early, total = np.inf, 0, 0
    for f in WC.FORMS:
        if f.env != 'ant':
            continue
        p = _problem(WC.problem_key(f))
        for c in WC.cases(f):
            dr, rad, seed = p.draws(c)
            free = WC.reference(p, dr, c.B, c.T, c.H, c.mode, c.determ)
            z = free['next'][:, :, 2]
            gap = float(np.minimum(np.abs(z - 0.2), np.abs(z - 1.0)).min())
            assert gap >= WC.RC.ANT_MARGIN, (f.name, c, gap)
            closest = min(closest, gap)
            if c.name == 'all-modes':
                e, h = free['done'] & (free['tpath'] < c.H - 1), free['done'] & (free['tpath'] == c.H - 1)
                assert e.any() and h.any(), (f.name, c.mode, int(e.sum()), int(h.sum()))
                assert (free['last_ts'] != 0).any()                                 # the call ends mid-path
                early += int(e.sum()); total += int(free['done'].sum())
    print('closest z to a threshold %.3g; %d of %d dones of the all-modes cases are early' % (closest, early, total))


def _passes(p, c, dev):
    try:
        WC.check_case(p, c, dev, 'cpu')
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize('key', KEYS, ids=['%s-K%d-%s-%s' % (k[0], k[1], 'x'.join(map(str, k[2])), 'x'.join(map(str, k[3]))) for k in KEYS])
def test_check_passes_the_reference_and_fails_every_mutation(key):
    p = _problem(key)
    forms = [f for f in WC.FORMS if WC.problem_key(f) == key]
    distinct = {}
    for f in forms:
        for c in WC.cases(f):
            distinct.setdefault(_ckey(c), c)
    # ---- no Philox normal is excluded; two float64 restatements (reference(), helpers.oracle_rollout behind _check) agree on every distinct case
    CK.REPORT.clear()
    for c in distinct.values():
        dr, rad, seed = p.draws(c)
        if c.philox:
            assert min(rad['eps'].min(), rad['sel_noise'].min()) >= CK.SMALL_R
        WC.check_case(p, c, WC.reference(p, dr, c.B, c.T, c.H, c.mode, c.determ), 'float64 %s' % c.name, form='cpu')
    assert max(CK.REPORT.values()) < 1e-6, CK.REPORT                   # ... to float64 rounding: 1e-6 of the fp32 bounds
    CK.REPORT.clear()
    verdict = {}                                                       # (mutation, case key) -> caught

    def caught_by(mut, c):
        k = (mut, _ckey(c))
        if k not in verdict:
            verdict[k] = not _passes(p, c, WC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ, mut=mut))
        return verdict[k]
    for f in forms:
        cs = WC.cases(f)
        for mut in WC.MUTATIONS:
            if not WC.mutation_applies(mut, f):
                continue
            # not by one lucky case class: the tile-edge cases must see these two themselves
            pick = [c for c in cs if c.name == 'edges'] if mut in ('row_block_tail', 'tpath_off_by_one') else sorted(cs, key=lambda c: -c.B)
            first = next((c for c in pick if caught_by(mut, c)), None)
            assert first is not None, (f.name, mut)
            if mut in WC.VALUE_MUTATIONS:                              # value faults: it is the tolerance row itself that they exceed, and by what factor
                ok, bad = (WC.reference(p, p.draws(first)[0], first.B, first.T, first.H, first.mode, first.determ, mut=m)['next'][0] for m in (None, mut))   # step 0: same state
                factor = float((np.abs(bad - ok) / (p.tol['atol'] + p.tol['rtol'] * np.abs(ok))).max())
                print('%s: %s exceeds the state row on the next state by %.3g x (%s B %d %s)' % (f.name, mut, factor, first.name, first.B, first.mode))
                assert factor > 1.0, (f.name, mut, factor)
