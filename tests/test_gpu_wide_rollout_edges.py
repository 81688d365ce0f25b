"""The wide-net rollout kernels (rollout_gemm.hip, rollout_resident.hip, mlp_streamk.h, mlp_persist.h, big_prepost.h) in every sub-form the dispatch chooses
between, against float64 at the edges of their own tilings.  The table, the dispatch rules restated and the float64 side are tests/wide_rollout_cases.py (held
to their own promises, and shown to fail a wrong kernel, by tests/test_wide_rollout_cases.py); the comparison is rollout_check._check, the one
tests/test_gpu_rollout_edges.py applies to the 2 x 64 table: every output tensor -- mean, act, rew, next state (last_obs included), obs[0] and the reset rows,
done, tpath, last_ts, last_model -- teacher-forced on the device's observations, values on the rows of tests/tolerances.py (WIDE; STEP for the widths 72 / 96
and the 2 x 32 policy's mean; ACTION), pool rows and integers exactly, and no row excluded.

One test per form, one engine alive at a time.  The form is forced with set_option / set_rollout_variant / set_exclusive and every option is restored in a
finally.  Behind EVERY launch the library's own report -- last_rollout_kernel(), last_rollout_launch(), rollout_note() -- is held to what
wide_rollout_cases.expect derives from the dispatch rules for that launch, field for field, with the CU census of this process (schedulable_cus()) where a
rule reads it.  Resident and persistent forms end with comm_check().  The last test of an
env's group is the identity-dynamics pass of tests/test_gpu_edge_vectors.py through every wide form of that env.

METRPO_TOL_REPORT=<file> also makes this file write <file>.wide_rollout_edges.json: the worst share of every bound per form, the case and launch counts, the
forms run, the launches per reported sub-form and the wall time (profiles/r27_wide_rollout_edges.txt)."""
import json
import os
import time
import numpy as np
import pytest
import torch
from conftest import load_golden
from oracle import metrpo_oracle as O
import helpers as Hh
import rollout_check as CK
import wide_rollout_cases as WC
from test_gpu_edge_vectors import identity_engine

pytestmark = pytest.mark.gpu

_CUR = {}                      # the one live problem with its engine
_STATS = dict(cases=0, launches=0, forms=[], reports={})       # reports: launches per reported sub-form
_SEEN = set()                  # every distinct launch report of the process, as sorted (field, value) pairs
_RAN = []                      # entries that ran
ENV_ORDER = ('swimmer', 'hopper', 'snake', 'half_cheetah', 'ant', 'humanoid')
FIELDS = ('obs', 'act', 'mean', 'rew', 'done', 'tpath', 'last_obs', 'last_ts', 'last_model')
NOTE_WIDTHS = 'are neither the fused kernels\' 64x64 nor multiples of 256'


@pytest.fixture(scope='module', autouse=True)
def _report():
    CK.REPORT.clear()
    t0 = time.time()
    yield
    _CUR.clear()
    path = os.environ.get('METRPO_TOL_REPORT')
    if path:
        shares = {}
        for (form, what), used in sorted(CK.REPORT.items()):
            shares.setdefault(form, {})[what] = used
        json.dump(dict(_STATS, n_forms=len(_STATS['forms']), table_forms=len(WC.FORMS), wall_seconds=time.time() - t0, shares=shares),
                  open(path + '.wide_rollout_edges.json', 'w'), indent=1, sort_keys=True)


def _same(a, b, what):
    for k in FIELDS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                                                           b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]), '%s: %s differs' % (what, k)


def _problem(f):
    key = WC.problem_key(f)
    if _CUR.get('key') != key:
        _CUR.clear()
        p = WC.Problem(*key)
        p.eng = Hh.engine_of(p.env, p.K, p.hidden, p.pol, p.dm, p.th)
        p.n_cu = p.eng.schedulable_cus()
        p.pool_t = torch.tensor(p.pool32, dtype=torch.float32, device=p.eng.device)
        _CUR.update(key=key, p=p)
    return _CUR['p']


def _force(eng, f, opts=()):
    for k, v in dict(f.opts, **dict(opts)).items():
        eng.set_option(k, v)
    eng.set_exclusive(True)
    assert eng.set_rollout_variant(f.variant) == 3, f.name                 # a large net: the step-wise GEMM families, or the resident kernel in front of them


def _restore(eng, f, opts=()):
    for k in dict(f.opts, **dict(opts)):
        eng.set_option(k, None)
    eng.set_rollout_variant(0); eng.set_exclusive(True)


def _hold_report(eng, f, e, what):
    """The library's report of the launch it just enqueued against the expectation `e` of wide_rollout_cases.expect."""
    rep = eng.last_rollout_launch()
    assert eng.last_rollout_kernel() == e['family'] == rep['family'], (what, e['family'], rep, eng.rollout_note())
    for k, v in e.items():
        assert rep[k] == v, (what, k, v, rep)
    assert set(rep) == set(e), (what, rep, e)
    _SEEN.add(tuple(sorted((k, str(v)) for k, v in rep.items())))
    tag = ' '.join('%s=%s' % (k, rep[k]) for k in eng.ROLLOUT_LAUNCH_FIELDS if k == 'family' or rep[k] not in (0, None, 'single', 'producer'))
    _STATS['reports'][tag] = _STATS['reports'].get(tag, 0) + 1
    note = eng.rollout_note()
    if e['family'] == 'gemm-stepwise' and f.variant == 0 and any(h % 256 for h in f.hidden):
        assert NOTE_WIDTHS in note and 'x'.join(map(str, f.hidden)) in note, (what, note)
    else:
        assert note == '', (what, note)


def _run_case(p, f, c, label):
    dr, rad, seed = p.draws(c)
    supplied = None if c.philox else {k: (v.astype(np.float32) if v.dtype == np.float64 else v.astype(np.int32)) for k, v in dr.items()}
    es = WC.expect_chunks(f, c, p.n_cu)
    family = es[0]['family']
    es = iter(es)
    _STATS['cases'] += 1; _STATS['launches'] += len(c.chunks or (0,))
    for k, v in c.opts.items():
        p.eng.set_option(k, v)
    try:
        return CK._device_run(p, c.B, c.T, c.H, c.mode, family, seed, determ=c.determ, supplied=supplied, chunks=c.chunks,
                              launched=lambda eng: _hold_report(eng, f, next(es), label))
    finally:
        for k in c.opts:
            p.eng.set_option(k, None)


def _run_form(f):
    p = _problem(f)
    one_call = {}
    try:
        _force(p.eng, f)
        for i, c in enumerate(WC.cases(f)):
            label = '%s/%s#%d' % (f.name, c.name, i)
            dev = _run_case(p, f, c, label)
            WC.check_case(p, c, dev, label, form=f.name)
            if c.name == 'all-modes':
                one_call[c.mode] = dev
            elif c.name == 'chunked':                                  # t0 / resume / last_state, same family and sub-form (test_wide_rollout_cases.py): field for field the one call
                _same(dev, one_call[c.mode], label + ' against the one call')
        if f.group in ('resident', 'persist'):
            p.eng.comm_check()                                         # no hand-over timed out
    finally:
        _restore(p.eng, f)
    _STATS['forms'].append(f.name)


def _run_identity(env):
    """tests/test_gpu_edge_vectors.py::test_edge_vectors_through_fused_rollouts through every wide form of this env: the reference-held reward rows, and for Ant
    the NaN / +-Inf rows and the exact 0.2 / 1.0 boundaries, through every closing kernel's reward and is_done code.  TWO steps: identity dynamics keep
    next = s, and every env that ends is reset onto its own row again, so both steps see the golden rows -- step 0 closed by what the form closes its inner
    steps with (k_big_post, the merged pre-steps' big_close_step, the persistent launch's closing workgroups, the resident post wave), the last step by
    k_big_post or the resident post wave.  The launch report must name that sub-form (T = 1 would collapse the merged and persistent forms)."""
    _CUR.clear()                                                       # one engine at a time
    rows = load_golden('rewards_' + env)
    ns, na, _ = O.ENV_SPECS[env]
    xn, u, ref_rew = rows['x_next'], rows['u'], -rows['cost']
    ref_done = np.zeros(len(xn), bool)
    if env == 'ant':
        a = load_golden('ant_done')
        n = len(a['x_next'])
        xn = np.concatenate([xn, a['x_next']]); u = np.concatenate([u, np.zeros((n, na))])
        ref_rew = np.concatenate([ref_rew, -O.cost_np_vec('ant', a['x_next'], np.zeros((n, na)), a['x_next'])])
        ref_done = np.concatenate([O.is_done('ant', rows['x_next'], rows['x_next']), a['done']])
        assert not np.isfinite(a['x_next']).all() and (a['x_next'][:, 2] == 0.2).any() and (a['x_next'][:, 2] == 1.0).any()
    B, T = len(xn), 2
    fin = np.isfinite(xn).all(axis=1)      # non-finite states make the policy output NaN: np.clip keeps NaN, fminf/fmaxf do not -- the reward of such a row is meaningless in both
    forms = [f for f in WC.FORMS if f.env == env]
    closers = set()
    for key in sorted({WC.problem_key(f) for f in forms}, key=str):
        eng, _, _ = identity_engine(env, key[1], key[2], key[3])
        for f in forms:
            if WC.problem_key(f) != key:
                continue
            try:
                _force(eng, f)
                traj = eng.rollout(B, T, 1000, 'eps_rand', xn.astype(np.float32), eps=np.stack([u] * T).astype(np.float32),
                                   reset_idx=np.stack([np.arange(B)] * (T + 1)).astype(np.int32), reset_model=np.zeros((T + 1, B), np.int32))
                e = WC.expect(f, B, T, 1000, 'eps_rand', n_cu=eng.schedulable_cus())
                _hold_report(eng, f, e, 'identity/' + f.name)
                closers.add((e['family'], e['pre']))
                _STATS['launches'] += 1
                for t in range(T):
                    np.testing.assert_array_equal(CK.cpu(traj.obs[t])[fin], xn.astype(np.float32).astype(np.float64)[fin], err_msg='%s step %d' % (f.name, t))
                    np.testing.assert_allclose(CK.cpu(traj.rew[t])[fin], ref_rew[fin], rtol=2e-6, atol=2e-6, err_msg='%s step %d' % (f.name, t))
                    assert np.array_equal(CK.cpu(traj.done[t]).astype(bool), ref_done), (f.name, t)
                    np.testing.assert_array_equal(CK.cpu(traj.act[t])[fin], u.astype(np.float32).astype(np.float64)[fin], err_msg='%s step %d' % (f.name, t))
                np.testing.assert_array_equal(CK.cpu(traj.tpath[0]), np.zeros(B), err_msg=f.name)
                np.testing.assert_array_equal(CK.cpu(traj.tpath[1]), np.where(ref_done, 0, 1), err_msg=f.name)
                if f.group in ('resident', 'persist'):
                    eng.comm_check()
            finally:
                _restore(eng, f)
        del eng
    # step 0 of this env's pass went through every closer its forms have
    if env == 'humanoid':
        assert closers >= {('gemm-stepwise', k) for k in ('mfma3', 'mfma3-split', 'mfma3-merged', 'valu', 'gemm-chain')} | {('gemm-streamk', 'mfma3-split')}, closers
    else:
        assert closers >= {('gemm-stepwise', 'mfma'), ('gemm-stepwise', 'mfma-merged'), ('gemm-streamk', 'mfma-merged'), ('streamk-persistent', 'mfma'), ('resident', None)}, closers


ENTRIES = [e for env in ENV_ORDER for e in sorted((f for f in WC.FORMS if f.env == env), key=lambda f: (str(WC.problem_key(f)), WC.FORMS.index(f))) + [env]]
assert len(ENTRIES) == len(WC.FORMS) + len(ENV_ORDER)


@pytest.mark.parametrize('entry', ENTRIES, ids=['identity-vectors-' + e if isinstance(e, str) else e.name for e in ENTRIES])
def test_wide_rollout_form(entry):
    if isinstance(entry, str):
        _run_identity(entry)
    else:
        _run_form(entry)
    _RAN.append(entry)


def test_the_whole_table_ran_and_the_device_reported_every_sub_form():
    """tests/test_wide_rollout_cases.py proves the table's coverage from the rules at the nominal CU count; here the same sets are taken from what the library
    REPORTED on this device (whose CU census moves the resident grid and the closing workgroups), when the whole module ran."""
    if len(_RAN) != len(ENTRIES):
        print('only %d of %d entries ran: nothing to hold' % (len(_RAN), len(ENTRIES)))
        return
    assert sorted(_STATS['forms']) == sorted(f.name for f in WC.FORMS)          # as many forms in the report as in the table
    reps = [dict(r) for r in _SEEN]
    of = lambda fam: [r for r in reps if r['family'] == fam]
    vals = lambda rs, k: {r[k] for r in rs}
    gs, sk, pe, re_ = of('gemm-stepwise'), of('gemm-streamk'), of('streamk-persistent'), of('resident')
    assert vals(gs, 'pre') == {'mfma', 'mfma-merged', 'mfma3', 'mfma3-split', 'mfma3-merged', 'valu', 'gemm-chain'} and vals(gs + sk, 'post_width') == {'32', '64'}
    assert {(r['fuse_tile'], r['out_splits']) for r in gs} >= {('0', '0'), ('0', '2'), ('1', '2'), ('1', '4')}
    assert {(r['sk_mode'], r['late'], r['l0']) for r in sk} >= {('1', '0', 'producer'), ('1', '1', 'producer'), ('2', '0', 'rows'), ('3', '0', 'rows'), ('3', '0', 'gemm'),
                                                                 ('3', '1', 'gemm')}
    assert vals(gs, 'rounds') == vals(sk, 'rounds') == {'single', 'merged', 'parallel'}
    assert vals(pe, 'persist_wide') == {'0', '1'} and all(1 <= int(r['nclose']) <= 8 and r['post_width'] == '0' for r in pe)
    assert {(r['res_ws'], r['res_threads']) for r in re_} == {('16', '512'), ('32', '512'), ('64', '256')}
    assert vals(re_, 'res_rot') == {'0', '1'} and vals(re_, 'rounds') == {'single', 'parallel'}       # the rotating-deal instantiations ran on this device
