"""Every compiled 2 x 64 rollout instantiation against float64 at the tile edges.  The table and the float64 side are tests/rollout_cases.py (held to their own
promises, and shown to fail a wrong kernel, by tests/test_rollout_cases.py); the comparison is rollout_check._check, the one tests/test_gpu_rollout_draws.py
applies to the production draws: every output tensor -- mean, act, rew, next state (last_obs included), obs[0] and the reset rows, done, tpath, last_ts,
last_model -- teacher-forced on the device's observations, values on the rows STEP / ACTION / REWARD of tests/tolerances.py, pool rows and integers exactly,
and no row excluded: the Ant cases are drawn clear of the done thresholds, so done / tpath equal the free-running oracle's on every row.

One test per (env, K, form): the 47 (env, K) entries of the cooperative kernel's table in every form they have (one workgroup per CU as the rule launches it,
its 4-wave form where that has 8 waves, two workgroups per CU, head-per-wave, generic) and the three off-table pairs on the step-wise tile GEMMs, each form
asserted from the library's own launch report.  One engine per (env, K) is alive at a time; the forms are switched on it.  The last test of a pair is the
identity-dynamics pass of tests/test_gpu_edge_vectors.py through every form of the pair: the reference-held reward rows, and for Ant the NaN / +-Inf rows and
the exact 0.2 / 1.0 boundaries, through every K's reward and is_done epilogue.

METRPO_TOL_REPORT=<file> (conftest.py) also makes this file write <file>.rollout_edges.json: the worst share of every bound per form, the case count, the wall
time and whether the generic kernel's eval_all_heads = 0 branch was bitwise its all-heads result (profiles/r20_rollout_edges.txt)."""
import json
import os
import time
import numpy as np
import pytest
import torch
from conftest import load_golden
from oracle import metrpo_oracle as O
import helpers as Hh
import rollout_cases as RC
import rollout_check as CK
from test_gpu_edge_vectors import identity_engine

pytestmark = pytest.mark.gpu

_CUR = {}                      # the one live (env, K): its problem with the engine, the one-call results of the all-modes cases per form
_STATS = dict(cases=0, launches=0, selected_head_only_bitwise=True, selected_head_only_cases=0)
FIELDS = ('obs', 'act', 'mean', 'rew', 'done', 'tpath', 'last_obs', 'last_ts', 'last_model')


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
        json.dump(dict(_STATS, wall_seconds=time.time() - t0, shares=shares), open(path + '.rollout_edges.json', 'w'), indent=1, sort_keys=True)


def _attach(p):
    p.eng = Hh.engine_of(p.env, p.K, p.hidden, (32, 32), p.dm, p.th)
    p.pool_t = torch.tensor(p.pool32, dtype=torch.float32, device=p.eng.device)
    return p


def _problem(env, K):
    if _CUR.get('key') != (env, K):
        _CUR.clear()
        _CUR.update(key=(env, K), p=_attach(RC.Problem(env, K)))
    return _CUR['p']


def _select(eng, env, K, form):
    """Force `form` on the engine -> (kernel the dispatch must report, force_generic, assertion on the launch report behind every launch)."""
    variant, split, generic, kernel, waves = RC.launch_of(env, K, form)
    running = eng.set_rollout_variant(variant)
    eng.set_coop_split(split)
    if form != 'generic':
        assert running == dict(zip(('mfma-cooperative', 'mfma-head-per-wave', 'gemm-stepwise'), (2, 1, 3)))[kernel], (form, running)

    def launched(e):
        if generic:
            return
        assert e.last_rollout_kernel() == kernel, (form, e.last_rollout_kernel(), e.rollout_note())
        if kernel == 'mfma-cooperative':
            assert e.last_coop_waves() == waves and e.rollout_note() == '', (form, e.last_coop_waves(), e.rollout_note())
        if kernel == 'gemm-stepwise':
            assert 'beyond the fused kernels' in e.rollout_note() and 'cooperative: K <= 10, half-cheetah 9, Ant 8' in e.rollout_note(), e.rollout_note()
    return kernel, generic, launched


def _run_case(p, c, kernel, generic, launched):
    dr, rad, seed = p.draws(c)
    supplied = None if c.philox else {k: (v.astype(np.float32) if v.dtype == np.float64 else v.astype(np.int32)) for k, v in dr.items()}
    _STATS['cases'] += 1; _STATS['launches'] += len(c.chunks or (0,))
    return CK._device_run(p, c.B, c.T, c.H, c.mode, kernel, seed, determ=c.determ, force_generic=generic, supplied=supplied, chunks=c.chunks,
                          eval_all_heads=c.eval_all, launched=launched)


def _same(a, b, what):
    for k in FIELDS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                                                           b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]), '%s: %s differs' % (what, k)


def _run_form(env, K, form):
    p = _problem(env, K)
    kernel, generic, launched = _select(p.eng, env, K, form)
    one_call = {}
    try:
        for i, c in enumerate(RC.cases(env, K, form)):
            label = '%s/K%d/%s/%s#%d' % (env, K, form, c.name, i)
            dev = _run_case(p, c, kernel, generic, launched)
            RC.check_case(p, c, dev, label, form=form)
            if c.name == 'all-modes':
                one_call[c.mode] = dev
            elif c.name == 'chunked':                                  # t0 / resume / last_state: field for field the one-call result
                _same(dev, one_call[c.mode], label + ' against the one call')
            elif c.name == 'selected-head-only':                       # held to float64 above; whether it is also bitwise the all-heads result is reported
                _STATS['selected_head_only_cases'] += 1
                try:
                    _same(dev, one_call[c.mode], label)
                except AssertionError as e:
                    _STATS['selected_head_only_bitwise'] = False
                    print('    eval_all_heads = 0 is not bitwise the all-heads result: %s' % e)
    finally:
        p.eng.set_rollout_variant(0); p.eng.set_coop_split(True)


def _run_identity(env, K):
    """tests/test_gpu_edge_vectors.py::test_edge_vectors_through_fused_rollouts, through every form of this pair (there: K = 5 only)."""
    _CUR.clear()                                                       # one engine per (env, K) at a time
    eng, ns, na = identity_engine(env, K, (64, 64))
    rows = load_golden('rewards_' + env)
    xn, u, ref_rew = rows['x_next'], rows['u'], -rows['cost']
    ref_done = np.zeros(len(xn), bool)
    if env == 'ant':
        a = load_golden('ant_done')
        n = len(a['x_next'])
        xn = np.concatenate([xn, a['x_next']]); u = np.concatenate([u, np.zeros((n, na))])
        ref_rew = np.concatenate([ref_rew, -O.cost_np_vec('ant', a['x_next'], np.zeros((n, na)), a['x_next'])])
        ref_done = np.concatenate([O.is_done('ant', rows['x_next'], rows['x_next']), a['done']])
        assert not np.isfinite(a['x_next']).all() and (a['x_next'][:, 2] == 0.2).any() and (a['x_next'][:, 2] == 1.0).any()
    B = len(xn)
    assert B <= 16 * 64                                                # far fewer tiles than CUs: no migrating schedule
    fin = np.isfinite(xn).all(axis=1)      # non-finite states make the policy output NaN: np.clip keeps NaN, fminf/fmaxf do not -- the reward of such a row is meaningless in both
    for form in RC.forms(env, K):
        kernel, generic, launched = _select(eng, env, K, form)
        traj = eng.rollout(B, 1, 1000, 'eps_rand', xn.astype(np.float32), eps=u[None].astype(np.float32),
                           reset_idx=np.stack([np.arange(B), np.zeros(B)]).astype(np.int32), reset_model=np.zeros((2, B), np.int32), force_generic=generic)
        launched(eng)
        _STATS['launches'] += 1
        np.testing.assert_allclose(CK.cpu(traj.rew[0])[fin], ref_rew[fin], rtol=2e-6, atol=2e-6, err_msg=form)
        assert np.array_equal(CK.cpu(traj.done[0]).astype(bool), ref_done), form
        np.testing.assert_array_equal(CK.cpu(traj.act[0])[fin], u.astype(np.float32).astype(np.float64)[fin], err_msg=form)
        np.testing.assert_array_equal(CK.cpu(traj.tpath[0]), np.zeros(B), err_msg=form)


ENTRIES = [(env, K, form) for env, K in RC.PAIRS for form in RC.forms(env, K) + ['identity-vectors']]


@pytest.mark.parametrize('env,K,form', ENTRIES, ids=['%s-K%d-%s' % e for e in ENTRIES])
def test_rollout_instantiation(env, K, form):
    if form == 'identity-vectors':
        _run_identity(env, K)
    else:
        _run_form(env, K, form)


@pytest.mark.parametrize('env,K,hidden', RC.NARROW, ids=['%s-K%d-%dx%d' % (e, K, h[0], h[1]) for e, K, h in RC.NARROW])
def test_zero_padded_narrow_nets(env, K, hidden):
    """Hidden widths below 64 run the same cooperative instantiation on a zero-padded copy of the weights: K = 10 swimmer and K = 8 Ant, the largest of
    their envs, at one full tile + one lane, every sampling mode."""
    _CUR.clear()
    p = _attach(RC.Problem(env, K, hidden))
    assert p.eng.set_rollout_variant(0) == 2

    def launched(e):
        assert e.last_rollout_kernel() == 'mfma-cooperative' and e.rollout_note() == '' and e.last_coop_waves() == 4, (e.last_rollout_kernel(), e.rollout_note())
    for m in O.SAM_MODES:
        c = RC.Case('narrow', 17, 6, 4, m, False, None, False, True, False)
        dev = _run_case(p, c, 'mfma-cooperative', False, launched)
        RC.check_case(p, c, dev, '%s/K%d/%dx%d/%s' % (env, K, hidden[0], hidden[1], m), form='coop-padded')
