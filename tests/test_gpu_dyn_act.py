"""Tanh and identity dynamics layers on every entry point that reads the ensemble, against float64.  The table and the float64 side are
tests/dyn_act_cases.py (held to their own promises, and shown to fail a net with the wrong activation, by tests/test_dyn_act_cases.py).

Every fused family is written for relu; a net with another hidden activation must run on the fallbacks and must SAY so.  Each test asserts the family from
the library's own report (last_rollout_kernel / rollout_note / last_rollout_launch, the sweep path set_det_path selects, last_svg_path, the last_*_kernel of
the supplied-action calls) and holds the result to the rows of tests/tolerances.py that a relu net of the same width is held to; no new bound.

  metrpo_rollout     f32, draws supplied, teacher-forced (rollout_check._check): thread-per-env, the tile GEMMs at shapes that are cooperative / stream-K /
                     resident / zero-padded with relu, the split-K reduce with act != 0, the fused output tile only behind a relu layer; bf16 operands
  metrpo_step        all sampling modes
  metrpo_bptt_grad, metrpo_bptt_grad_stochastic, metrpo_validation_cost, metrpo_lbfgs_policy      the generic sweeps
  metrpo_svg_grad    auto -> generic; gemm refused
  metrpo_dyn_eval_losses against dynamics_oracle.validation_losses on DYN_LOSS; metrpo_dyn_train_step refused, state untouched
  the supplied-action family: rollout_actions in all modes, model_error, ensemble_disagreement, the four scoring calls with and without a terminal value

METRPO_TOL_REPORT=<file> (conftest.py) also makes this file write <file>.dyn_act.json: the worst share of every bound per entry point
(profiles/r29_dyn_act.txt)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from oracle import dynamics_oracle as D
import helpers as Hh
import tolerances as TOL
import rollout_check as CK
import bptt_cases as BC
import terminal_value_cases as TC
import disagreement_ref as DR
import model_error_ref as MR
import dyn_bf16_ref as BF
import lbfgs_ref as L
import dyn_act_cases as DA

pytestmark = pytest.mark.gpu

_WORST, _ENGINES = {}, {}
FIELDS = ('obs', 'act', 'mean', 'rew', 'done', 'tpath', 'last_obs', 'last_ts', 'last_model')


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _note(ep, row, share):
    d = _WORST.setdefault(ep, {})
    d[row] = max(d.get(row, 0.0), float(share))


@pytest.fixture(scope='module', autouse=True)
def _report():
    CK.REPORT.clear()
    t0 = time.time()
    yield
    _ENGINES.clear()
    for (form, what), used in CK.REPORT.items():
        _note(form, what, used)
    path = os.environ.get('METRPO_TOL_REPORT')
    if path:
        json.dump(dict(shares=_WORST, wall_seconds=time.time() - t0), open(path + '.dyn_act.json', 'w'), indent=1, sort_keys=True)


def engine(kind, env, K, hidden, acts, dm, theta):
    """One engine per net of a kind of problem (`kind` names whose weights it holds), kept while the module runs (the cases of a net share it)."""
    key = (kind, env, K, tuple(hidden), tuple(acts))
    if key not in _ENGINES:
        _ENGINES[key] = Hh.engine_of(env, K, tuple(hidden), DA.H32, dm, theta, dyn_act=list(acts))
    return _ENGINES[key]


def _same(a, b, what):
    for k in FIELDS:
        x, y = (v.view(np.uint64) if v.dtype == np.float64 else v for v in (a[k], b[k]))
        assert a[k].shape == b[k].shape and np.array_equal(x, y), '%s: %s differs' % (what, k)


# ---- metrpo_rollout ----------------------------------------------------------------------------------------------------------------------------------------
ROLL_IDS = ['%s-%s' % (n, DA.tag(a)) for n, a in DA.ROLLOUTS]


@pytest.mark.parametrize('name,acts', DA.ROLLOUTS, ids=ROLL_IDS)
def test_rollout_on_the_fallback_the_library_reports(name, acts):
    s, p = DA.SHAPE[name], DA.problem(name, acts)
    p.eng = Hh.engine_of(s.env, s.K, s.hidden, DA.H32, p.dm, p.th, dyn_act=list(acts))
    p.pool_t = torch.tensor(p.pool32, dtype=torch.float32, device=p.eng.device)
    try:
        for k, v in s.opts.items():
            p.eng.set_option(k, v)
        if s.exclusive:
            p.eng.set_exclusive(True)
        form = 'rollout ' + ('thread-per-env' if s.family == 'generic' else 'tile GEMMs')
        one_call = {}
        for i, c in enumerate(DA.rollout_cases(name, acts)):
            def launched(e, B=c.B):
                note = e.rollout_note()
                assert e.last_rollout_kernel() == s.family, (e.last_rollout_kernel(), note)
                if s.family == 'generic':
                    assert 'thread-per-env kernel' in note, note
                    return
                assert ('step-wise tile GEMMs' in note) if any(w % 256 for w in s.hidden) else note == '', note
                rep, exp = e.last_rollout_launch(), DA.expect_launch(s, acts, B)
                assert {k: rep[k] for k in exp} == exp, (rep, exp)
            dr = p.draws(c)[0]
            supplied = {k: (v.astype(np.float32) if v.dtype == np.float64 else v.astype(np.int32)) for k, v in dr.items()}
            dev = CK._device_run(p, c.B, c.T, c.H, c.mode, s.family, 0, determ=c.determ, supplied=supplied, chunks=c.chunks, launched=launched)
            DA.check_rollout(p, c, dev, '%s/%s/%s#%d' % (name, DA.tag(acts), c.name, i), form=form)
            if c.name == 'all-modes':
                one_call[c.mode] = dev
            elif c.name == 'chunked':
                _same(dev, one_call[c.mode], 'chunks (2, 1) against the one call')
    finally:
        del p.eng, p.pool_t


def test_relu_twins_of_the_declined_shapes_take_the_fused_families():
    """The same shapes and options with relu layers: cooperative, stream-K or persistent, resident, zero-padded cooperative.  So it is the activation
    that the fused families of the test above declined."""
    want = {'tile-64x64-hc': ('mfma-cooperative',), 'tile-64x64-ant': ('mfma-cooperative',), 'split-256x256': ('gemm-streamk', 'streamk-persistent'),
            'wide-512x512': ('resident',), 'narrow-48x20': ('mfma-cooperative',)}
    for name, fams in want.items():
        s = DA.SHAPE[name]
        dm, theta, pdims, pool = Hh.problem_data(s.env, s.K, s.hidden, DA.H32, seed=7, n_pool=64)
        eng = Hh.engine_of(s.env, s.K, s.hidden, DA.H32, dm, theta)
        for k, v in s.opts.items():
            eng.set_option(k, v)
        eng.set_exclusive(True)
        eng.rollout(17, 3, 2, 'step_rand', pool.astype(np.float32), seed=1)
        assert eng.last_rollout_kernel() in fams, (name, eng.last_rollout_kernel(), eng.rollout_note())
        if name == 'split-256x256':
            assert eng.last_rollout_launch()['sk_mode'] == 1


@pytest.mark.parametrize('acts', DA.BF16_VARIANTS, ids=DA.tag)
def test_rollout_bf16_operands(acts):
    """tests/test_gpu_dyn_bf16.py::test_random_nets_within_the_measured_bound under other activations: per-head rel-L2 of s' - s against the rounded
    float64 restatement, within dyn_bf16_ref.random_bound of the same case (8 x the float32 emulation's own distance)."""
    bound, fig, (dm, s, ac), ref = BF.random_bound(DA.BF16_HIDDEN, acts)
    env, B, K = 'half_cheetah', s.shape[0], dm.K
    pdims = O.policy_dims(dm.ns, DA.H32, dm.na)
    eng = Hh.engine_of(env, K, DA.BF16_HIDDEN, DA.H32, dm, np.zeros(O.policy_num_params(pdims)), dyn_act=list(acts))      # mean 0, log_std 0: the action is the draw
    eng.set_dyn_precision('bf16')
    rows = np.tile(np.arange(B), (2, 1))
    for k in range(K):
        tr = eng.rollout(B, 1, 10, 'step_rand', s, eps=ac[None], model_idx=np.full((1, B), k), reset_idx=rows, reset_model=np.zeros((2, B), np.int64))
        assert eng.last_rollout_kernel() == 'gemm-bf16'
        got = cpu(tr.last_obs) - s.astype(np.float64)
        rel = float(np.linalg.norm(got - ref[k]) / np.linalg.norm(ref[k]))
        print('bf16 %s head %d: rel-L2 %.3e (emulation %.3e, bound %.3e)' % (DA.tag(acts), k, rel, fig, bound))
        _note('rollout bf16', 'measured bound', rel / bound)
        assert rel <= bound, (rel, bound)


# ---- metrpo_step ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DA.STEP_SHAPES)
@pytest.mark.parametrize('acts', DA.TWO, ids=DA.tag)
def test_step_in_every_mode(name, acts):
    s, p = DA.SHAPE[name], DA.problem(name, acts)
    eng = engine('rollout', s.env, s.K, s.hidden, acts, p.dm, p.th)
    rng = np.random.RandomState(17)
    B = 17
    st, a = p.pool32[:B], DA.f32(0.8 * rng.randn(B, p.dm.na))
    idx, noise = rng.randint(p.K, size=B), DA.f32(rng.randn(B, p.dm.ns))
    for mode in O.SAM_MODES:
        nxt, rew, done, nall = eng.step(st.astype(np.float32), a.astype(np.float32), mode, model_idx=idx.astype(np.int32), noise=noise.astype(np.float32), want_all=True)
        rn, rr, rd, rh = DA.step_ref(p, st, a, mode, idx, noise)
        for what, got, ref, tol in (('next', nxt, rn, p.tol), ('heads', nall, rh, p.tol), ('rew', rew, rr, TOL.REWARD)):
            share = float((np.abs(cpu(got) - ref) / (tol['atol'] + tol['rtol'] * np.abs(ref))).max())
            _note('step', what, share)
            assert share <= 1.0, (mode, what, share)
        assert np.array_equal(cpu(done).astype(bool), rd)


# ---- the BPTT sweeps -----------------------------------------------------------------------------------------------------------------------------------------------
def _bptt_engine(c, d):
    eng = engine('bptt', c.env, c.K, c.dh, c.acts, d['dm'], d['th'])
    assert eng.set_det_path(True) == 0, c.id                           # the fused MFMA and the GEMM-path sweeps have declined: generic sweeps
    eng.set_policy(d['th'])
    return eng


@pytest.mark.parametrize('case', DA.BPTT_CASES, ids=[c.id for c in DA.BPTT_CASES])
def test_bptt_on_the_generic_sweeps(case):
    d = DA.bptt_data(case)
    assert d['accepted'] == case.B and d['replaced'] <= DA.MAX_REPLACED * case.B
    eng = _bptt_engine(case, d)
    x0 = d['x0'].astype(np.float32)
    if case.stoch:
        costs, g = (cpu(t) for t in eng.bptt_grad_stochastic(x0, case.T, case.gamma, noise=d['eps'].astype(np.float32)))
    else:
        costs, g = (cpu(t) for t in eng.bptt_grad(x0, case.T, case.gamma))
    assert np.all(np.isfinite(costs)) and np.all(np.isfinite(g))
    cost, whole, worst, where = DA.bptt_shares(costs, g, d)
    ep = 'bptt_grad_stochastic' if case.stoch else 'bptt_grad'
    _note(ep, 'BPTT_COST', cost); _note(ep, 'BPTT_GRAD_REL_L2', whole); _note(ep, 'BPTT_GRAD_REL_L2 per variable', worst)
    print('%s: cost %.3g, gradient %.3g whole, %.3g per variable (%s) of their bounds' % (case.id, cost, whole, worst, where))
    assert cost <= 1.0 and whole <= 1.0 and worst <= 1.0, (cost, whole, worst, where)
    if not case.stoch:
        assert np.all(g[-d['dm'].na:] == 0.0)
        v = cpu(eng.validation_cost(x0, case.T, case.gamma))
        vshare = BC.cost_use(v, DA.bptt_reference(d)[0])
        _note('validation_cost', 'BPTT_COST', vshare)
        assert vshare <= 1.0, vshare
        np.testing.assert_allclose(v, costs, rtol=1e-6, atol=1e-7)     # the same forward sweep without the tape (tests/test_gpu_bptt_edges.py's figure)


def test_lbfgs_policy_on_a_tanh_net_matches_the_host_driven_loop():
    from test_gpu_lbfgs import host_fg
    env, K, dh, acts, B, T = DA.LBFGS_CASE
    case = next(c for c in DA.BPTT_CASES if (c.env, c.dh, c.acts, c.B, c.T, c.stoch) == (env, dh, acts, B, T, False))
    d = DA.bptt_data(case)
    eng = _bptt_engine(case, d)
    x0, gamma = d['x0'].astype(np.float32), case.gamma
    th0 = eng.get_policy().cpu().numpy()
    r = L.minimize(host_fg(eng, x0, T, gamma), th0.astype(np.float64), maxiter=3)
    eng.set_policy(th0)
    out = eng.lbfgs_policy(x0, T, gamma, eng.lbfgs_opts(maxiter=3))
    assert (out['nit'], out['nfev'], out['task'], out['status']) == (r.nit, r.nfev, r.task, r.status) and r.nit >= 1
    th = eng.get_policy().cpu().numpy()
    assert np.array_equal(th, r.x.astype(np.float32)) and out['fun'] == r.fun
    oc0 = Bp.policy_costs_and_grad(d['dm'], th0.astype(np.float64), d['pdims'], env, d['x0'], T, gamma)[0]
    oc = Bp.policy_costs_and_grad(d['dm'], th.astype(np.float64), d['pdims'], env, d['x0'], T, gamma)[0]
    assert out['fun'] < float(np.mean(oc0))
    np.testing.assert_allclose(out['fun'], np.mean(oc), **TOL.BPTT_COST)
    eng.set_policy(d['th'])


# ---- metrpo_svg_grad -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', DA.SVG_NETS, ids=['%s-%s' % (n[0], DA.tag(n[3])) for n in DA.SVG_NETS])
def test_svg_auto_is_generic_and_gemm_is_refused(net):
    from metrpo_amd._lib import MetrpoError
    env, K, dh, acts = net
    d = DA.svg_data(*net)
    eng = engine('svg', env, K, dh, acts, d['dm'], d['theta'])
    eng.set_policy(d['theta'])
    args = (d['obs'].astype(np.float32), d['act'].astype(np.float32), d['lengths'])
    got = {k: cpu(v) for k, v in eng.svg_grad(*args, model=DA.SVG_MODEL, gamma=DA.SVG_GAMMA, path='auto').items()}
    assert eng.last_svg_path() == 'generic'
    whole, worst, state = DA.svg_shares(got, d)
    for row, share in (('GRAD_REL_L2', whole), ('GRAD_REL_L2 per variable', worst), ('GRAD_REL_L2 state', state)):
        _note('svg_grad', row, share)
    print('svg %s %s: %.3g whole, %.3g per variable, %.3g state of their bounds' % (env, DA.tag(acts), whole, worst, state))
    assert whole <= 1.0 and worst <= 1.0 and state <= 1.0
    assert np.all(got['theta'][-d['dm'].na:] == 0.0)
    with pytest.raises(MetrpoError, match='needs relu hidden layers'):
        eng.svg_grad(*args, model=DA.SVG_MODEL, gamma=DA.SVG_GAMMA, path='gemm')


# ---- metrpo_dyn_eval_losses, metrpo_dyn_train_step ---------------------------------------------------------------------------------------------------------------------
EVAL_IDS = ['%s-%s' % ('x'.join(map(str, h)), DA.tag(a)) for h, a in DA.EVAL_NETS]


@pytest.mark.parametrize('hidden,acts', DA.EVAL_NETS, ids=EVAL_IDS)
def test_eval_losses_against_the_validation_losses(hidden, acts):
    """On the build before train_forward took identity layers (it launched EPI_BIAS_TANH for everything but relu) the seven nets with an identity layer
    failed this test -- at n = 1, reg = 0 by 558 ... 2817 x DYN_LOSS, the layer<l>_tanh mutation of tests/test_dyn_act_cases.py -- and the six without one
    passed; all thirteen pass since."""
    dm, th, pdims, pool = DA.eval_problem(hidden, acts)
    eng = engine('eval', DA.EVAL_ENV, DA.EVAL_K, hidden, acts, dm, th)
    for n in DA.eval_rows(hidden):
        x, y = DA.eval_data(dm, pool, n)
        for reg in DA.EVAL_REGS:
            got = cpu(eng.eval_losses(x.astype(np.float32), y.astype(np.float32), reg))
            share = DA.loss_share(got, D.validation_losses(dm, x, y, reg))
            print('eval_losses %s %s n %d reg %g: %.3g of DYN_LOSS' % (hidden, DA.tag(acts), n, reg, share))
            _note('dyn_eval_losses', 'DYN_LOSS', share)
            assert share <= 1.0, (n, reg, share, got)


@pytest.mark.parametrize('acts', DA.TRAIN_REFUSED, ids=DA.tag)
def test_train_step_refuses_and_touches_nothing(acts):
    from metrpo_amd._lib import MetrpoError
    hidden = (64, 64)
    dm, th, pdims, pool = DA.eval_problem(hidden, acts)
    eng = Hh.engine_of(DA.EVAL_ENV, DA.EVAL_K, hidden, DA.H32, dm, th, dyn_act=list(acts))
    rng = np.random.RandomState(1)
    shape = (DA.EVAL_K, eng.dyn_param_count)
    eng.set_train_adam(rng.randn(*shape).astype(np.float32), rng.rand(*shape).astype(np.float32), 5)
    before = [t.clone() for t in (eng.get_dynamics(),) + eng.get_train_adam()[:2]]
    bs = 17
    x, y = DA.eval_data(dm, pool, bs * DA.EVAL_K)
    with pytest.raises(MetrpoError, match='unsupported configuration: dyn_train: only relu hidden layers'):
        eng.train_step(x.astype(np.float32), y.astype(np.float32), bs, 1e-3)
    m, v, t = eng.get_train_adam()
    assert t == 5
    for a, b in zip(before, (eng.get_dynamics(), m, v)):
        assert torch.equal(a, b)


# ---- the supplied-action family --------------------------------------------------------------------------------------------------------------------------------------------
def _supplied_engine(case):
    dm, th, pdims, pool = DA.supplied_problem(case.env, case.K, case.act)
    return engine('supplied', case.env, case.K, case.dh, case.act, dm, th)


def _score(eng, d, which, force=False):
    """One of the four scoring calls on a case's data, with whatever terminal value the engine holds -> (host dict, the path the library reports)."""
    case, loop = d['case'], d['loop']
    init = np.asarray(d['init'], np.float32)
    seq = torch.as_tensor(d['seq'], dtype=torch.float32, device=eng.device)
    kw = dict(gamma=case.gamma, stop_at_done=case.stop, force_generic=force)
    want = ('ret', 'len') if which == 'score' else ('grad', 'ret', 'len', 'lam0')
    if loop == 'open':
        if which == 'score':
            out, kern = eng.score_actions(init, seq, want=want, **kw), eng.last_score_actions_kernel()
        else:
            out, kern = eng.score_actions_grad(init, seq, want=want, **kw), eng.last_score_actions_grad_kernel()
    else:
        kw.update(T=case.T, noise_in_std=case.in_std)
        if which == 'score':
            out, kern = eng.score_policy_actions(init, seq, want=want, **kw), eng.last_score_policy_actions_kernel()
        else:
            out, kern = eng.score_policy_actions_grad(init, seq, want=want, **kw), eng.last_score_policy_actions_grad_kernel()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, kern


@pytest.mark.parametrize('case,loop', DA.SUPPLIED_RUNS, ids=['%s-%s' % (c.id, l) for c, l in DA.SUPPLIED_RUNS])
def test_scoring_calls_report_generic_and_match_the_restatement(case, loop):
    d = DA.supplied_data(case, loop)
    assert d['accepted'] == case.B and d['replaced'] <= DA.MAX_REPLACED * case.B
    eng = _supplied_engine(case)
    eng.set_policy(d['theta'])
    ref = TC.reference(d)
    if 'plain' not in d:
        d['plain'] = TC.walk(d, tv=None)
    res = {}
    for tv in (False, True):
        if tv:
            eng.set_terminal_value(*d['tv'])
        try:
            for which in ('score', 'grad'):
                res[(tv, which)], kern = _score(eng, d, which)
                assert kern == 'generic', (tv, which, kern)                # a shape of the fused class apart from its activations: never 'fused'
        finally:
            eng.clear_terminal_value()
    eps = ('score_policy_actions', 'score_policy_actions_grad') if loop == 'closed' else ('score_actions', 'score_actions_grad')
    for tv, r in ((False, d['plain']), (True, ref)):
        use = TC.shares(res[(tv, 'grad')], r, case) if tv else TC.GC.shares(res[(tv, 'grad')], r, case)
        suse = (TC.shares(dict(ret=res[(tv, 'score')]['ret']), r, case) if tv else TC.GC.shares(dict(res[(tv, 'grad')], ret=res[(tv, 'score')]['ret']), r, case))[5]
        sfx = ' + terminal value' if tv else ''
        _note(eps[0] + sfx, 'ret', suse)
        for row, share in zip(('grad whole', 'grad per step', 'grad per candidate', 'lam0 whole', 'lam0 per candidate', 'ret'), use):
            _note(eps[1] + sfx, row, share)
        print('%s %s%s: %s, scoring ret %.3g of their bounds' % (case.id, loop, sfx, np.array2string(np.asarray(use), precision=3), suse))
        assert max(use) <= 1.0 and suse <= 1.0, (tv, use, suse)
        assert np.array_equal(res[(tv, 'grad')]['len'], r['len']) and np.array_equal(res[(tv, 'score')]['len'], r['len'])
        assert np.array_equal(res[(tv, 'score')]['ret'], res[(tv, 'grad')]['ret'])                       # the gradient call carries the scoring call's bits
    # the relu twin of the same weights, forced generic: another result, so the activation was used
    dm = d['dm']
    twin = engine('supplied', case.env, case.K, case.dh, ('relu', 'relu') + case.act, dm, d['theta'])
    twin.set_policy(d['theta'])
    tw, kern = _score(twin, d, 'score', force=True)
    assert kern == 'generic'
    assert TC.GC.shares(dict(res[(False, 'grad')], ret=tw['ret']), d['plain'], case)[5] > 1.0


@pytest.mark.parametrize('env,K', DA.SUPPLIED_NETS)
@pytest.mark.parametrize('acts', DA.SUPPLIED_VARIANTS, ids=DA.tag)
def test_rollout_actions_model_error_and_disagreement(env, K, acts):
    from metrpo_amd import model_error as M
    from test_gpu_model_error import bounds as me_bounds
    dm, th, pdims, pool = DA.supplied_problem(env, K, acts)
    eng = engine('supplied', env, K, (64, 64), acts, dm, th)
    eng.set_policy(th)
    rng = np.random.RandomState(23)
    B, T = 17, DA.SUPPLIED_T
    init, actions = pool[:B], DA.f32(1.5 * rng.randn(T, B, dm.na))
    heads, midx, noise = rng.randint(K, size=B), rng.randint(K, size=(T, B)), DA.f32(rng.randn(T, B, dm.ns))
    a_dev = torch.as_tensor(actions, dtype=torch.float32, device=eng.device)
    i32 = lambda a: torch.as_tensor(a, dtype=torch.int32)
    modes = [('model_mean', {}, {}), ('eps_rand', dict(model=i32(heads)), dict(model=heads)), ('eps_rand', dict(model=K - 1), dict(model=np.full(B, K - 1))),
             ('one_model', {}, {}), ('step_rand', dict(model_idx=i32(midx)), dict(model_idx=midx)),
             ('model_mean_std', dict(noise=noise.astype(np.float32)), dict(noise=noise)), ('model_med', {}, {})]
    twin = engine('supplied', env, K, (64, 64), ('relu', 'relu') + tuple(acts), dm, th)
    for mode, kw, rkw in modes:
        obs, rew, done = eng.rollout_actions(init.astype(np.float32), a_dev, sam_mode=mode, **kw)
        assert eng.last_rollout_actions_kernel() == 'step-loop', mode
        ref = DA.rollout_actions_ref(dm, env, init, actions, mode, **rkw)
        for what, got, r, tol in (('obs', cpu(obs)[1:], ref['obs'][1:], TOL.FREE_RUN), ('rew', cpu(rew), ref['rew'], TOL.REWARD)):
            share = float((np.abs(got - r) / (tol['atol'] + tol['rtol'] * np.abs(r))).max())
            _note('rollout_actions', what, share)
            assert share <= 1.0, (mode, what, share)
        assert np.array_equal(cpu(done).astype(bool), ref['done'])
        if mode in ('model_mean', 'one_model'):                            # the forced step loop of the relu twin: another result
            tobs = cpu(twin.rollout_actions(init.astype(np.float32), a_dev, sam_mode=mode, force_step_loop=True)[0])
            assert twin.last_rollout_actions_kernel() == 'step-loop'
            assert float((np.abs(tobs[1] - ref['obs'][1]) / (TOL.FREE_RUN['atol'] + TOL.FREE_RUN['rtol'] * np.abs(ref['obs'][1]))).max()) > 1.0
    # ---- ensemble_disagreement
    N = 33
    o2, a2 = pool[40:40 + N], DA.f32(1.5 * rng.randn(N, dm.na))
    got = {k: cpu(v) for k, v in eng.ensemble_disagreement(o2.astype(np.float32), a2.astype(np.float32),
                                                           want=('score', 'maxdev', 'std', 'mean', 'next_all', 'rew_std')).items()}
    assert eng.last_disagreement_kernel() == 'generic'
    sh = DR.shares(got, DR.disagreement(dm, env, o2, a2), TOL.STEP)
    for k, v in sh.items():
        _note('ensemble_disagreement', k, v)
    assert max(sh.values()) <= 1.0, sh
    # ---- model_error: the policy's rollout through metrpo_rollout's dispatch, and the recorded actions through rollout_actions' step loop
    Os, As, Rs = MR.recorded_trajectories(dm, th, pdims, env, pool, 3, 5, seed=1)
    hs = (1, 3, 5)
    for known in (False, True):
        for model in (-1, 0):
            r = M.model_error(eng, Os, As, Rs, list(hs), model=model, known_actions=known)
            assert (eng.last_rollout_actions_kernel() == 'step-loop') if known else (eng.last_rollout_kernel() == 'gemm-stepwise')
            ref = MR.evaluate_model_predictions(dm, th, pdims, env, Os, Rs, timesteps=hs, model=model, As=As, known_actions=known)
            g_sd, g_cd, g_va = cpu(r['state_diff']), cpu(r['cost_diff']), cpu(r['valid']).astype(bool)
            for p_, h in enumerate(hs):
                e = ref['per_h'][p_]
                w, k = e['i'] * 5 + e['t'], e['keep']
                assert k.all() and g_va[p_][w].all()
                b_state, b_cost = me_bounds(e, h)
                s_state = float((np.abs(g_sd[p_][w] - e['state_diff']) / b_state).max()); s_cost = float((np.abs(g_cd[p_][w] - e['cost_diff']) / b_cost).max())
                _note('model_error', 'state_diff', s_state); _note('model_error', 'cost_diff', s_cost)
                assert s_state <= 1.0 and s_cost <= 1.0, (known, model, h, s_state, s_cost)
