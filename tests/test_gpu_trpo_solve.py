"""The CG solve and the line search of metrpo_trpo_update against float64 at the tile edges, on every kernel family: what tests/test_gpu_update_kernels.py
leaves out.  Per case of tests/solve_cases.py (the cases of update_cases.py at cg_iters = 2, one lead N per shape also at 0, 1, 3, 10; residual_tol = 0,
reg_coeff = solve_cases.REG):
  * the whole-batch update: g within GRAD_REL_L2 (whole and per block), loss_before within LOSS_RTOL, d, beta and step = beta d within the bounds
    solve_cases derives from the reference (the float64 solve started from the DEVICE's g, its products perturbed by what FVP_REL_L2 admits), cg_iters_run,
    and what Engine.last_solve_launch reports of the products: family, table, the cached op, the scope;
  * the same update with fvp_batch a second make_batch of the same arrays (other pointers: the products run uncached): g bit for bit, d and beta within
    the same bounds, the cached-versus-uncached distance recorded;
  * the tail of the update, teacher-forced: the accepted policy is float32(theta_prev - ratio^n beta_dev d_dev) within one fp32 ulp per element, diag.loss
    / diag.kl match float64 at the device's own theta (LOSS_RTOL, KL_ATOL / KL_RTOL), and float64 loss and KL at every device trial theta agree with the
    device's accept sequence wherever they are clear of the thresholds.
Routes (two halves with 1 and 3 speculated trials, explicit_final_hvp, a host all-reduce callback = the stand-alone CG kernels), a rejected update, and
cache / state hygiene against fresh engines follow; test_cases_reach_every_path asserts the coverage from the reported launches.
Sharded routes stay with tests/test_gpu_comm.py; the early exit with tests/test_gpu_engine.py.

Observed on an MI355X (worst share of each bound, cached-versus-uncached distance, worst ulp distance, per family): profiles/r12_trpo_solve.txt."""
import json
import os

import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import tolerances as TOL
import update_cases as U
import solve_cases as S
from helpers import engine_of
from test_gpu_update_kernels import engine_for, derive_n, cpu

pytestmark = pytest.mark.gpu
_SOLVES, _ROUTES, _WORST = {}, [], {}
KEYS = ('loss_before', 'loss', 'kl', 'beta', 'n_backtrack', 'accepted', 'cg_iters_run')
HYGIENE = {'mfma': ('swimmer', (32, 32)), 'fused3': ('humanoid', (100, 50, 25)), 'generic': ('swimmer', (32, 32)), 'gemm': ('swimmer', (65, 33))}


def _note(family, row, value):
    """Worst figure per family and row; with METRPO_TOL_REPORT set also written next to the other reports."""
    _WORST.setdefault(family, {})
    _WORST[family][row] = max(_WORST[family].get(row, 0.0), float(value))
    if os.environ.get('METRPO_TOL_REPORT'):
        json.dump(_WORST, open(os.environ['METRPO_TOL_REPORT'] + '.trpo_solve', 'w'), indent=1, sort_keys=True)


def update(eng, batch, k, **kw):
    return eng.trpo_update(batch, max_kl=S.MAX_KL, cg_iters=k, reg_coeff=S.REG, backtrack_ratio=S.RATIO, max_backtracks=S.MAX_BACKTRACKS,
                           residual_tol=0.0, want_vectors=True, **kw)


def batch_of(eng, d, adv=None):
    return eng.make_batch(d['obs'], d['act'], d['adv'] if adv is None else adv, d['om'], d['ols'], valid=d['valid'])


def engine_or_none(uc, d):
    from metrpo_amd._lib import MetrpoError
    try:
        return engine_for(uc, d)
    except MetrpoError as e:                                # a policy without a hidden layer may be refused, by name (as in test_gpu_update_kernels.py)
        assert uc.ph == () and str(e).split(':')[0] in ('unsupported configuration', 'invalid argument'), e
        return None


def fresh_engine(uc, d):
    eng = engine_of(uc.env, 2, (64, 64), uc.ph, d['dm'], d['th'])
    path = U.PATHS[uc.family][0]
    assert eng.set_update_path(path) == path
    return eng


def want_record(uc, k, cached=True, fused=True, explicit=False):
    n = (k + (1 if explicit and k > 0 else 0))
    mfma = uc.family == 'mfma'
    return dict(family=uc.family, table=U.FUSED_ENVS.index(uc.env) if mfma else -1, n_fvp=n,
                op=-1 if n == 0 else (3 if mfma and cached else 1), cache_activations=cached, publish_image=bool(mfma and cached and fused),
                fused_tails=fused, fvp_batch=not cached)


def ulps(got, want):
    """Largest |got - want| in units of the fp32 spacing at `want` (both fp32 values held in float64)."""
    sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - want) / sp)) if got.size else 0.0


def snapshot(eng, out):
    return dict(out={k: out[k] for k in KEYS}, g=out['g'].clone(), d=out['d'].clone(), theta=eng.get_policy().clone())


def same_bits(a, b):
    for k in KEYS:
        x, y = a['out'][k], b['out'][k]
        if not (x == y or (isinstance(x, float) and np.isnan(x) and np.isnan(y))):
            return False, k
    for k in ('g', 'd', 'theta'):
        if not torch.equal(a[k].view(torch.int64 if a[k].dtype == torch.float64 else torch.int32), b[k].view(torch.int64 if b[k].dtype == torch.float64 else torch.int32)):
            return False, k
    return True, None


@pytest.mark.parametrize('case', S.CASES, ids=[c.id for c in S.CASES])
def test_solve_matches_float64(case):
    uc, k = case.ucase, case.k
    eng = engine_or_none(uc, U.case_data(uc, 1) if not isinstance(uc.nspec, int) else U.case_data(uc))
    if eng is None:
        return
    N = derive_n(uc, eng)
    d = U.case_data(uc, N)
    pd, th, fails = d['pdims'], d['th'], []
    assert eng.update_path(N) == U.PATHS[uc.family][1]

    def hold(row, share, what=''):
        _note(uc.family, row, share)
        print('%s %s%s: %.3g of the bound' % (case.id, row, what, share))
        if not share <= 1.0:
            fails.append((row, what, share))

    # ---- the whole-batch update (cached products)
    eng.set_policy(th)
    b1 = batch_of(eng, d)
    out = update(eng, b1, k)
    rec = eng.last_solve_launch()
    theta_dev = cpu(eng.get_policy())
    g_dev, d_dev, beta_dev = cpu(out['g']), cpu(out['d']), float(out['beta'])
    _SOLVES[case.id] = (N, th.size, rec)
    assert rec == want_record(uc, k), (case.id, rec)
    assert out['cg_iters_run'] == k
    pb = S.problem(d)
    loss0, g_ref = O.surrogate_loss_grad(th, pd, *pb['sel'])
    hold('LOSS_RTOL', abs(out['loss_before'] - loss0) / (TOL.LOSS_RTOL * max(1.0, abs(loss0))), ' loss_before')
    worst, where, whole = U.vector_use(g_dev, g_ref, TOL.GRAD_REL_L2, pd)
    hold('GRAD_REL_L2', whole)
    hold('GRAD_REL_L2 per block', worst, ' ' + where)
    ref, bounds = S.solve_and_bounds(d, k, g=g_dev, draws=case.draws)
    sh = S.shares(d_dev, beta_dev, ref, bounds, pd)
    hold('solve d', sh['d'][0], ' ' + sh['d'][1]); hold('solve beta', sh['beta']); hold('solve step', sh['step'][0], ' ' + sh['step'][1])

    # ---- the tail of the update, teacher-forced on the device's own beta and d
    n, accepted = int(out['n_backtrack']), bool(out['accepted'])
    if accepted:
        want = S.trial_theta(th, beta_dev, d_dev, n)
        u = ulps(theta_dev, want)
        _note(uc.family, 'accepted policy, fp32 ulps', u)
        assert u <= 1.0, (case.id, u)
        loss_at, kl_at = O.surrogate_loss_kl(theta_dev, pd, *pb['sel'])
    else:
        assert np.array_equal(theta_dev, th), case.id                      # restored bit for bit
        with np.errstate(all='ignore'):
            loss_at, kl_at = O.surrogate_loss_kl(S.trial_theta(th, beta_dev, d_dev, n), pd, *pb['sel'])
    if k > 0:                                               # (k = 0: the trial theta IS theta; the loss there is loss_before, held above)
        hold('LOSS_RTOL', abs(out['loss'] - loss_at) / (TOL.LOSS_RTOL * max(1.0, abs(loss_at))), ' diag.loss')
        hold('KL', abs(out['kl'] - kl_at) / max(TOL.KL_ATOL, TOL.KL_RTOL * abs(kl_at)), ' diag.kl')
    else:
        assert np.array_equal(theta_dev, th) and np.all(d_dev == 0.0), case.id
    n_clear = 0
    for nn, loss, kl, acc, clear in S.line_search(d, beta_dev, d_dev, loss_before=loss0, upto=n):
        if clear:
            n_clear += 1
            assert acc == (accepted and nn == n), (case.id, nn, loss, kl, loss0, out)
    assert k == 0 or n_clear >= 1, case.id

    # ---- the same update with the products on a second batch of the same arrays: uncached
    eng.set_policy(th)
    b2 = batch_of(eng, d)
    out2 = update(eng, b1, k, fvp_batch=b2)
    rec2 = eng.last_solve_launch()
    assert rec2 == want_record(uc, k, cached=False), (case.id, rec2)
    assert torch.equal(out2['g'], out['g']) and out2['loss_before'] == out['loss_before'] and out2['cg_iters_run'] == k
    d2, beta2 = cpu(out2['d']), float(out2['beta'])
    sh2 = S.shares(d2, beta2, ref, bounds, pd)
    hold('solve d', sh2['d'][0], ' uncached ' + sh2['d'][1]); hold('solve beta', sh2['beta'], ' uncached'); hold('solve step', sh2['step'][0], ' uncached ' + sh2['step'][1])
    dist = float(np.linalg.norm(d2 - d_dev) / max(np.linalg.norm(d_dev), 1e-300)) if k > 0 else 0.0
    _note(uc.family, 'cached vs uncached, rel-L2 of d', dist)
    print('%s cached vs uncached: %.3g' % (case.id, dist))
    eng.set_policy(th)
    assert not fails, (case.id, N, fails)


def _route_cases():
    """The lead N of every (family, env, policy shape) and N = 17 with mask `seven` (a case of the table where it has one, else made here)."""
    out, seen = [], set()
    for c in S.CASES:
        uc = c.ucase
        key = (uc.family, uc.env, uc.ph)
        if key in seen:
            continue
        seen.add(key)
        lead = next(x.ucase for x in S.CASES if (x.ucase.family, x.ucase.env, x.ucase.ph) == key and x.k == S.K_ALL and x.ucase.nspec == S.lead_n(uc) and x.ucase.mask == 'none')
        small = next((x.ucase for x in S.CASES if (x.ucase.family, x.ucase.env, x.ucase.ph) == key and x.k == S.K_ALL and x.ucase.nspec == 17 and x.ucase.mask == 'seven'), None)
        if small is None:
            small = U.Case('%s-%s-%s-N17-seven' % (uc.family, uc.env, 'x'.join(str(h) for h in uc.ph)), uc.family, uc.env, uc.ph, 17, 'seven', 4000 + len(out))
        out += [lead, small]
    return out


ROUTE_CASES = _route_cases()


@pytest.mark.parametrize('uc', ROUTE_CASES, ids=[u.id for u in ROUTE_CASES])
def test_routes_agree(uc):
    k = S.K_ALL
    d = U.case_data(uc)
    eng = engine_or_none(uc, d)
    if eng is None:
        return
    th, pd = d['th'], d['pdims']
    b = batch_of(eng, d)
    eng.set_policy(th)
    one = snapshot(eng, update(eng, b, k))
    ref, bounds = S.solve_and_bounds(d, k, g=cpu(one['g']))
    # two halves, the first 1 / 3 trials decided on the device (the GEMM path runs the whole update inside the first half)
    for spec in (1, 3):
        eng.set_policy(th)
        assert update(eng, b, k, spec_trials=spec) is None
        two = snapshot(eng, eng.trpo_update_end())
        assert same_bits(one, two) == (True, None), (uc.id, spec, same_bits(one, two))
        assert eng.last_solve_launch() == want_record(uc, k)
    # rllab's literal step scale: one more product on d
    eng.set_policy(th)
    exp = snapshot(eng, update(eng, b, k, explicit_final_hvp=True))
    assert eng.last_solve_launch() == want_record(uc, k, explicit=True)
    assert torch.equal(exp['g'], one['g']) and torch.equal(exp['d'], one['d'])
    sh = S.shares(cpu(exp['d']), exp['out']['beta'], ref, bounds, pd)
    _note(uc.family, 'solve beta', sh['beta'])
    assert sh['beta'] <= 1.0, (uc.id, sh)
    # a host all-reduce callback between every reduction and its consumer: the stand-alone k_cg_init / k_cg_step / k_cg_finish*
    eng.set_policy(th)
    cb = snapshot(eng, update(eng, b, k, allreduce=lambda t: t))
    rec = eng.last_solve_launch()
    _ROUTES.append((uc, rec))
    assert rec == want_record(uc, k, fused=False), (uc.id, rec)
    sh = S.shares(cpu(cb['d']), cb['out']['beta'], ref, bounds, pd)
    for row in ('d', 'step'):
        _note(uc.family, 'solve ' + row, sh[row][0])
    _note(uc.family, 'solve beta', sh['beta'])
    assert S.worst_share(sh) <= 1.0, (uc.id, sh)
    assert torch.equal(cb['g'], one['g'])
    assert (cb['out']['n_backtrack'], cb['out']['accepted']) == (one['out']['n_backtrack'], one['out']['accepted']), (uc.id, cb['out'], one['out'])
    eng.set_policy(th)


@pytest.mark.parametrize('family', sorted(HYGIENE))
def test_rejected_update_restores_the_policy(family):
    """N = 17, advantages of zero: the gradient is zero, no trial improves the loss; the policy keeps its bits on the one-call and on the two-halves route."""
    env, ph = HYGIENE[family]
    uc = U.Case('rejected-' + family, family, env, ph, 17, 'none', 4100)
    d = U.case_data(uc)
    eng = engine_for(uc, d)
    b = batch_of(eng, d, adv=np.zeros(17))
    th0 = torch.as_tensor(d['th'], dtype=torch.float32)
    for spec in (0, 1, 3):
        eng.set_policy(d['th'])
        out = update(eng, b, S.K_ALL, spec_trials=spec) if not spec else (update(eng, b, S.K_ALL, spec_trials=spec), eng.trpo_update_end())[1]
        assert not out['accepted'], (family, spec, out)
        assert torch.equal(eng.get_policy().cpu().view(torch.int32), th0.view(torch.int32)), (family, spec)


def _hygiene_case(family, N, seed=4200):
    env, ph = HYGIENE[family]
    return U.Case('hygiene-%s-N%d' % (family, N), family, env, ph, N, 'seven', seed + N)


@pytest.mark.parametrize('family', sorted(HYGIENE))
def test_a_solve_does_not_depend_on_the_one_before(family):
    """Bit for bit a fresh engine's: N = 17 after N = 129 on one engine (the caches hold 129 rows), and N = 129 after N = 17 (the workspace grows)."""
    u17, u129 = _hygiene_case(family, 17), _hygiene_case(family, 129)
    d17, d129 = U.case_data(u17), U.case_data(u129)
    want = {}
    for uc, d in ((u17, d17), (u129, d129)):
        eng = fresh_engine(uc, d)
        want[d['N']] = snapshot(eng, update(eng, batch_of(eng, d), S.K_ALL))
    for first, second in (((u129, d129), (u17, d17)), ((u17, d17), (u129, d129))):
        eng = fresh_engine(first[0], first[1])
        update(eng, batch_of(eng, first[1]), S.K_ALL)
        eng.set_policy(second[1]['th'])
        got = snapshot(eng, update(eng, batch_of(eng, second[1]), S.K_ALL))
        assert same_bits(got, want[second[1]['N']]) == (True, None), (family, first[1]['N'], second[1]['N'], same_bits(got, want[second[1]['N']]))


@pytest.mark.parametrize('family', sorted(HYGIENE))
def test_a_solve_after_the_batch_was_overwritten_in_place(family):
    """Same pointers, new data, new theta: nothing cached for the first solve (activations, forward pass, image) serves the second."""
    ua, ub = _hygiene_case(family, 129, seed=4300), _hygiene_case(family, 129, seed=4400)
    da, db = U.case_data(ua), U.case_data(ub)
    eng = fresh_engine(ub, db)
    want = snapshot(eng, update(eng, batch_of(eng, db), S.K_ALL))
    eng = fresh_engine(ua, da)
    b = batch_of(eng, da)
    update(eng, b, S.K_ALL)
    obs, act, adv, om, ols, valid = b._keep
    for t, src in ((obs, db['obs']), (act, db['act']), (adv, db['adv']), (om, db['om']), (ols, db['ols']), (valid, db['valid'])):
        t.copy_(torch.as_tensor(np.asarray(src).reshape(tuple(t.shape))).to(t.dtype))
    eng.set_policy(db['th'])
    got = snapshot(eng, update(eng, b, S.K_ALL))
    assert same_bits(got, want) == (True, None), (family, same_bits(got, want))


@pytest.mark.parametrize('family', sorted(HYGIENE))
def test_fvp_alone_before_and_after_a_solve(family):
    """metrpo_fvp as a call of its own recomputes its activations: the same bits before and after a solve left its caches, and op 1 noted."""
    uc = _hygiene_case(family, 129)
    d = U.case_data(uc)
    eng = fresh_engine(uc, d)
    b = batch_of(eng, d)
    before = eng.fvp(b, d['v']).clone()
    assert eng.last_update_launch()['op'] == 1 and eng.last_update_launch()['family'] == family
    update(eng, b, S.K_ALL)
    eng.set_policy(d['th'])
    after = eng.fvp(b, d['v'])
    assert eng.last_update_launch()['op'] == 1
    assert torch.equal(before.view(torch.int64), after.view(torch.int64)), family
    ref = S.fisher(S.problem(d))(d['v'])
    assert U.vector_use(cpu(after), ref, TOL.FVP_REL_L2, d['pdims'])[0] <= 1.0


@pytest.mark.parametrize('family', sorted(HYGIENE))
def test_twenty_updates_in_a_row(family):
    """Twenty updates on one engine, each from the policy the one before left, equal twenty updates on fresh engines: the arrival ticket, the
    weight-fragment image and the caches are left clean by every update."""
    uc = _hygiene_case(family, 129)
    d = U.case_data(uc)
    eng = fresh_engine(uc, d)
    b = batch_of(eng, d)
    run, thetas = [], [eng.get_policy().clone()]
    for i in range(20):
        run.append(snapshot(eng, update(eng, b, S.K_ALL)))
        thetas.append(run[-1]['theta'])
    # (the batch's old distribution stays the first theta's: once the KL to it is spent the search rejects and the policy is restored -- both ends of an update are in the run)
    acc = [bool(r['out']['accepted']) for r in run]
    assert any(acc) and not all(acc), acc
    for i in range(20):
        fe = fresh_engine(uc, d)
        fe.set_policy(thetas[i])
        got = snapshot(fe, update(fe, batch_of(fe, d), S.K_ALL))
        assert same_bits(got, run[i]) == (True, None), (family, i, same_bits(got, run[i]))
        del fe


def test_cases_reach_every_path():
    """From what the library reports of the solves of the table's cases (those test_solve_matches_float64 already made in this process; the others, with
    no mask, are launched here without their references): all five fused 2 x 32 tables with the cached op, the fused 100-50-25 kernels, each sample tile
    of the generic kernels, the GEMM path with P below one block, a P in each of the four ranges of the CG step, fused and stand-alone tails."""
    for case in S.CASES:
        uc = case.ucase
        if case.id in _SOLVES or uc.mask != 'none' or case.k != S.K_ALL:
            continue
        eng = engine_or_none(uc, U.case_data(uc, 1))
        if eng is None:
            continue
        N = derive_n(uc, eng)
        d = U.case_data(uc, N)
        eng.set_policy(d['th'])
        update(eng, batch_of(eng, d), case.k)
        _SOLVES[case.id] = (N, d['th'].size, eng.last_solve_launch())
        eng.set_policy(d['th'])
    by = {c.id: c for c in S.CASES}
    reps = [(by[i].ucase, by[i].k, N, P, rec) for i, (N, P, rec) in _SOLVES.items()]
    assert {rec['table'] for uc, k, N, P, rec in reps if rec['family'] == 'mfma' and rec['op'] == 3 and rec['publish_image']} == set(range(len(U.FUSED_ENVS)))
    for t, env in enumerate(U.FUSED_ENVS):
        assert {uc.env for uc, k, N, P, rec in reps if rec['family'] == 'mfma' and rec['table'] == t} == {env}
    assert any(rec['family'] == 'fused3' and rec['op'] == 1 and rec['cache_activations'] for uc, k, N, P, rec in reps)
    pts = set()
    for ph in ((32, 32), (100, 50, 25), (256, 128)):        # the sample tile of a generic product, from a product launched on its own on the same engine
        uc = next(uc for uc, k, N, P, rec in reps if rec['family'] == 'generic' and uc.ph == ph)
        d = U.case_data(uc, 33)
        eng = engine_for(uc, d)
        eng.fvp(batch_of(eng, d), d['v'])
        pts.add(eng.last_update_launch()['pt'])
    assert pts == {128, 64, 32}, pts
    gemm = {P for uc, k, N, P, rec in reps if rec['family'] == 'gemm' and rec['op'] == 1}
    assert any(p < 1024 for p in gemm), sorted(gemm)
    allP = {P for uc, k, N, P, rec in reps if rec['n_fvp'] >= 2}
    assert any(p <= 2048 for p in allP) and any(2048 < p <= 4096 for p in allP) and any(4096 < p <= 13312 for p in allP) and any(p > 13312 for p in allP), sorted(allP)
    assert all(rec['fused_tails'] for uc, k, N, P, rec in reps)
    if not _ROUTES:                                         # (test_routes_agree did not run in this process)
        uc = ROUTE_CASES[0]
        d = U.case_data(uc)
        eng = engine_for(uc, d)
        eng.set_policy(d['th'])
        update(eng, batch_of(eng, d), S.K_ALL, allreduce=lambda t: t)
        _ROUTES.append((uc, eng.last_solve_launch()))
        eng.set_policy(d['th'])
    assert any(not rec['fused_tails'] and rec['n_fvp'] == S.K_ALL for uc, rec in _ROUTES)
    print('reached:', json.dumps(sorted({(rec['family'], rec['op'], rec['table'], rec['n_fvp'], P) for uc, k, N, P, rec in reps})))
