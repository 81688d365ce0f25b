"""tests/dyn_act_cases.py held to its own promises, on the CPU and without the library: the table reaches every (entry point, fallback family, variant)
triple; the first layer is scaled as stated; the per-layer BPTT oracle agrees with central differences of its own cost and is, on relu nets, bit for bit
what it was; every kink guard replaces at most 5 % of a case; the float64 side passes every check at float64 rounding; and every mutation -- an activation
replaced, the order reversed, relu' in the adjoint of a tanh layer, tanh' left out -- misses the bound of every case it applies to, by the factor printed.

METRPO_TOL_REPORT=<file> (conftest.py) also makes this file write <file>.dyn_act_cases.json: mutation factors and kink shares per entry point
(profiles/r29_dyn_act.txt)."""
import json
import os

import numpy as np
import pytest

from oracle import metrpo_oracle as O
from oracle import bptt_oracle as Bp
from oracle import dynamics_oracle as D
import tolerances as TOL
import rollout_cases as RC
import rollout_check as CK
import bptt_cases as BC
import terminal_value_cases as TC
import disagreement_ref as DR
import dyn_bf16_ref as BF
import dyn_act_cases as DA

_FIG = {}                      # entry point -> dict(least factor by which a mutation misses, worst kink share, ...)


def _least(ep, name, factor):
    d = _FIG.setdefault(ep, {})
    d[name] = min(d.get(name, np.inf), float(factor))


def _most(ep, name, v):
    d = _FIG.setdefault(ep, {})
    d[name] = max(d.get(name, 0.0), float(v))


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    path = os.environ.get('METRPO_TOL_REPORT')
    if path:
        json.dump(_FIG, open(path + '.dyn_act_cases.json', 'w'), indent=1, sort_keys=True)
    for ep in sorted(_FIG):
        print(ep, {k: float('%.3g' % v) for k, v in sorted(_FIG[ep].items())})


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_entry_point_family_and_variant():
    got = DA.reached()
    want = set()
    for acts in DA.TWO:
        want |= {('rollout', 'thread-per-env', acts), ('rollout', 'tile-gemm', acts), ('step', 'thread-per-env', acts), ('step', 'tile-gemm', acts),
                 ('bptt_grad', 'generic-sweeps', acts), ('bptt_grad_stochastic', 'generic-sweeps', acts), ('validation_cost', 'generic-sweeps', acts),
                 ('dyn_eval_losses', 'tile-gemm', acts)}
    want |= {('rollout', 'tile-gemm', DA.THREE), ('dyn_eval_losses', 'tile-gemm', DA.THREE), ('svg_grad', 'generic', DA.THREE)}
    want |= {('rollout', 'skinny-split-reduce', a) for a in (('tanh', 'tanh'), ('relu', 'tanh'), ('relu', 'identity'))}      # act 2 and act 0 behind a split contraction
    want |= {('rollout', 'bf16-layer-gemm', a) for a in (('tanh', 'tanh'), ('tanh', 'relu'), ('relu', 'tanh'))}
    want |= {('svg_grad', 'generic', a) for a in (('identity', 'identity'), ('tanh', 'relu'), ('relu', 'tanh'))}
    want |= {('lbfgs_policy', 'generic-sweeps', ('tanh', 'tanh'))}
    want |= {('dyn_train_step', 'refused', a) for a in DA.TRAIN_REFUSED}
    for acts in DA.SUPPLIED_VARIANTS:
        want |= {('rollout_actions', 'step-loop', acts), ('model_error', 'step-loop', acts), ('ensemble_disagreement', 'generic', acts)}
        for ep in ('score_actions', 'score_policy_actions', 'score_actions_grad', 'score_policy_actions_grad'):
            want |= {(ep, 'generic', acts), (ep + '+terminal_value', 'generic', acts)}
    assert want <= got, sorted(want - got)
    assert set(DA.VARIANTS) == {v for _, _, v in got}
    # rollout: B = 1, 17, 65; all six modes at 17; a deterministic policy; chunks (2, 1)
    for name, acts in DA.ROLLOUTS:
        cs = DA.rollout_cases(name, acts)
        assert {c.B for c in cs} == {1, 17, 65} and {c.mode for c in cs if c.B == 17 and c.name == 'all-modes'} == set(O.SAM_MODES)
        assert all((c.T, c.H) == (3, 2) for c in cs) and any(c.determ for c in cs) and [c.chunks for c in cs if c.chunks] == [(2, 1)]
    # over a shape's variants the rotating cases meet several modes
    assert {c.mode for name, acts in DA.ROLLOUTS for c in DA.rollout_cases(name, acts) if c.B in (1, 65)} == set(O.SAM_MODES)
    assert {(c.B, c.T) for c in DA.BPTT_CASES} == {(1, 3), (17, 3), (65, 3), (17, 1)}
    assert {(c.env, c.dh) for c in DA.BPTT_CASES} == {('swimmer', (64, 64)), ('half_cheetah', (64, 64)), ('swimmer', (128, 128))}
    assert {(c.B, c.S, c.T) for c in DA.SUPPLIED_CASES} == {(17, 1, 3), (33, 3, 3)}
    assert all(DA.eval_rows(h) == ((1, 17, 129, 8193) if h == (64, 64) else (1, 17, 129)) for h, _ in DA.EVAL_NETS)


def test_the_dispatch_restated_for_the_rollout_shapes():
    """What the table's names promise of the library's rules: which hidden layers gemm_skinny_bias splits, and where the fused output tile may stand."""
    nin = lambda s: O.ENV_SPECS[s.env][0] + O.ENV_SPECS[s.env][1] - O.ENV_SPECS[s.env][2]
    for s in DA.SHAPES:
        for B in (1, 17, 65):
            sp = DA.hidden_splits(s.hidden, s.variants[0], nin(s), B, s.K)
            assert bool(sp) == (s.name in ('split-256x256', 'wide-512x512')), (s.name, B, sp)       # the smallest contraction that splits is 256
            if s.name == 'split-256x256':
                assert sp == [(1, 2)]
    s = DA.SHAPE['tile-128x128']
    assert DA.expect_launch(s, ('tanh', 'relu'), 17)['fuse_tile'] == 1 and DA.expect_launch(s, ('tanh', 'relu'), 17)['out_splits'] == 2
    for acts in (('relu', 'tanh'), ('relu', 'identity'), ('tanh', 'tanh')):
        e = DA.expect_launch(s, acts, 17)
        assert e['fuse_tile'] == 0 and e['out_splits'] == 0
    s = DA.SHAPE['tile-64x64-hc']
    assert DA.expect_launch(s, ('tanh', 'relu'), 65)['fuse_tile'] == 1 and DA.expect_launch(s, ('relu', 'tanh'), 65)['fuse_tile'] == 0
    assert DA.expect_launch(DA.SHAPE['split-256x256'], ('tanh', 'tanh'), 17)['out_splits'] == 2       # the output layer's own contraction of 256, added in k_big_post


@pytest.mark.parametrize('name,acts', DA.ROLLOUTS, ids=['%s-%s' % (n, DA.tag(a)) for n, a in DA.ROLLOUTS])
def test_first_layer_scale_of_the_rollout_problems(name, acts):
    p = DA.problem(name, acts)
    share = DA.near_share(p.dm, p.th, p.pdims, p.pool32)
    _least('first layer', 'least share of |z| in [0.5, 2]', share)
    assert share >= DA.MIN_NEAR_SHARE, share


def test_first_layer_scale_of_the_other_problems():
    probs = [DA.bptt_problem(c) for c in DA.BPTT_CASES] + [DA.eval_problem(h, a) for h, a in DA.EVAL_NETS] + \
            [DA.supplied_problem(e, K, a) for e, K in DA.SUPPLIED_NETS for a in DA.SUPPLIED_VARIANTS]
    for dm, th, pdims, pool in probs:
        share = DA.near_share(dm, th, pdims, pool)
        _least('first layer', 'least share of |z| in [0.5, 2]', share)
        assert share >= DA.MIN_NEAR_SHARE, share
    for hidden, acts in DA.EVAL_NETS:                                  # ... and on the validation rows themselves
        dm, th, pdims, pool = DA.eval_problem(hidden, acts)
        x, _ = DA.eval_data(dm, pool, 129)
        z = np.abs(((x - dm.in_mean) / dm.in_std)[:, dm.n_drop:] @ dm.Ws[0][0] + dm.bs[0][0])
        assert np.mean((z >= DA.NEAR[0]) & (z <= DA.NEAR[1])) >= 0.4


# ---- the per-layer BPTT oracle ---------------------------------------------------------------------------------------------------------------------------------
def _former_forward_cache(dm, k, s, a):
    """oracle/bptt_oracle.py's forward before it took per-layer activations (relu only), kept here to show that relu nets lose no bit."""
    xu = np.concatenate([s, a], axis=1)
    h = ((xu - dm.in_mean) / dm.in_std)[:, dm.n_drop:]
    hs = [h]
    L = len(dm.Ws)
    for l in range(L):
        h = h @ dm.Ws[l][k] + dm.bs[l][k]
        if l < L - 1:
            assert dm.acts[l] == 'relu'
            h = np.maximum(h, 0); hs.append(h)
    return dm.diff_mean[:dm.ns] + dm.diff_std[:dm.ns] * h + s, hs


def _former_vjp(dm, k, hs, g_next):
    ns, na = dm.ns, dm.na
    d = g_next * dm.diff_std[:ns]
    L = len(dm.Ws)
    for l in range(L - 1, -1, -1):
        d = d @ dm.Ws[l][k].T
        if l > 0:
            d = d * (hs[l] > 0)
    gxu = np.zeros((g_next.shape[0], ns + na), dtype=g_next.dtype)
    gxu[:, dm.n_drop:] = d
    gxu = gxu / dm.in_std
    return g_next + gxu[:, :ns], gxu[:, ns:]


@pytest.mark.parametrize('env,dh', [('swimmer', (64, 64)), ('ant', (16, 24, 8)), ('half_cheetah', (32, 32))])
def test_bptt_oracle_on_relu_nets_is_bit_for_bit_what_it_was(env, dh, monkeypatch):
    dm, theta, pdims, pool = DA.net_problem(env, 2, dh, ['relu'] * len(dh), seed=5)
    x0 = pool[:9]
    now = Bp.policy_costs_and_grad(dm, theta, pdims, env, x0, 4, 0.97)
    monkeypatch.setattr(Bp, '_dyn_forward_cache', _former_forward_cache)
    monkeypatch.setattr(Bp, '_dyn_vjp', _former_vjp)
    was = Bp.policy_costs_and_grad(dm, theta, pdims, env, x0, 4, 0.97)
    assert np.array_equal(now[0].view(np.uint64), was[0].view(np.uint64)) and np.array_equal(now[1].view(np.uint64), was[1].view(np.uint64))
    assert np.linalg.norm(now[1]) > 0


@pytest.mark.parametrize('acts', DA.VARIANTS, ids=DA.tag)
def test_bptt_oracle_matches_central_differences(acts):
    """The adjoint with relu' / 1 - h^2 / 1 per layer against central differences of the oracle's own float64 cost, along random directions and along single
    parameters of every variable; a wrong derivative in any layer is off by O(1) of the directional derivative."""
    dh = (10, 12) if len(acts) == 2 else (10, 12, 8)
    dm, theta, pdims, pool = DA.net_problem('swimmer', 2, dh, acts, seed=11)
    rng = np.random.RandomState(3)
    theta = theta + 0.05 * rng.randn(theta.size); theta[-dm.na:] = 0.0          # means inside the clip: the cost is smooth along the directions taken
    x0, T, gamma = pool[:6], 3, 0.97
    f = lambda th: float(np.mean(Bp.policy_costs_and_grad(dm, th, pdims, 'swimmer', x0, T, gamma)[0]))
    g = Bp.policy_costs_and_grad(dm, theta, pdims, 'swimmer', x0, T, gamma)[1]
    assert np.all(g[-dm.na:] == 0.0) and np.linalg.norm(g) > 0
    h = 1e-5
    worst = 0.0
    for i in range(8):
        v = rng.randn(theta.size); v[-dm.na:] = 0.0
        if i >= 4:                                                     # a single variable at a time
            name, sl = BC.blocks(pdims)[i - 4]
            m = np.zeros(theta.size); m[sl] = 1.0; v = v * m
        v /= np.linalg.norm(v)
        fd = (f(theta + h * v) - f(theta - h * v)) / (2 * h)
        worst = max(worst, abs(fd - g @ v) / max(abs(fd), 1e-12))
    _most('bptt oracle', 'worst relative distance from central differences', worst)
    assert worst < 1e-6, worst
    for kind in DA.adjoint_mutations(acts):                            # ... and the check sees the two wrong adjoints
        with DA.adjoint_mutation(kind):
            gm = Bp.policy_costs_and_grad(dm, theta, pdims, 'swimmer', x0, T, gamma)[1]
        assert np.linalg.norm(gm - g) > 1e-3 * np.linalg.norm(g), kind


# ---- rollout and step ---------------------------------------------------------------------------------------------------------------------------------------------
def _passes(p, c, dev):
    try:
        DA.check_rollout(p, c, dev, 'cpu')
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize('name,acts', DA.ROLLOUTS, ids=['%s-%s' % (n, DA.tag(a)) for n, a in DA.ROLLOUTS])
def test_rollout_check_passes_float64_and_fails_every_mutation(name, acts):
    p = DA.problem(name, acts)
    cs = DA.rollout_cases(name, acts)
    CK.REPORT.clear()
    for c in cs:
        dr = p.draws(c)[0]
        DA.check_rollout(p, c, RC.reference(p, dr, c.B, c.T, c.H, c.mode, c.determ), 'float64 %s' % c.name, form='cpu')
    assert max(CK.REPORT.values()) < 1e-6, CK.REPORT
    if p.env == 'ant':
        early = sum(int((r['done'] & (r['tpath'] < c.H - 1)).sum()) for c in cs for r in [RC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ)])
        assert early > 0
    dm = p.dm
    try:
        for mut, wrong in DA.mutations(p.acts):
            p.dm = DA.with_acts(dm, wrong)
            devs = [RC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ) for c in cs]
            p.dm = dm
            for c, dev in zip(cs, devs):
                ok = RC.reference(p, p.draws(c)[0], c.B, c.T, c.H, c.mode, c.determ)
                factor = float((np.abs(dev['next'][0] - ok['next'][0]) / (p.tol['atol'] + p.tol['rtol'] * np.abs(ok['next'][0]))).max())      # step 0: the same state
                _least('rollout', mut, factor)
                assert factor > 1.0 and not _passes(p, c, dev), (mut, c, factor)
    finally:
        p.dm = dm


@pytest.mark.parametrize('name', DA.STEP_SHAPES)
@pytest.mark.parametrize('acts', DA.TWO, ids=DA.tag)
def test_step_reference_fails_every_mutation(name, acts):
    p = DA.problem(name, acts)
    rng = np.random.RandomState(17)
    B = 17
    s, a = p.pool32[:B], RC.f32(0.8 * rng.randn(B, p.dm.na))
    idx, noise = rng.randint(p.K, size=B), RC.f32(rng.randn(B, p.dm.ns))
    dm = p.dm
    for mode in O.SAM_MODES:
        ok = DA.step_ref(p, s, a, mode, idx, noise)[0]
        for mut, wrong in DA.mutations(acts):
            p.dm = DA.with_acts(dm, wrong)
            try:
                bad = DA.step_ref(p, s, a, mode, idx, noise)[0]
            finally:
                p.dm = dm
            factor = float((np.abs(bad - ok) / (p.tol['atol'] + p.tol['rtol'] * np.abs(ok))).max())
            _least('step', mut, factor)
            assert factor > 1.0, (mode, mut, factor)


@pytest.mark.parametrize('acts', DA.BF16_VARIANTS, ids=DA.tag)
def test_bf16_measured_bound_separates_the_activations(acts):
    """dyn_bf16_ref.random_bound under `acts` (8 x the float32 emulation's distance from the rounded float64 restatement): the restatement of the same
    weights under any mutated activation lies beyond it on every head."""
    bound, fig, (dm, s, ac), ref = BF.random_bound(DA.BF16_HIDDEN, acts)
    assert 0 < fig and bound == BF.BOUND_FACTOR * fig
    print('bf16 %s: emulation %.3e, bound %.3e' % (DA.tag(acts), fig, bound))
    for mut, wrong in DA.mutations(acts):
        rel = BF.rel_l2_per_head(BF.ref_delta(DA.with_acts(dm, wrong), s, ac), ref)
        _least('rollout bf16', mut, rel.min() / bound)
        assert rel.min() > bound, (mut, rel, bound)


# ---- BPTT -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DA.BPTT_CASES, ids=[c.id for c in DA.BPTT_CASES])
def test_bptt_cases_kinks_restatement_and_mutations(case):
    d = DA.bptt_data(case)
    assert d['accepted'] == case.B and d['replaced'] <= DA.MAX_REPLACED * case.B and d['margin'] >= BC.KINK_FACTOR, (d['replaced'], d['margin'])
    _most('bptt', 'worst replaced share', d['replaced'] / float(case.B))
    rc, rg = DA.bptt_reference(d)
    assert np.linalg.norm(rg) > 0
    # the restated walk (tests/bptt_cases.py, generalised with the oracle) in float64 reproduces the reference; in float32 it uses a small share of the bounds
    w64 = BC.walk(d['dm'], d['th'], d['pdims'], case.env, d['x0'], case.T, case.gamma, d['eps'], np.float64)
    assert max(DA.bptt_shares(w64['costs'], w64['grad'], d)[:3]) < 1e-6
    w32 = BC.walk(d['dm'], d['th'], d['pdims'], case.env, d['x0'], case.T, case.gamma, d['eps'], np.float32)
    s32 = DA.bptt_shares(w32['costs'], w32['grad'], d)
    _most('bptt', 'float32 NumPy restatement, worst share of a bound', max(s32[:3]))
    assert max(s32[:3]) <= 1.0, s32
    for mut, wrong in DA.mutations(case.acts):
        mc, mg = DA.bptt_reference(d, DA.with_acts(d['dm'], wrong))
        cost, whole, worst, _ = DA.bptt_shares(mc, mg, d)
        _least('bptt cost', mut, cost); _least('bptt grad', mut, whole)
        assert cost > 1.0 and whole > 1.0 and worst > 1.0, (mut, cost, whole, worst)
    if not case.stoch:                                                 # (the stochastic reference is torch autograd: it has no hand-written adjoint to get wrong)
        for kind in DA.adjoint_mutations(case.acts):
            with DA.adjoint_mutation(kind):
                mc, mg = Bp.policy_costs_and_grad(d['dm'], d['th'], d['pdims'], case.env, d['x0'], case.T, case.gamma)
            cost, whole, worst, _ = DA.bptt_shares(mc, mg, d)
            _least('bptt grad', kind, whole)
            assert cost == 0.0 and whole > 1.0 and worst > 1.0, (kind, cost, whole, worst)


# ---- SVG --------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', DA.SVG_NETS, ids=['%s-%s' % (n[0], DA.tag(n[3])) for n in DA.SVG_NETS])
def test_svg_cases_kinks_and_mutations(net):
    d = DA.svg_data(*net)
    n_draws = DA.SVG_N + d['replaced']
    _most('svg', 'worst replaced share', d['replaced'] / float(n_draws))
    assert d['replaced'] <= DA.MAX_REPLACED * n_draws and d['margin'] >= DA.SV.KINK_FACTOR, (d['replaced'], d['margin'])
    assert DA.near_share(d['dm'], d['theta'], d['pdims'], d['obs'].reshape(-1, d['dm'].ns)) >= 0.4
    ref = DA.svg_reference(d)
    assert max(DA.svg_shares(ref, d)) == 0.0
    for mut, wrong in DA.mutations(net[3]):
        s = DA.svg_shares(DA.svg_reference(d, DA.with_acts(d['dm'], wrong)), d)
        _least('svg', mut, s[0])
        assert s[0] > 1.0 and s[2] > 1.0, (mut, s)
    for kind in DA.adjoint_mutations(net[3]):
        with DA.adjoint_mutation(kind):
            s = DA.svg_shares(DA.svg_reference(d, d['dm']), d)
        _least('svg', kind, s[0])
        assert s[0] > 1.0 and s[2] > 1.0, (kind, s)


# ---- validation losses ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden,acts', DA.EVAL_NETS, ids=['%s-%s' % ('x'.join(map(str, h)), DA.tag(a)) for h, a in DA.EVAL_NETS])
def test_validation_losses_fail_every_mutation(hidden, acts):
    dm, th, pdims, pool = DA.eval_problem(hidden, acts)
    for n in DA.eval_rows(hidden):
        x, y = DA.eval_data(dm, pool, n)
        for reg in DA.EVAL_REGS:
            ref = D.validation_losses(dm, x, y, reg)
            for mut, wrong in DA.mutations(acts):
                factor = DA.loss_share(D.validation_losses(DA.with_acts(dm, wrong), x, y, reg), ref)
                _least('dyn_eval_losses', mut, factor)
                assert factor > 1.0, (n, reg, mut, factor)


# ---- the supplied-action family ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,loop', DA.SUPPLIED_RUNS, ids=['%s-%s' % (c.id, l) for c, l in DA.SUPPLIED_RUNS])
def test_scoring_cases_kinks_and_mutations(case, loop):
    d = DA.supplied_data(case, loop)
    assert tuple(d['dm'].acts) == case.act
    assert d['accepted'] == case.B and d['replaced'] <= DA.MAX_REPLACED * case.B and d['margin'] >= TC.KINK_FACTOR, (d['replaced'], d['margin'])
    _most('scoring', 'worst replaced share', d['replaced'] / float(case.B))
    ref = TC.reference(d)
    plain = TC.walk(d, tv=None)
    assert max(TC.shares(ref, ref, case)) == 0.0
    dm = d['dm']
    try:
        for mut, wrong in DA.mutations(case.act):
            d['dm'] = DA.with_acts(dm, wrong)
            use = TC.shares(TC.walk(d), ref, case)
            use0 = TC.GC.shares(TC.walk(d, tv=None), plain, case)                # ... and without a terminal value, on tests/score_grad_cases.py's bounds
            _least('scoring ret', mut, min(use[5], use0[5])); _least('scoring grad', mut, min(use[0], use0[0]))
            assert use[0] > 1.0 and use[3] > 1.0 and use[5] > 1.0 and use0[0] > 1.0 and use0[5] > 1.0, (mut, use, use0)
        d['dm'] = dm
        for kind in DA.adjoint_mutations(case.act):
            with DA.adjoint_mutation(kind):
                use = TC.shares(TC.walk(d), ref, case)
            _least('scoring grad', kind, use[0])
            assert use[0] > 1.0 and use[3] > 1.0 and use[5] == 0.0, (kind, use)
    finally:
        d['dm'] = dm
    # the relu twin of the same weights is another function: what the GPU test's "differs from the forced-generic relu twin" rests on
    d['dm'] = DA.relu_twin(dm)
    try:
        assert TC.shares(TC.walk(d), ref, case)[5] > 1.0
    finally:
        d['dm'] = dm


@pytest.mark.parametrize('env,K', DA.SUPPLIED_NETS)
@pytest.mark.parametrize('acts', DA.SUPPLIED_VARIANTS, ids=DA.tag)
def test_rollout_actions_and_disagreement_fail_every_mutation(env, K, acts):
    dm, th, pdims, pool = DA.supplied_problem(env, K, acts)
    rng = np.random.RandomState(23)
    B, T = 17, DA.SUPPLIED_T
    init, actions = pool[:B], RC.f32(1.5 * rng.randn(T, B, dm.na))
    heads = rng.randint(K, size=B)
    ok = DA.rollout_actions_ref(dm, env, init, actions, 'model_mean')
    okd = DR.disagreement(dm, env, init, actions[0])
    for mut, wrong in DA.mutations(acts):
        bad = DA.rollout_actions_ref(DA.with_acts(dm, wrong), env, init, actions, 'model_mean')
        factor = float((np.abs(bad['obs'][1] - ok['obs'][1]) / (TOL.FREE_RUN['atol'] + TOL.FREE_RUN['rtol'] * np.abs(ok['obs'][1]))).max())
        _least('rollout_actions', mut, factor)
        sh = DR.shares(DR.disagreement(DA.with_acts(dm, wrong), env, init, actions[0]), okd, TOL.STEP)
        _least('ensemble_disagreement', mut, sh['next_all'])
        assert factor > 1.0 and sh['next_all'] > 1.0 and sh['mean'] > 1.0, (mut, factor, sh)
    # eps_rand with a head per env equals the per-head forward (the restatement of tests/rollout_actions_ref.py)
    import rollout_actions_ref as RA
    a = DA.rollout_actions_ref(dm, env, init, actions, 'eps_rand', model=heads)
    b = RA.rollout_actions(dm, env, init, actions, model=heads)
    assert np.array_equal(a['obs'], b['obs']) and np.array_equal(a['rew'], b['rew'])
