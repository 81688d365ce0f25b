"""GPU tests of the terminal value's MLP form (metrpo_set_terminal_value_mlp; csrc/sact_sum.h: TermVal's mlp_*, and the four score_*.hip files):
metrpo_score_actions, metrpo_score_actions_grad, metrpo_score_policy_actions and metrpo_score_policy_actions_grad with a net set, against the float64
restatement tests/terminal_mlp_ref.py on the cases of tests/terminal_mlp_cases.py (drawn clear of every relu / clip / cost / done kink and of the
value's own clip), between the calls, across chunkings, against the quadratic form where the two coincide, and against the calls with no value set.

Bounds, all from tests/tolerances.py, none new (tests/terminal_mlp_cases.py states them): grad, lam0 per head rel-L2 <= BPTT_GRAD_REL_L2 and per step
and per candidate by block_bound; ret by the per-step REWARD / LONG_RUN rows with one more term for the value; len exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import tolerances as TOL
import terminal_mlp_cases as MC
import terminal_mlp_ref as R

pytestmark = pytest.mark.gpu

GRAD_WANT = {'open': ('grad', 'ret', 'len', 'grad_mean', 'lam0'), 'closed': ('grad', 'ret', 'len', 'grad_mean', 'lam0', 'act_out')}
SCORE_WANT = {'open': ('ret', 'len', 'ret_mean', 'ret_std'), 'closed': ('ret', 'len', 'ret_mean', 'ret_std', 'act_out')}


def cpu(t):
    return t.detach().cpu().numpy()


_engines = {}


def engine(case):
    key = MC.shape_key(case)
    if key not in _engines:
        dm, theta, _, _ = MC.problem(case)
        _engines[key] = Hh.engine_of(case.env, case.K, case.dh, (32, 32), dm, theta, dyn_act=case.act)
    return _engines[key]


def fused_shape(case):
    return case.env in MC.FUSED_ENVS and len(case.dh) == 2 and max(case.dh) <= 64 and case.act == 'relu'


def call(d, which, chunk=0, force=None):
    """One of the four calls on a case's data, with whatever terminal value the engine holds: which = 'score' or 'grad'."""
    case, loop = d['case'], d['loop']
    eng = engine(case)
    force = (case.path == 'generic') if force is None else force
    init = np.asarray(d['init'], np.float32)
    seq = None if d['seq'] is None else torch.as_tensor(d['seq'], dtype=torch.float32, device=eng.device)
    kw = dict(gamma=case.gamma, stop_at_done=case.stop, force_generic=force)
    if loop == 'open':
        if which == 'score':
            out, kern = eng.score_actions(init, seq, want=SCORE_WANT[loop], **kw), eng.last_score_actions_kernel()
        else:
            out, kern = eng.score_actions_grad(init, seq, want=GRAD_WANT[loop], chunk=chunk, **kw), eng.last_score_actions_grad_kernel()
    else:
        kw.update(T=case.T, noise_in_std=case.in_std)
        if which == 'score':
            out, kern = eng.score_policy_actions(init, seq, want=SCORE_WANT[loop], **kw), eng.last_score_policy_actions_kernel()
        else:
            out, kern = eng.score_policy_actions_grad(init, seq, want=GRAD_WANT[loop], chunk=chunk, **kw), eng.last_score_policy_actions_grad_kernel()
    assert kern == ('fused' if (fused_shape(case) and not force) else 'generic')
    return {k: cpu(v) for k, v in out.items()}


class net_set(object):
    """with net_set(d): the case's net is set on its engine, and cleared behind the block whatever happens in it"""

    def __init__(self, d, tv=None):
        self.eng, self.tv, self.hid = engine(d['case']), d['tv'] if tv is None else tv, d['case'].hid

    def __enter__(self):
        self.eng.set_terminal_value_mlp(R.pack(self.tv), self.hid, self.tv[6])
        assert self.eng.terminal_value == len(self.tv[6]) and self.eng.terminal_value_kind == 2
        return self.eng

    def __exit__(self, *exc):
        self.eng.clear_terminal_value()
        assert self.eng.terminal_value == 0 and self.eng.terminal_value_kind == 0


def same(a, b, names=None):
    for w in (names or a.keys()):
        assert np.array_equal(a[w], b[w]), w


# ---- 1. all four calls on either path against the restatement, and against each other ---------------------------------------------------------------
@pytest.mark.parametrize('case,loop', MC.RUNS, ids=MC.RUN_IDS)
def test_against_the_restatement(case, loop):
    d = MC.case_data(case, loop)
    assert d['accepted'] == case.B
    ref = MC.reference(d)
    unset = call(d, 'grad')
    with net_set(d):
        got = call(d, 'grad')
        again = call(d, 'grad')
        score = call(d, 'score') if case.calls == 'all' else None
        score_again = call(d, 'score') if case.calls == 'all' else None
    K, T, B = case.K, case.T, case.B
    dm = d['dm']
    assert got['grad'].shape == (K, T, B, dm.na) and got['lam0'].shape == (K, B, dm.ns) and got['ret'].shape == (K, B)
    use = MC.shares(got, ref, case)
    print("%s %s: grad %.3g whole, %.3g per step, %.3g per candidate; lam0 %.3g whole, %.3g per candidate; ret %.3g of their bounds" %
          ((case.id, loop) + tuple(use)))
    assert np.array_equal(got['len'], ref['len']) and np.array_equal(got['len'], unset['len'])       # len is unchanged by the value
    assert use.max() <= 1.0, use
    gm_use = max(MC.GC.grad_use(got['grad_mean'], ref['grad_mean'], TOL.BPTT_GRAD_REL_L2))
    assert gm_use <= 1.0, gm_use
    same(got, again)                                                                                 # repeated calls are bit-identical
    if loop == 'closed':
        assert np.array_equal(got['act_out'], unset['act_out'])                                      # the value moves no action
    if score is not None:
        same(score, score_again)
        same(score, got, [w for w in ('ret', 'len', 'act_out') if w in score])                       # the gradient call carries the scoring call's bits
        suse = MC.shares(dict(ret=score['ret']), ref, case)
        assert suse.max() <= 1.0, suse
        mean = ref['ret'].sum(axis=0) / K
        assert np.allclose(score['ret_mean'], mean, rtol=1e-4, atol=float(MC.ret_bound(ref, case).max()))
    # the value reaches the outputs: a candidate that is still alive at T has another return than without it
    alive = ref['wT'] != 0
    if alive.any():
        assert np.any(got['ret'][alive] != unset['ret'][alive])
    assert np.array_equal(got['ret'][~alive], unset['ret'][~alive])                                  # no bootstrap behind a done: bit for bit
    if case.path == 'generic' and fused_shape(case) and case.T == 11:                                # the two device paths against each other
        with net_set(d):
            fused = call(d, 'grad', force=False)
        assert np.array_equal(fused['len'], got['len'])
        assert MC.shares(fused, ref, case).max() <= 1.0


# ---- 2. chunking changes no bit -----------------------------------------------------------------------------------------------------------------------
_CHUNKED = [(c, l) for c, l in MC.RUNS if c.B == 33 and c.T == 11 and c.env in ('swimmer', 'ant', 'hopper')]


@pytest.mark.parametrize('case,loop', _CHUNKED, ids=['%s-%s' % (c.id, l) for c, l in _CHUNKED])
def test_chunked_calls_equal_the_unchunked_call(case, loop):
    d = MC.case_data(case, loop)
    with net_set(d):
        whole = call(d, 'grad')
        for chunk in (16, 17):
            same(whole, call(d, 'grad', chunk=chunk))


@pytest.mark.parametrize('case', [c for c in MC.CASES if c.path == 'generic' and (c.B, c.T, c.S, c.nb) == (33, 11, 3, 3) and c.env in ('swimmer', 'ant', 'hopper')],
                         ids=lambda c: c.id)
def test_chunked_generic_scoring_equals_the_unchunked_call(case):
    """metrpo_score_policy_actions' generic path under metrpo_debug_score_policy_chunk: chunks that start at c0 > 0 and a ragged last chunk
    (k_sact_reduce<MLP> reads s_T from the last step's s_out at the chunk's own row stride, the bias row is (c0 + i) / per)."""
    from metrpo_amd import _lib
    d = MC.case_data(case, 'closed')
    eng = engine(case)
    try:
        with net_set(d):
            whole = call(d, 'score')
            for cap in (16, 17, 5):
                assert _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, cap) == 0
                same(whole, call(d, 'score'))
                assert _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, 0) == 0
    finally:
        _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, 0)
    ref = MC.reference(d)
    assert MC.shares(dict(ret=whole['ret']), ref, case).max() <= 1.0 and np.array_equal(whole['len'], ref['len'])


# ---- 3. where the two forms coincide; replacing one by the other; clearing ----------------------------------------------------------------------------------
_T11 = [(c, l) for c, l in MC.RUNS if c.T == 11 and c.env in ('swimmer', 'ant') and c.S == 3]


@pytest.mark.parametrize('case,loop', _T11, ids=['%s-%s' % (c.id, l) for c, l in _T11])
def test_a_net_with_a_zero_head_is_the_quadratic_value_with_zero_weights(case, loop):
    """W2 = 0, b2 = 0: V = bias_row + (0 + sum_j 0 p1_j) = bias_row exactly, and dV/ds = 0; the quadratic form with w1 = w2 = 0 is bias_row exactly too."""
    d = MC.case_data(case, loop)
    ns, eng = d['dm'].ns, engine(case)
    tv = d['tv']
    zero_head = tv[:4] + (np.zeros_like(tv[4]), np.zeros_like(tv[5]), tv[6])
    with net_set(d, zero_head):
        mlp = {w: call(d, w) for w in ('score', 'grad')}
    eng.set_terminal_value(np.zeros(ns), np.zeros(ns), tv[6])
    try:
        assert eng.terminal_value_kind == 1
        quad = {w: call(d, w) for w in ('score', 'grad')}
    finally:
        eng.clear_terminal_value()
    for w in ('score', 'grad'):
        same(quad[w], mlp[w])
    unset = call(d, 'grad')
    alive = MC.reference(d)['wT'] != 0
    if alive.any():
        assert np.any(mlp['grad']['ret'][alive] != unset['ret'][alive])                              # the bias is there


@pytest.mark.parametrize('case,loop', _T11, ids=['%s-%s' % (c.id, l) for c, l in _T11])
def test_either_form_replaces_the_other_and_clearing_gives_the_unset_outputs(case, loop):
    d = MC.case_data(case, loop)
    ns, eng, tv = d['dm'].ns, engine(case), d['tv']
    rng = np.random.RandomState(7)
    quad = (MC.f32(0.5 * rng.randn(ns)), MC.f32(0.1 * rng.randn(ns)), tv[6])
    before = {w: call(d, w) for w in ('score', 'grad')}
    assert (eng.terminal_value_kind, eng.terminal_value) == (0, 0)
    try:
        eng.set_terminal_value(*quad)
        assert (eng.terminal_value_kind, eng.terminal_value) == (1, case.nb)
        q1 = call(d, 'grad')
        eng.set_terminal_value_mlp(R.pack(tv), case.hid, tv[6])                                        # the net replaces the quadratic
        assert (eng.terminal_value_kind, eng.terminal_value) == (2, case.nb)
        m1 = {w: call(d, w) for w in ('score', 'grad')}
        eng.set_terminal_value(*quad)                                                                  # ... and the reverse
        assert (eng.terminal_value_kind, eng.terminal_value) == (1, case.nb)
        q2 = call(d, 'grad')
        eng.set_terminal_value_mlp(R.pack(tv), case.hid, tv[6])
    finally:
        eng.clear_terminal_value()
    assert (eng.terminal_value_kind, eng.terminal_value) == (0, 0)
    after = {w: call(d, w) for w in ('score', 'grad')}                                               # behind metrpo_clear_terminal_value
    same(q1, q2)
    with net_set(d):
        m2 = {w: call(d, w) for w in ('score', 'grad')}
    for w in ('score', 'grad'):
        same(m1[w], m2[w])
        same(before[w], after[w])
    assert not np.array_equal(m1['grad']['ret'], before['grad']['ret']) and not np.array_equal(m1['grad']['ret'], q1['ret'])
    assert MC.shares(m1['grad'], MC.reference(d), case).max() <= 1.0


# ---- 4. every other entry point ignores the value ----------------------------------------------------------------------------------------------------------
def test_other_entry_points_ignore_the_net():
    case = next(c for c in MC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.B == 33 and c.T == 11 and c.stop)
    d = MC.case_data(case, 'open')
    eng = engine(case)
    dm, _, _, pool = MC.problem(case)
    init = np.asarray(pool[:33], np.float32)
    acts = torch.as_tensor(d['seq'], dtype=torch.float32, device=eng.device)
    theta0 = eng.get_policy().clone()
    rng = np.random.RandomState(1)
    B, T, H = 64, 6, 3
    eps = rng.randn(T, B, dm.na); midx = rng.randint(dm.K, size=(T, B)); ridx = rng.randint(len(pool), size=(T + 1, B)); rmod = rng.randint(dm.K, size=(T + 1, B))

    def others():
        eng.set_policy(theta0)
        traj = eng.rollout(B, T, H, 'step_rand', pool, eps=eps, model_idx=midx, reset_idx=ridx, reset_model=rmod)
        ra = eng.rollout_actions(init, acts, 'model_mean')
        vc = eng.validation_cost(init, 5, 0.99)
        costs, grad = eng.bptt_grad(init, 5, 0.99)
        adv, ret, valid, stats = eng.gae(traj, None, 0.99, 0.95)
        eng.center_advantages(adv, valid, stats)
        batch = eng.make_batch(traj.obs, traj.act, adv, traj.mean, eng.get_policy()[-dm.na:], valid=valid)
        out = eng.trpo_update(batch)
        res = [cpu(t) for t in [traj.obs, traj.act, traj.rew] + list(ra) + [vc, costs, grad, eng.get_policy()]]
        return res + [np.asarray([out['loss_before'], out['loss'], out['kl']], np.float64)]

    try:
        before = others()
        with net_set(d, d['tv'][:6] + (d['tv'][6][:1],)):
            during = others()
    finally:
        eng.set_policy(theta0)
    for a, b in zip(before, during):
        assert np.array_equal(a, b)


# ---- 5. the ABI's status codes --------------------------------------------------------------------------------------------------------------------------------
def test_status_codes():
    from metrpo_amd import _lib
    lib = _lib.lib
    case = next(c for c in MC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.K == 5)
    eng, dm = engine(case), MC.problem(case)[0]
    dev = eng.device
    ns, na, K = dm.ns, dm.na, dm.K
    h1, h2 = 17, 5
    par = torch.zeros(ns * h1 + h1 + h1 * h2 + 2 * h2 + 1, device=dev); bias = torch.ones(3, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = eng._stream()
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_set_terminal_value_mlp(None, p(par), h1, h2, p(bias), 1, st) == -2              # METRPO_ENULL
    assert lib.metrpo_terminal_value_kind(None) == -2
    for args in ((None, p(bias)), (p(par), None)):
        assert lib.metrpo_set_terminal_value_mlp(eng._ctx, args[0], h1, h2, args[1], 1, st) == -2 and b'set_terminal_value_mlp: NULL pointer' in err()
    for bad in ((0, 5), (33, 5), (17, 0), (17, 33), (-1, -1)):
        assert lib.metrpo_set_terminal_value_mlp(eng._ctx, p(par), bad[0], bad[1], p(bias), 1, st) == -1 and b'hidden widths' in err()      # METRPO_EINVAL
    for bad in (0, -1):
        assert lib.metrpo_set_terminal_value_mlp(eng._ctx, p(par), h1, h2, p(bias), bad, st) == -1 and b'n_bias' in err()
    assert eng.terminal_value == 0 and eng.terminal_value_kind == 0
    # a net with three biases: a scoring call whose S is not 3 returns METRPO_EINVAL and writes nothing; S = 3, and n_bias = 1 with any S, run
    assert lib.metrpo_set_terminal_value_mlp(eng._ctx, p(par), h1, h2, p(bias), 3, st) == 0 and eng.terminal_value == 3 and eng.terminal_value_kind == 2
    B, T = 6, 2
    init, seq = torch.zeros(3, ns, device=dev), torch.zeros(T, B, na, device=dev)
    ret = torch.full((K, B), 555.0, device=dev); grad = torch.full((K, T, B, na), 555.0, device=dev)

    def calls(S):
        a = _lib.ScoreActionsArgs(); a.B, a.T, a.S, a.stop_at_done, a.gamma = B, T, S, 1, 0.99
        a.d_init_obs, a.d_actions, a.d_ret = init.data_ptr(), seq.data_ptr(), ret.data_ptr()
        g = _lib.ScoreActionsGradArgs(); g.B, g.T, g.S, g.stop_at_done, g.gamma = B, T, S, 1, 0.99
        g.d_init_obs, g.d_actions, g.d_grad, g.d_ret = init.data_ptr(), seq.data_ptr(), grad.data_ptr(), ret.data_ptr()
        pa = _lib.ScorePolicyActionsArgs(); pa.B, pa.T, pa.S, pa.stop_at_done, pa.gamma = B, T, S, 1, 0.99
        pa.d_init_obs, pa.d_noise, pa.d_ret = init.data_ptr(), seq.data_ptr(), ret.data_ptr()
        pg = _lib.ScorePolicyActionsGradArgs(); pg.B, pg.T, pg.S, pg.stop_at_done, pg.gamma = B, T, S, 1, 0.99
        pg.d_init_obs, pg.d_noise, pg.d_grad, pg.d_ret = init.data_ptr(), seq.data_ptr(), grad.data_ptr(), ret.data_ptr()
        return [lib.metrpo_score_actions(eng._ctx, C.byref(a), st), lib.metrpo_score_actions_grad(eng._ctx, C.byref(g), st),
                lib.metrpo_score_policy_actions(eng._ctx, C.byref(pa), st), lib.metrpo_score_policy_actions_grad(eng._ctx, C.byref(pg), st)]

    try:
        for S in (1, 2, 6):
            assert calls(S) == [-1] * 4 and b'n_bias = 3, neither 1 nor S' in err()
        torch.cuda.synchronize()
        assert torch.all(ret == 555.0) and torch.all(grad == 555.0)
        assert calls(3) == [0] * 4
        assert lib.metrpo_set_terminal_value_mlp(eng._ctx, p(par), h1, h2, p(bias), 1, st) == 0 and eng.terminal_value == 1
        for S in (1, 2, 3, 6):
            assert calls(S) == [0] * 4
        torch.cuda.synchronize()
        assert not torch.any(ret == 555.0) and not torch.any(grad == 555.0)
    finally:
        assert lib.metrpo_clear_terminal_value(eng._ctx) == 0
    assert eng.terminal_value == 0 and eng.terminal_value_kind == 0 and calls(2) == [0] * 4
    # the host method: a scalar bias, a vector, and the shapes it refuses
    eng.set_terminal_value_mlp(np.zeros(par.numel()), (h1, h2))
    assert eng.terminal_value == 1 and eng.terminal_value_kind == 2
    eng.set_terminal_value_mlp(torch.zeros(par.numel(), dtype=torch.float64), (h1, h2), np.arange(4.0))
    assert eng.terminal_value == 4
    with pytest.raises(AssertionError, match='expected shape'):
        eng.set_terminal_value_mlp(np.zeros(par.numel() + 1), (h1, h2))
    eng.clear_terminal_value()
    assert eng.terminal_value == 0


# ---- 6. the controller sets and clears around a plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy_prior', [False, True], ids=['actions', 'noise'])
def test_shooting_controller_plans_with_the_net_behind_the_horizon(policy_prior, monkeypatch):
    from metrpo_amd import planning as P
    case = next(c for c in MC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.K == 5)
    eng, (dm, _, _, pool) = engine(case), MC.problem(case)
    S, H = 3, 4
    net = P.ValueMLP(dm.ns, (17, 5), generator=torch.Generator().manual_seed(5))
    net.W2 = 4.0 * net.W2
    during = []
    real_score = eng.score_policy_actions if policy_prior else eng.score_actions

    def score(*a, **kw):
        during.append((eng.terminal_value_kind, eng.terminal_value))
        return real_score(*a, **kw)
    monkeypatch.setattr(eng, 'score_policy_actions' if policy_prior else 'score_actions', score)
    gen = lambda: torch.Generator(device=eng.device).manual_seed(0)
    ctl = P.ShootingController(eng, H, 16, 4, 2, gamma=0.99, generator=gen(), terminal_value=net, policy_prior=policy_prior, init_std=0.5)
    obs = np.asarray(pool[:S], np.float32)
    a0, _ = ctl.get_actions(obs)
    assert eng.terminal_value == 0 and eng.terminal_value_kind == 0 and during and all(k == (2, 1) for k in during)      # set for every scoring call, cleared behind
    assert a0.shape == (S, dm.na) and np.isfinite(a0).all()
    net.bias = np.array([0.5, -1.0, 2.0])                                                              # a bias per env, the caller's
    n = len(during)
    ctl.get_actions(obs)
    assert all(k == (2, S) for k in during[n:]) and eng.terminal_value == 0
    net.bias = 0.0
    # the value is part of what the plan maximises: the same draws without it score differently
    plain = P.ShootingController(eng, H, 16, 4, 2, gamma=0.99, generator=gen(), policy_prior=policy_prior, init_std=0.5)
    with_tv = P.ShootingController(eng, H, 16, 4, 2, gamma=0.99, generator=gen(), terminal_value=net, policy_prior=policy_prior, init_std=0.5)
    plain.get_actions(obs); with_tv.get_actions(obs)
    assert not torch.equal(plain.last_plan['best_score'], with_tv.last_plan['best_score'])
    assert eng.terminal_value == 0
