"""GPU tests of metrpo_score_policy_actions (csrc/score_policy_actions.hip): the discounted return every head predicts for candidate NOISE sequences
around the policy, against the float64 restatement tests/score_policy_ref.py, against the device's own open-loop scorer fed the actions the call took
(d_act_out), against the device's policy forward along the replayed trajectories, between its two paths, against the device's validation cost, and
under the noise-space planner of metrpo_amd.planning.

Bounds, all from tests/tolerances.py, none new: a return's bound is the sum of its rewards' bounds, sum_t gamma^t (row(t).atol + row(t).rtol |r_t^ref|)
with row = REWARD for steps t <= 10 and LONG_RUN beyond, CROSS_KERNEL between the two device paths at T <= 10 (tests/test_gpu_score_actions.py's
rules); ret_mean and ret_std are held to the largest head's bound of the candidate; ACTION for an action against the device's own policy forward.
tests/test_score_policy_ref.py shows on the CPU that every case here is fit: the fp32 restatement agrees on len and uses at most 0.022 of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import tolerances as TOL
import score_actions_ref as SA
import score_policy_ref as SP

pytestmark = pytest.mark.gpu
WANT = ('ret', 'len', 'ret_mean', 'ret_std')
WANT_ACT = WANT + ('act_out',)


def cpu(t):
    return t.detach().cpu().numpy()


def reward_row(t):
    return TOL.REWARD if t <= 10 else TOL.LONG_RUN


def cross_row(t):
    return TOL.CROSS_KERNEL


_engines = {}


def engine(name):
    if name not in _engines:
        env, K, hidden, _ = SP.SHAPES[name]
        dm, theta = SP.problem_data(name)[:2]
        _engines[name] = Hh.engine_of(env, K, hidden, (32, 32), dm, theta)
    return _engines[name]


def run(name, B, T, S, gamma, stop, in_std, with_noise, force_generic=False, want=WANT, seed=0, init=None, noise=None):
    eng = engine(name)
    if init is None:
        init, noise = SP.inputs(name, B, T, S, with_noise, seed)
    n_dev = torch.as_tensor(noise, device=eng.device) if noise is not None else None
    n_before = n_dev.clone() if n_dev is not None else None
    out = eng.score_policy_actions(init, n_dev, T=T, gamma=gamma, stop_at_done=stop, noise_in_std=in_std, want=want, force_generic=force_generic)
    kernel = eng.last_score_policy_actions_kernel()
    assert n_dev is None or torch.equal(n_dev, n_before)                              # d_noise is never written
    K = eng.K
    assert out['ret'].shape == (K, B) and all(out[w].shape == ((K, B) if w == 'len' else (B,)) for w in want if w in ('len', 'ret_mean', 'ret_std'))
    if 'act_out' in want:
        assert out['act_out'].shape == (K, T, B, eng.na)
    return {k: cpu(v) for k, v in out.items()}, kernel


def assert_follows(tag, got, ref, gamma, row=reward_row):
    bnd = SP.bound(ref['rew'], gamma, row)                                            # [K, B]
    top = bnd.max(axis=0)
    shares = [float((np.abs(got['ret'] - ref['ret']) / bnd).max()), float((np.abs(got['ret_mean'] - ref['mean']) / top).max()),
              float((np.abs(got['ret_std'] - ref['std']) / top).max())]
    print("%s: ret %.3g, mean %.3g, std %.3g of their bounds" % ((tag,) + tuple(shares)))
    assert np.all(np.abs(got['ret'] - ref['ret']) <= bnd), "%s ret" % tag
    assert np.all(np.abs(got['ret_mean'] - ref['mean']) <= top), "%s ret_mean" % tag
    assert np.all(np.abs(got['ret_std'] - ref['std']) <= top), "%s ret_std" % tag
    assert np.array_equal(got['len'], ref['len']), "%s len" % tag


def within_one_ulp(got32, ref32):
    ref64 = ref32.astype(np.float64)
    return np.abs(got32.astype(np.float64) - ref64) <= np.spacing(np.abs(ref32).astype(np.float32)).astype(np.float64)


def tag_of(name, B, T, S, gamma, stop, in_std, with_noise):
    return "%s B=%d T=%d S=%d gamma=%g stop=%d in_std=%d noise=%d" % (name, B, T, S, gamma, stop, in_std, with_noise)


# ---- 1. the fused kernel against the restatement, at the tile edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B,T,S,gamma,stop,in_std,with_noise', SP.CASES)
def test_fused_against_the_restatement(name, B, T, S, gamma, stop, in_std, with_noise):
    env = SP.problem_data(name)[4]
    ref = SP.reference(name, B, T, S, gamma, stop, in_std, with_noise)
    assert SP.z_clear(env, ref)
    got, kernel = run(name, B, T, S, gamma, stop, in_std, with_noise)
    assert kernel == 'fused'
    assert_follows(tag_of(name, B, T, S, gamma, stop, in_std, with_noise), got, ref, gamma)
    if engine(name).K == 1:
        assert np.array_equal(got['ret_std'], np.zeros(B, np.float32)) and np.array_equal(got['ret_mean'], got['ret'][0])
    if env == 'ant' and S >= 3 and stop:
        assert (got['len'] == 1).any() and (got['len'] == T).any()                     # the planted rows: the mask acts


# ---- 2. d_act_out fed to the open-loop scorer reproduces the returns: the step arithmetic is shared, no restatement involved ----------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('name,B,T,S,gamma,stop,in_std,with_noise', [c for c in SP.CASES if c[1] in (17, 33) or c[0] == 'swimmer'])
def test_act_out_replays_through_score_actions(name, B, T, S, gamma, stop, in_std, with_noise, force):
    eng = engine(name)
    got, kernel = run(name, B, T, S, gamma, stop, in_std, with_noise, force_generic=force, want=WANT_ACT)
    assert kernel == ('generic' if force else 'fused')
    plain, _ = run(name, B, T, S, gamma, stop, in_std, with_noise, force_generic=force)
    assert np.array_equal(plain['ret'], got['ret']) and np.array_equal(plain['len'], got['len'])      # asking for d_act_out changes no bit
    init, _ = SP.inputs(name, B, T, S, with_noise)
    for k in range(eng.K):
        rep = eng.score_actions(init, torch.as_tensor(got['act_out'][k], device=eng.device), gamma=gamma, stop_at_done=stop,
                                want=('ret', 'len'), force_generic=force)
        assert np.all(within_one_ulp(got['ret'][k], cpu(rep['ret'])[k])), "%s head %d" % (name, k)
        assert np.array_equal(got['len'][k], cpu(rep['len'])[k])


# ---- 3. closed loop: along the replayed trajectory the device's own policy forward gives the actions the call took --------------------------------------
@pytest.mark.parametrize('name,B,T,S,gamma,stop,in_std,with_noise', [c for c in SP.CASES if c[1] in (17, 33) and c[7]] + [c for c in SP.CASES if c[1] == 17])
def test_closed_loop_consistency(name, B, T, S, gamma, stop, in_std, with_noise):
    eng = engine(name)
    got, kernel = run(name, B, T, S, gamma, stop, in_std, with_noise, want=WANT_ACT)
    assert kernel == 'fused'
    init, noise = SP.inputs(name, B, T, S, with_noise)
    starts = SP.start_rows(init, B).astype(np.float32)
    worst = 0.0
    for k in range(eng.K):
        obs, _, _ = eng.rollout_actions(starts, got['act_out'][k], 'eps_rand', model=k)
        obs = obs[:T].reshape(T * B, eng.ns)
        if with_noise and in_std:
            want = cpu(eng.policy_actions(obs, noise.reshape(T * B, eng.na))[0])
        else:
            want = cpu(eng.policy_actions(obs)[1])
            if with_noise:
                want = want + noise.reshape(T * B, eng.na)
        a = got['act_out'][k].reshape(T * B, eng.na)
        worst = max(worst, float((np.abs(a - want) / (TOL.ACTION['atol'] + TOL.ACTION['rtol'] * np.abs(want))).max()))
        np.testing.assert_allclose(a, want, **TOL.ACTION)
    print("%s: %.3g of ACTION" % (tag_of(name, B, T, S, gamma, stop, in_std, with_noise), worst))


# ---- 4. bit identities ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('name', ['swimmer', 'ant', 'hopper'])
def test_bit_identities(name, force):
    B, T, gamma = 33, 5, 0.99
    eng = engine(name)
    init, noise = SP.inputs(name, B, T, B)
    none, kernel = run(name, B, T, B, gamma, True, False, False, force_generic=force, init=init, noise=None)
    assert kernel == ('generic' if force else 'fused')
    for in_std in (False, True):                                                     # a zero noise tensor is no noise
        zero, _ = run(name, B, T, B, gamma, True, in_std, True, force_generic=force, init=init, noise=np.zeros_like(noise))
        for w in WANT:
            assert np.array_equal(zero[w], none[w]), (w, in_std)
    first, _ = run(name, B, T, B, gamma, True, True, True, force_generic=force, init=init, noise=noise)
    big_init, big_noise = SP.inputs(name, 160, 7, 160, seed=3)
    run(name, 160, 7, 160, gamma, True, False, True, force_generic=force, init=big_init, noise=big_noise)     # a larger call in between
    again, _ = run(name, B, T, B, gamma, True, True, True, force_generic=force, init=init, noise=noise)
    for w in WANT:
        assert np.array_equal(first[w], again[w]), w
    assert not np.array_equal(first['ret'], none['ret'])


# ---- 5. against the device's validation cost ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['swimmer', 'ant'])
def test_no_noise_gives_the_device_validation_cost(name):
    B, T, gamma = 33, 11, 0.97
    eng = engine(name)
    pool = SP.problem_data(name)[3]
    s0 = pool[:B].astype(np.float32)
    want = cpu(eng.validation_cost(s0, T, gamma))
    out = eng.score_policy_actions(s0, None, T=T, gamma=gamma)
    assert eng.last_score_policy_actions_kernel() == 'fused'
    got = -cpu(out['ret']).astype(np.float64).mean(axis=1)
    print("%s: %s against validation_cost %s" % (name, got, want))
    np.testing.assert_allclose(got, want, **TOL.VALIDATION_COST)


# ---- 6. the generic path ---------------------------------------------------------------------------------------------------------------------------------
def host_chain(eng, init, noise, T, gamma, stop, in_std):
    """The host loop the call replaces: per head and step policy_actions (+ add) and step, then the formula in NumPy float64 -> (ret [K, B], len)"""
    B = noise.shape[1] if noise is not None else init.shape[0]
    starts = torch.as_tensor(SP.start_rows(init, B).astype(np.float32), device=eng.device)
    nz = torch.as_tensor(noise, device=eng.device) if noise is not None else None
    rets, lens = [], []
    for k in range(eng.K):
        s, rews, dones = starts, [], []
        model = torch.full((B,), k, dtype=torch.int32, device=eng.device)
        for t in range(T):
            if nz is not None and in_std:
                a = eng.policy_actions(s, nz[t])[0]
            else:
                a = eng.policy_actions(s)[0]
                if nz is not None:
                    a = a + nz[t]
            s, r, d = eng.step(s, a, 'eps_rand', model_idx=model)[:3]
            rews.append(cpu(r)); dones.append(cpu(d))
        ret, n = SA.discount_and_sum(np.stack(rews), np.stack(dones), gamma, stop)
        rets.append(ret); lens.append(n)
    return np.stack(rets), np.stack(lens)


@pytest.mark.parametrize('name,B,T,S,gamma,stop,in_std,with_noise', SP.CASES)
def test_generic_on_the_fused_shapes(name, B, T, S, gamma, stop, in_std, with_noise):
    env = SP.problem_data(name)[4]
    ref = SP.reference(name, B, T, S, gamma, stop, in_std, with_noise)
    got, kernel = run(name, B, T, S, gamma, stop, in_std, with_noise, force_generic=True)
    assert kernel == 'generic'
    tag = tag_of(name, B, T, S, gamma, stop, in_std, with_noise)
    assert_follows(tag + " generic", got, ref, gamma)
    if T <= 10:
        fused, f_kernel = run(name, B, T, S, gamma, stop, in_std, with_noise)
        assert f_kernel == 'fused'
        bnd = SP.bound(ref['rew'], gamma, cross_row)
        print("%s fused vs generic: %.3g of the bound" % (tag, float((np.abs(fused['ret'] - got['ret']) / bnd).max())))
        assert np.all(np.abs(fused['ret'] - got['ret']) <= bnd)
        assert np.array_equal(fused['len'], got['len'])
    if B == 17 or (B == 33 and T == 2):
        init, noise = SP.inputs(name, B, T, S, with_noise)
        ret, n = host_chain(engine(name), init, noise, T, gamma, stop, in_std)
        assert np.all(within_one_ulp(got['ret'], ret.astype(np.float32))) and np.array_equal(got['len'], n)


@pytest.mark.parametrize('name,B,T,S,cap', [('swimmer', 33, 11, 3, 7), ('ant', 33, 2, 33, 16), ('hopper', 17, 5, 1, 16), ('swimmer9', 33, 3, 33, 1)])
def test_generic_chunking_changes_no_bit(name, B, T, S, cap):
    """The generic path walks the candidates in chunks (workspace within 2^26 floats).  With the chunk capped through the library's test hook so that
    there are several chunks and a ragged last one (33 = 4 x 7 + 5, 2 x 16 + 1, 17 = 16 + 1, and chunks of one), every output is the unchunked call's
    bit for bit -- with plain noise, noise in std and no noise, and with act_out."""
    from metrpo_amd import _lib
    eng = engine(name)
    gamma = 0.99
    init, noise = SP.inputs(name, B, T, S)
    if S != B:
        variants = [(False, True), (True, True)]
    else:
        variants = [(False, True), (True, True), (False, False)]
    for in_std, with_noise in variants:
        nz = noise if with_noise else None
        whole, kernel = run(name, B, T, S, gamma, True, in_std, with_noise, force_generic=True, want=WANT_ACT, init=init, noise=nz)
        assert kernel == 'generic'
        assert _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, cap) == 0
        try:
            parts, kernel = run(name, B, T, S, gamma, True, in_std, with_noise, force_generic=True, want=WANT_ACT, init=init, noise=nz)
        finally:
            assert _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, 0) == 0
        assert kernel == 'generic'
        for w in WANT_ACT:
            assert np.array_equal(parts[w], whole[w]), (w, in_std, with_noise)
    assert _lib.lib.metrpo_debug_score_policy_chunk(eng._ctx, -1) == -1 and _lib.lib.metrpo_debug_score_policy_chunk(None, 1) == -2


OFF_TABLE = [('wide', 'swimmer', 5, (128, 128), (32, 32)), ('humanoid', 'humanoid', 2, (256, 256), (100, 50, 25)), ('pol3', 'swimmer', 3, (64, 64), (100, 50, 25))]


@pytest.mark.parametrize('tag,env,K,dh,ph', OFF_TABLE, ids=[c[0] for c in OFF_TABLE])
def test_off_table_shapes_take_the_generic_path(tag, env, K, dh, ph):
    B, T, S, gamma = 17, 3, 17, 0.99
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, dh, ph, seed=11, n_pool=32)
    rng = np.random.RandomState(5)
    init = pool[rng.randint(len(pool), size=S)].astype(np.float32)
    noise = (0.5 * rng.randn(T, B, dm.na)).astype(np.float32)
    for in_std, nz in ((False, noise), (True, noise), (False, None)):
        out = eng.score_policy_actions(init, nz, T=T, gamma=gamma, noise_in_std=in_std, want=WANT)
        assert eng.last_score_policy_actions_kernel() == 'generic'
        ret, n = host_chain(eng, init, nz, T, gamma, True, in_std)
        assert np.isfinite(cpu(out['ret'])).all()
        assert np.all(within_one_ulp(cpu(out['ret']), ret.astype(np.float32))) and np.array_equal(cpu(out['len']), n)
        ref = SP.score_policy_actions(dm.astype(np.float32).astype(np.float64), theta.astype(np.float32).astype(np.float64), pdims, env, init, nz, T=T,
                                      gamma=gamma, noise_in_std=in_std, keep=True)
        assert np.isfinite(ref['obs']).all() and np.array_equal(ref['len'], n)
        bnd = SP.bound(ref['rew'], gamma, lambda t: TOL.WIDE)                         # three free-running steps of a wide net: row 2 per step
        print("%s in_std=%d noise=%d: %.3g of the bound" % (tag, in_std, nz is not None, float((np.abs(cpu(out['ret']) - ref['ret']) / bnd).max())))
        assert np.all(np.abs(cpu(out['ret']) - ref['ret']) <= bnd)


# ---- 7. memory and state ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('force', [False, True], ids=['fused', 'generic'])
@pytest.mark.parametrize('name', ['swimmer', 'ant'])
@pytest.mark.parametrize('B', [17, 1])
def test_no_write_beyond_B_and_no_read_beyond_B(name, B, force):
    """Each output is the front of a larger allocation whose tail holds a sentinel; the noise is the front of an allocation whose tail is NaN."""
    eng = engine(name)
    K, T, G, na = eng.K, 3, 5, eng.na
    init, noise = SP.inputs(name, B, T, 1)
    dev = eng.device
    big = torch.full((T * B * na + 64,), float('nan'), dtype=torch.float32, device=dev)
    big[:T * B * na] = torch.as_tensor(noise, device=dev).reshape(-1)
    n_dev = big[:T * B * na].view(T, B, na)
    size = {'ret': K * B, 'len': K * B, 'ret_mean': B, 'ret_std': B, 'act_out': K * T * B * na}
    g = {w: torch.full((size[w] + G,), -77 if w == 'len' else 777.0, dtype=torch.int32 if w == 'len' else torch.float32, device=dev) for w in size}
    out = eng.score_policy_actions(init, n_dev, gamma=0.99, noise_in_std=True, want=WANT_ACT, force_generic=force, out={w: g[w][:size[w]] for w in g})
    assert eng.last_score_policy_actions_kernel() == ('generic' if force else 'fused')
    plain = eng.score_policy_actions(init, torch.as_tensor(noise, device=dev), gamma=0.99, noise_in_std=True, want=WANT_ACT, force_generic=force)
    torch.cuda.synchronize()
    for w in g:
        assert torch.all(g[w][size[w]:] == (-77 if w == 'len' else 777.0)), w          # nothing behind the output
        assert not torch.any(g[w][:size[w]] == (-77 if w == 'len' else 777.0)), w      # every cell in front of it was written
        assert torch.equal(out[w].reshape(-1), plain[w].reshape(-1)), w                # NaN tails never read; repeated calls bit-identical
    assert torch.isfinite(plain['ret']).all() and torch.isfinite(plain['act_out']).all()


def test_a_call_changes_nothing_else_and_follows_set_policy():
    dm, theta, pdims, pool, env = SP.problem_data('swimmer')
    eng = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)
    rng = np.random.RandomState(0)
    x = rng.randn(5 * 16, dm.ns + dm.na).astype(np.float32); y = rng.randn(5 * 16, dm.ns).astype(np.float32)
    eng.train_step(x, y, 16, 1e-3)
    eng.policy_adam_step(torch.as_tensor(rng.randn(eng.P), dtype=torch.float64, device=eng.device), 1e-3)
    state = lambda: [eng.get_policy().clone(), eng.get_dynamics().clone()] + [t.clone() if torch.is_tensor(t) else t for t in eng.get_train_adam()] + \
        [t.clone() if torch.is_tensor(t) else t for t in eng.get_policy_adam()]
    before = state()
    roll = lambda: eng.rollout(128, 6, 4, 'step_rand', pool.astype(np.float32), seed=5)
    t1 = roll()
    o1, r1, a1 = t1.obs.clone(), t1.rew.clone(), t1.act.clone()
    kernel, note = eng.last_rollout_kernel(), eng.rollout_note()
    acts = (1.5 * rng.randn(5, 40, dm.na)).astype(np.float32)
    eng.rollout_actions(pool[:40].astype(np.float32), acts, 'model_mean')
    eng.ensemble_disagreement(pool[:40].astype(np.float32), acts[0], force_generic=True)
    eng.score_actions(pool[:8].astype(np.float32), acts, force_generic=True)
    reporters = lambda: (eng.last_rollout_actions_kernel(), eng.last_disagreement_kernel(), eng.last_score_actions_kernel(), eng.last_score_actions_grad_kernel())
    rep = reporters()
    assert rep == ('fused', 'generic', 'generic', None) and eng.last_score_policy_actions_kernel() is None
    res = {}
    for force in (False, True):
        res[force] = eng.score_policy_actions(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT_ACT, force_generic=force)
        assert eng.last_score_policy_actions_kernel() == ('generic' if force else 'fused')
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note and reporters() == rep
    t2 = roll()                                                                           # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)
    # the policy is read at call time: another theta, another result; the first theta again, the first result again
    th0 = eng.get_policy().clone()
    eng.set_policy(cpu(th0) + 0.05 * rng.randn(eng.P).astype(np.float32))
    for force in (False, True):
        other = eng.score_policy_actions(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT_ACT, force_generic=force)
        assert not torch.equal(other['ret'], res[force]['ret'])
    eng.set_policy(th0)
    for force in (False, True):
        back = eng.score_policy_actions(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT_ACT, force_generic=force)
        for w in WANT_ACT:
            assert torch.equal(back[w], res[force][w]), w


def test_abi_argument_and_state_errors():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    eng = engine('swimmer')
    dm, theta, pdims, pool, env = SP.problem_data('swimmer')
    dev = eng.device
    B, T, S, K, ns, na = 4, 2, 2, eng.K, eng.ns, eng.na
    init, nz = torch.zeros(S, ns, device=dev), torch.zeros(T, B, na, device=dev)
    ret = torch.full((K, B), 555.0, dtype=torch.float32, device=dev)
    ln = torch.full((K, B), -55, dtype=torch.int32, device=dev)
    mean, sd = torch.full((B,), 555.0, device=dev), torch.full((B,), 555.0, device=dev)

    def args(**kw):
        a = _lib.ScorePolicyActionsArgs()
        a.B, a.T, a.S, a.stop_at_done, a.gamma = B, T, S, 1, 0.99
        a.d_init_obs, a.d_noise, a.d_ret, a.d_len, a.d_ret_mean, a.d_ret_std = (init.data_ptr(), nz.data_ptr(), ret.data_ptr(), ln.data_ptr(),
                                                                               mean.data_ptr(), sd.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.metrpo_score_policy_actions(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_score_policy_actions(None, C.byref(args()), eng._stream()) == -2 and lib.metrpo_last_score_policy_actions_kernel(None) == -2
    assert lib.metrpo_score_policy_actions(eng._ctx, None, eng._stream()) == -2 and b'args NULL' in err()
    for name in ('d_init_obs', 'd_ret'):
        assert call(args(**{name: None})) == -2 and b'required pointer' in err()          # METRPO_ENULL
    assert call(args(B=-1)) == -1 and b'bad B/T' in err()                                 # METRPO_EINVAL
    assert call(args(T=-1)) == -1 and b'bad B/T' in err()
    for bad in (0, -1, 3):
        assert call(args(S=bad)) == -1 and b'must be at least 1 and divide B' in err()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(args(gamma=bad)) == -1 and b'gamma is not finite' in err()
    for kw in (dict(B=0), dict(T=0), dict(B=0, d_ret=None)):                              # B == 0 or T == 0: OK, nothing written
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert torch.all(ret == 555.0) and torch.all(ln == -55) and torch.all(mean == 555.0) and torch.all(sd == 555.0)
    for kw in (dict(d_len=None), dict(d_ret_mean=None), dict(d_noise=None, B=S), dict(d_len=None, d_ret_mean=None, d_ret_std=None), dict(force_generic=1, d_len=None)):
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert not torch.any(ret == 555.0) and not torch.any(ln == -55) and not torch.any(mean == 555.0) and not torch.any(sd == 555.0)
    # dynamics AND the policy must be set
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_score_policy_actions(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    bare.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    assert lib.metrpo_score_policy_actions(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_policy' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_score_policy_actions_kernel() is None
    # while a TRPO update is open the policy is undecided
    own = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)
    traj = own.rollout(64, 6, 3, 'step_rand', pool.astype(np.float32), seed=1)
    adv, _, valid, stats = own.gae(traj, None, 0.99, 0.95)
    own.center_advantages(adv, valid, stats)
    batch = own.make_batch(traj.obs, traj.act, adv, traj.mean, own.get_policy()[-na:], valid=valid)
    assert own.trpo_update(batch, spec_trials=1) is None
    with pytest.raises(_lib.MetrpoError, match='still open'):
        own.score_policy_actions(init, nz)
    own.trpo_update_end()
    assert own.score_policy_actions(init, nz)['ret'].shape == (K, B)
    # the host method's own checks
    with pytest.raises(ValueError, match=r'init_obs: expected \[S, 10\]'):
        eng.score_policy_actions(torch.zeros(S, ns + 1), nz)
    with pytest.raises(ValueError, match=r'noise: expected \[T, B, 2\] with B a multiple of 3'):
        eng.score_policy_actions(torch.zeros(3, ns), nz)
    with pytest.raises(ValueError, match='want'):
        eng.score_policy_actions(init, nz, want=('ret', 'median'))
    with pytest.raises(ValueError, match='needs T='):
        eng.score_policy_actions(init)
    with pytest.raises(ValueError, match='gamma must be finite'):
        eng.score_policy_actions(init, nz, gamma=float('inf'))
    assert eng.score_policy_actions(torch.zeros(ns), nz, want=WANT)['ret'].shape == (K, B)   # [ns]: one start state
    assert eng.score_policy_actions(init, T=3)['ret'].shape == (K, S)


# ---- 8. the planner on the device -----------------------------------------------------------------------------------------------------------------------
def test_plan_cem_policy_on_the_device(monkeypatch):
    from metrpo_amd import planning as P
    eng = engine('swimmer')
    dm, theta, pdims, pool, env = SP.problem_data('swimmer')
    S, N, T, E, gamma = 2, 48, 5, 6, 0.99
    states = pool[[3, 17]].astype(np.float32)
    shown = []

    def restated(noise, init):                                  # the float64 restatement wrapped for torch
        ref = SP.score_policy_actions(dm, theta, pdims, env, cpu(init), cpu(noise), gamma=gamma, keep=True)
        shown.append(ref)
        return torch.as_tensor(ref['ret'], dtype=torch.float32, device=noise.device)

    gen = lambda seed: torch.Generator(device=eng.device).manual_seed(seed)
    seed = None
    for s in range(8):                                          # a seed at which the restatement's elite set is decided by more than the bound
        del shown[:]
        want = P.plan_cem_policy(eng, states, T, N, E, 1, gamma=gamma, generator=gen(s), scorer=restated)
        ref = shown[0]
        score = ref['ret'].mean(axis=0).reshape(S, N)
        bnd = SP.bound(ref['rew'], gamma, reward_row).max(axis=0).reshape(S, N)
        el = cpu(want['elites'])
        ok = True
        for i in range(S):
            rest = np.setdiff1d(np.arange(N), el[i])
            ok = ok and (score[i, el[i]] - bnd[i, el[i]]).min() > (score[i, rest] + bnd[i, rest]).max()
        if ok:
            seed = s
            break
    assert seed is not None
    got1 = P.plan_cem_policy(eng, states, T, N, E, 1, gamma=gamma, generator=gen(seed))
    assert eng.last_score_policy_actions_kernel() == 'fused'
    for i in range(S):
        assert set(cpu(got1['elites'])[i].tolist()) == set(el[i].tolist())
    np.testing.assert_allclose(cpu(got1['noise']), cpu(want['noise']), rtol=0, atol=1e-6)             # the same elites: the same refit
    # three iterations with nothing read back: one synchronize behind the call, none inside
    torch.cuda.synchronize()
    counts = dict(sync=0, item=0, cpu=0)
    real_sync, real_item, real_cpu = torch.cuda.synchronize, torch.Tensor.item, torch.Tensor.cpu

    def counted(key, fn):
        def wrapper(*a, **kw):
            counts[key] += 1
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(torch.cuda, 'synchronize', counted('sync', real_sync))
    monkeypatch.setattr(torch.Tensor, 'item', counted('item', real_item))
    monkeypatch.setattr(torch.Tensor, 'cpu', counted('cpu', real_cpu))
    got3 = P.plan_cem_policy(eng, states, T, N, E, 3, gamma=gamma, generator=gen(seed))
    inside = dict(counts)
    torch.cuda.synchronize()
    assert inside == dict(sync=0, item=0, cpu=0) and counts['sync'] == 1
    monkeypatch.undo()
    assert got3['history'].shape == (3, S) and torch.isfinite(got3['history']).all() and torch.isfinite(got3['noise']).all()
    assert torch.all(got3['best_score'] >= got3['policy_score'])                          # never worse than the policy under the scorer
    pol = eng.score_policy_actions(states, None, T=T, gamma=gamma)['ret'].mean(dim=0)
    torch.testing.assert_close(pol, got3['policy_score'], rtol=1e-5, atol=1e-5)           # delta = 0 is the policy itself
    sc = P.score_noise_sequences(eng, states, got3['best_noise'], gamma=gamma)
    torch.testing.assert_close(sc, got3['best_score'], rtol=1e-5, atol=1e-5)              # the best candidate scores what the planner recorded
    # the controller: one planning call and one policy forward
    ctl = P.ShootingController(eng, horizon=T, n_candidates=N, n_elites=E, n_iters=2, init_std=0.5, gamma=gamma, generator=gen(1), policy_prior=True)
    a, _ = ctl.get_actions(states)
    mean = cpu(eng.policy_actions(states)[1])
    np.testing.assert_allclose(a, np.clip(mean + cpu(ctl.last_plan['noise'])[:, 0], -1.0, 1.0), rtol=0, atol=1e-6)
    assert a.shape == (S, eng.na) and np.abs(a).max() <= 1.0 and torch.all(ctl._mean[:, -1] == 0)


def test_example_loop_collects_with_the_policy_prior_controller():
    """examples/me_trpo_loop.py --shooting --shooting-policy-prior: from the second outer iteration on the real data are collected by
    planning.ShootingController planning in noise space around the policy (tests/test_gpu_score_actions.py's sizes)."""
    import importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('me_trpo_loop', os.path.join(root, 'examples', 'me_trpo_loop.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    hist = mod.main(['--outer', '2', '--K', '3', '--T', '20', '--traj', '40', '--n-envs', '200', '--policy-iters', '6', '--model-passes', '6',
                     '--quiet', '--shooting', '--shooting-policy-prior'])
    assert len(hist) == 2 and hist[1]['n_data'] > hist[0]['n_data'] > 0
    assert all(np.isfinite([h['real_cost'], h['model_val'], h['est_cost']]).all() for h in hist)
