"""GPU tests of metrpo_score_policy_actions_grad (csrc/score_policy_actions_grad.hip): the gradient of every head's closed-loop return with respect to
noise sequences around the policy, against the float64 restatement tests/score_policy_grad_ref.py on the cases of tests/score_policy_grad_cases.py
(drawn clear of every relu / clip / cost / done kink), against metrpo_score_policy_actions and metrpo_score_actions_grad, and under
metrpo_amd.planning.refine_noise / plan_cem_policy_gd.

Bounds, all from tests/tolerances.py, none new:
  grad, grad_mean, lam0  rel-L2 <= BPTT_GRAD_REL_L2 per head (the project's row for gradients through this same policy-plus-dynamics chain, tanh_fast
                         included), and per time step and per candidate by block_bound(BPTT_GRAD_REL_L2, block, whole);
  ret                    sum_t gamma^t (atol + rtol |r_t|) with REWARD / LONG_RUN rows (score_actions_ref.bound);
  len                    exact;  ret / len / act_out bit for bit metrpo_score_policy_actions' on the same path.
Worst shares observed are recorded in profiles/r25_score_policy_actions_grad.txt."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
import tolerances as TOL
import score_policy_grad_cases as PC

pytestmark = pytest.mark.gpu

ROW = TOL.BPTT_GRAD_REL_L2
WANT = ('grad', 'ret', 'len', 'grad_mean', 'lam0', 'act_out')
FUSED_ENVS = PC.GC.FUSED_ENVS


def cpu(t):
    return t.detach().cpu().numpy()


_engines = {}


def engine(case):
    key = PC.shape_key(case)
    if key not in _engines:
        dm, theta, _, _ = PC.problem(case)
        _engines[key] = Hh.engine_of(case.env, case.K, case.dh, (32, 32), dm, theta, dyn_act=case.act)
    return _engines[key]


def fused_shape(case):
    return case.env in FUSED_ENVS and len(case.dh) == 2 and max(case.dh) <= 64 and case.act == 'relu'


def forced(case):
    return case.path == 'generic'


def run(case, d=None, force_generic=None, chunk=0, want=WANT, noise='case'):
    d = PC.case_data(case) if d is None else d
    eng = engine(case)
    force = forced(case) if force_generic is None else force_generic
    nz = d['noise'] if isinstance(noise, str) else noise
    kw = dict(gamma=case.gamma, stop_at_done=case.stop, noise_in_std=case.in_std, want=want, force_generic=force, chunk=chunk)
    init = np.asarray(d['init'], np.float32)
    if nz is None:
        out = eng.score_policy_actions_grad(init, None, T=case.T, **kw)
    else:
        n_dev = torch.as_tensor(nz, dtype=torch.float32, device=eng.device)
        before = n_dev.clone()
        out = eng.score_policy_actions_grad(init, n_dev, **kw)
        assert torch.equal(n_dev, before)                                             # d_noise is never written
    assert eng.last_score_policy_actions_grad_kernel() == ('fused' if (fused_shape(case) and not force) else 'generic')
    return {k: cpu(v) for k, v in out.items()}


def head_order_mean(grad):
    """(sum_k grad_k) / K in fp32, summed in head order"""
    s = np.zeros(grad.shape[1:], np.float32)
    for k in range(grad.shape[0]):
        s = s + grad[k]
    return s / np.float32(grad.shape[0])


def pick(path, env='swimmer', **kw):
    return next(c for c in PC.CASES if c.path == path and c.env == env and all(getattr(c, k) == v for k, v in kw.items()))


# ---- 1. either path against the restatement, at the tile and workgroup edges --------------------------------------------------------------------------
@pytest.mark.parametrize('case', PC.CASES, ids=[c.id for c in PC.CASES])
def test_against_the_restatement(case):
    """Worst shares observed over the table (MI355X): profiles/r25_score_policy_actions_grad.txt."""
    d = PC.case_data(case)
    assert d['accepted'] == case.B
    ref = PC.reference(d)
    got = run(case, d)
    K, T, B = case.K, case.T, case.B
    dm = d['dm']
    assert got['grad'].shape == (K, T, B, dm.na) and got['lam0'].shape == (K, B, dm.ns) and got['grad_mean'].shape == (T, B, dm.na)
    use = PC.shares(got, ref, case)
    print("%s: grad %.3g whole, %.3g per step, %.3g per candidate; lam0 %.3g whole, %.3g per candidate; ret %.3g; grad_mean %.3g of their bounds"
          % ((case.id,) + tuple(use)))
    assert np.array_equal(got['len'], ref['len'])
    assert use.max() <= 1.0, use
    # exact zeros: a clipped action of the head's own trajectory, and every step behind a candidate's last counted step
    clipped = np.abs(got['act_out']) > 1
    assert clipped.any() and np.all(got['grad'][clipped] == 0)
    assert np.array_equal(clipped, np.abs(ref['act']) > 1)                             # the guard kept every action clear of the clip
    behind = np.arange(T)[None, :, None] >= ref['len'][:, None, :]
    assert np.all(got['grad'][behind] == 0)
    assert np.array_equal(got['grad_mean'], head_order_mean(got['grad']))             # bit for bit the head-order sum divided by K
    if case.path == 'generic' and fused_shape(case):                                   # the two device paths against each other
        fused = run(case, d, force_generic=False)
        for k in range(K):
            rel = np.linalg.norm(fused['grad'][k].astype(np.float64) - got['grad'][k]) / max(np.linalg.norm(ref['grad'][k]), 1e-300)
            rl = np.linalg.norm(fused['lam0'][k].astype(np.float64) - got['lam0'][k]) / max(np.linalg.norm(ref['lam0'][k]), 1e-300)
            assert rel <= ROW and rl <= ROW, (k, rel, rl)
        assert np.array_equal(fused['len'], got['len'])


def test_cases_reach_both_paths():
    seen = set()
    for case in PC.CASES:
        if (case.path, fused_shape(case)) in seen:
            continue
        seen.add((case.path, fused_shape(case)))
        run(case, want=('grad',))                                                      # (run asserts the reporter)
        want = 'fused' if case.path == 'fused' else 'generic'
        assert engine(case).last_score_policy_actions_grad_kernel() == want, case.id
    assert seen == {('fused', True), ('generic', True), ('generic', False)}
    assert all(fused_shape(c) for c in PC.CASES if c.path == 'fused')


# ---- 2. ret / len / act_out are metrpo_score_policy_actions', bit for bit on the same path ----------------------------------------------------------------
SAME_PATH = [c for c in PC.CASES if c.T == 11 or c.dh != (64, 64) or c.K != 5 or c.T == 1 or c.B in (1, 65)]


@pytest.mark.parametrize('case', SAME_PATH, ids=[c.id for c in SAME_PATH])
def test_ret_len_and_act_out_are_score_policy_actions_bits(case):
    d = PC.case_data(case)
    got = run(case, d)
    eng = engine(case)
    sp = eng.score_policy_actions(np.asarray(d['init'], np.float32), np.asarray(d['noise'], np.float32), gamma=case.gamma, stop_at_done=case.stop,
                                  noise_in_std=case.in_std, want=('ret', 'len', 'act_out'), force_generic=forced(case))
    assert eng.last_score_policy_actions_kernel() == eng.last_score_policy_actions_grad_kernel()
    for w in ('ret', 'len', 'act_out'):
        assert np.array_equal(got[w], cpu(sp[w])), w


# ---- 3. T = 1: no policy path, the gradient is metrpo_score_actions_grad's at act_out -------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_one_step_is_the_open_loop_gradient_at_act_out(path):
    case = pick(path, 'half_cheetah', T=1)
    d = PC.case_data(case)
    ref = PC.reference(d)
    got = run(case, d)
    eng = engine(case)
    scale = np.exp(np.maximum(d['theta'][-d['dm'].na:], np.log(1e-6))) if case.in_std else 1.0
    for k in range(case.K):
        sa = eng.score_actions_grad(np.asarray(d['init'], np.float32), got['act_out'][k], gamma=case.gamma, stop_at_done=case.stop,
                                    want=('grad', 'lam0', 'ret'), force_generic=forced(case))
        use = PC.GC.grad_use(cpu(sa['grad'])[k].astype(np.float64) * scale, ref['grad'][k], ROW)
        assert max(use) <= 1.0, (k, use)
        if not case.in_std:                                                            # the same tables, the same chains, no sigma: the same bits
            assert np.array_equal(cpu(sa['grad'])[k], got['grad'][k])
        assert np.array_equal(cpu(sa['ret'])[k], got['ret'][k])
    # with a policy in the loop lam0 differs from the open-loop one even at T = 1 (s_0 moves a_0); it is held against the restatement above


# ---- 4. d_noise NULL is a zero noise tensor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('in_std', [False, True], ids=['act', 'std'])
def test_no_noise_equals_zero_noise(path, in_std):
    case = pick(path, 'hopper', S=16)._replace(in_std=in_std)                          # B = S
    d = PC.case_data(pick(path, 'hopper', S=16))
    none = run(case, d, noise=None)
    zero = run(case, d, noise=np.zeros_like(d['noise']))
    for w in WANT:
        assert np.array_equal(none[w], zero[w]), w
    assert np.any(none['grad'] != 0)


# ---- 5. chunking changes no bit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_chunked_calls_equal_the_unchunked_call(path, env):
    case = pick(path, env, B=33, T=11, stop=True)
    whole = run(case)
    for chunk in (16, 17, 1000):                                                       # a ragged last chunk: 33 = 16 + 16 + 1 = 17 + 16
        part = run(case, chunk=chunk)
        for w in WANT:
            assert np.array_equal(whole[w], part[w]), (chunk, w)


# ---- 6. guard cells, oversized outputs, repeated calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('B', [17, 1])
def test_no_write_outside_the_outputs(path, B):
    """Each output sits in the middle of a larger allocation: G guard cells in front of it and a NaN (-77 for len) tail behind it stay put."""
    case = pick(path, 'swimmer', B=B, K=5)
    d = PC.case_data(case)
    eng = engine(case)
    dev = eng.device
    K, T, G = case.K, case.T, 7
    ns, na = d['dm'].ns, d['dm'].na
    n = {'grad': K * T * B * na, 'ret': K * B, 'len': K * B, 'grad_mean': T * B * na, 'lam0': K * B * ns, 'act_out': K * T * B * na}
    fill = lambda w: -77 if w == 'len' else float('nan')
    buf = {w: torch.full((G + n[w] + G,), fill(w), dtype=torch.int32 if w == 'len' else torch.float32, device=dev) for w in WANT}
    n_dev = torch.as_tensor(d['noise'], dtype=torch.float32, device=dev)
    init = np.asarray(d['init'], np.float32)
    kw = dict(gamma=case.gamma, noise_in_std=case.in_std, want=WANT, force_generic=forced(case))
    out = eng.score_policy_actions_grad(init, n_dev, out={w: buf[w][G:] for w in WANT}, **kw)
    plain = eng.score_policy_actions_grad(init, n_dev, **kw)
    again = eng.score_policy_actions_grad(init, n_dev, **kw)
    torch.cuda.synchronize()
    for w in WANT:
        edge = torch.cat([buf[w][:G], buf[w][G + n[w]:]])
        assert torch.all(edge == -77) if w == 'len' else torch.all(torch.isnan(edge)), w
        body = buf[w][G:G + n[w]]
        assert not torch.any(body == -77) if w == 'len' else not torch.any(torch.isnan(body)), w      # every cell of the output was written
        assert torch.equal(body, plain[w].reshape(-1)) and torch.equal(plain[w], again[w]), w         # repeated calls are bit-identical
        assert out[w].data_ptr() == buf[w][G:].data_ptr()


def test_a_small_call_after_a_large_one():
    small = pick('fused', 'swimmer', B=17, K=5)
    large = pick('fused', 'swimmer', B=33, T=11, stop=True)
    assert PC.shape_key(small) == PC.shape_key(large)
    for force in (False, True):
        first = run(small, force_generic=force)
        run(large, force_generic=force)                                               # grows the workspace and leaves it full of another case's states
        second = run(small, force_generic=force)
        for w in WANT:
            assert np.array_equal(first[w], second[w]), w


# ---- 7. a call changes nothing else --------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_else():
    case = pick('fused', 'swimmer', B=17, K=5)
    dm, theta, pdims, pool = PC.problem(case)
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
    acts = (0.8 * rng.randn(5, 40, dm.na)).astype(np.float32)
    eng.rollout_actions(pool[:40].astype(np.float32), acts, 'model_mean')
    eng.ensemble_disagreement(pool[:40].astype(np.float32), acts[0], force_generic=True)
    eng.score_actions(pool[:8].astype(np.float32), acts, gamma=0.99)
    eng.score_actions_grad(pool[:8].astype(np.float32), acts, gamma=0.99, force_generic=True)
    eng.score_policy_actions(pool[:8].astype(np.float32), acts, gamma=0.99)
    sibs = lambda: (eng.last_rollout_actions_kernel(), eng.last_disagreement_kernel(), eng.last_score_actions_kernel(), eng.last_score_actions_grad_kernel(),
                    eng.last_score_policy_actions_kernel())
    assert sibs() == ('fused', 'generic', 'fused', 'generic', 'fused') and eng.last_score_policy_actions_grad_kernel() is None
    for force in (False, True):
        eng.score_policy_actions_grad(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT, force_generic=force)
        assert eng.last_score_policy_actions_grad_kernel() == ('generic' if force else 'fused')
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note and sibs() == ('fused', 'generic', 'fused', 'generic', 'fused')
    t2 = roll()                                                                           # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


# ---- 8. the ABI's argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_and_state_errors():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    case = pick('fused', 'swimmer', K=5)
    eng, (dm, theta, _, pool) = engine(case), PC.problem(case)
    dev = eng.device
    B, T, S, K, ns, na = 4, 2, 2, dm.K, dm.ns, dm.na
    init, nz = torch.zeros(S, ns, device=dev), torch.zeros(T, B, na, device=dev)
    grad = torch.full((K, T, B, na), 555.0, device=dev); gm = torch.full((T, B, na), 555.0, device=dev); lam = torch.full((K, B, ns), 555.0, device=dev)
    ret = torch.full((K, B), 555.0, device=dev); ln = torch.full((K, B), -55, dtype=torch.int32, device=dev); ao = torch.full((K, T, B, na), 555.0, device=dev)
    outs = (grad, gm, lam, ret, ao)

    def args(**kw):
        a = _lib.ScorePolicyActionsGradArgs()
        a.B, a.T, a.S, a.stop_at_done, a.gamma = B, T, S, 1, 0.99
        a.d_init_obs, a.d_noise, a.d_grad, a.d_ret, a.d_len, a.d_grad_mean, a.d_lam0, a.d_act_out = (
            init.data_ptr(), nz.data_ptr(), grad.data_ptr(), ret.data_ptr(), ln.data_ptr(), gm.data_ptr(), lam.data_ptr(), ao.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.metrpo_score_policy_actions_grad(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_score_policy_actions_grad(None, C.byref(args()), eng._stream()) == -2 and lib.metrpo_last_score_policy_actions_grad_kernel(None) == -2
    assert lib.metrpo_score_policy_actions_grad(eng._ctx, None, eng._stream()) == -2 and b'score_policy_actions_grad: args NULL' in err()
    for name in ('d_init_obs', 'd_grad'):
        assert call(args(**{name: None})) == -2 and b'score_policy_actions_grad: required pointer' in err()      # METRPO_ENULL
    assert call(args(B=-1)) == -1 and b'score_policy_actions_grad: bad B/T' in err()                              # METRPO_EINVAL
    assert call(args(T=-1)) == -1 and b'bad B/T' in err()
    for bad in (0, -1, 3):
        assert call(args(S=bad)) == -1 and b'must be at least 1 and divide B' in err()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(args(gamma=bad)) == -1 and b'score_policy_actions_grad: gamma is not finite' in err()
    assert call(args(chunk=-1)) == -1 and b'chunk must not be negative' in err()
    for kw in (dict(B=0), dict(T=0), dict(B=0, d_grad=None)):                            # B == 0 or T == 0: OK, nothing written
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert all(torch.all(t == 555.0) for t in outs) and torch.all(ln == -55)
    for kw in (dict(d_ret=None), dict(d_len=None), dict(d_grad_mean=None), dict(d_lam0=None), dict(d_act_out=None), dict(d_noise=None, noise_in_std=1),
               dict(d_ret=None, d_len=None, d_grad_mean=None, d_lam0=None, d_act_out=None), dict(force_generic=1, d_ret=None, d_lam0=None),
               dict(force_generic=1, d_noise=None), dict(chunk=3), dict()):              # the optional pointers may be left out, each on its own
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert not any(torch.any(t == 555.0) for t in outs) and not torch.any(ln == -55)
    # dynamics AND the policy must be set
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_score_policy_actions_grad(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    bare.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    assert lib.metrpo_score_policy_actions_grad(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_policy' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_score_policy_actions_grad_kernel() is None
    # while a TRPO update is open the policy is undecided
    own = Hh.engine_of('swimmer', 5, (64, 64), (32, 32), dm, theta)
    traj = own.rollout(64, 6, 3, 'step_rand', pool.astype(np.float32), seed=1)
    adv, _, valid, stats = own.gae(traj, None, 0.99, 0.95)
    own.center_advantages(adv, valid, stats)
    batch = own.make_batch(traj.obs, traj.act, adv, traj.mean, own.get_policy()[-na:], valid=valid)
    assert own.trpo_update(batch, spec_trials=1) is None
    with pytest.raises(_lib.MetrpoError, match='still open'):
        own.score_policy_actions_grad(init, nz)
    own.trpo_update_end()
    assert own.score_policy_actions_grad(init, nz)['grad'].shape == (K, T, B, na)
    # the host method's own checks
    with pytest.raises(ValueError, match=r'init_obs: expected \[S, 10\]'):
        eng.score_policy_actions_grad(torch.zeros(S, ns + 1), nz)
    with pytest.raises(ValueError, match=r'noise: expected \[T, B, 2\] with B a multiple of 3'):
        eng.score_policy_actions_grad(torch.zeros(3, ns), nz)
    with pytest.raises(ValueError, match='want'):
        eng.score_policy_actions_grad(init, nz, want=('grad', 'hessian'))
    with pytest.raises(ValueError, match='chunk'):
        eng.score_policy_actions_grad(init, nz, chunk=-2)
    with pytest.raises(ValueError, match='needs T='):
        eng.score_policy_actions_grad(init)
    with pytest.raises(ValueError, match='gamma must be finite'):
        eng.score_policy_actions_grad(init, nz, gamma=float('inf'))
    one = eng.score_policy_actions_grad(torch.zeros(ns), nz)                               # [ns]: one start state; the default want
    assert set(one) == {'grad', 'ret'} and one['grad'].shape == (K, T, B, na)
    assert eng.score_policy_actions_grad(init, T=3)['grad'].shape == (K, 3, S, na)


# ---- 9. refine_noise and plan_cem_policy_gd on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aggregate', ['mean', ('pessimistic', 0.5)], ids=['mean', 'pessimistic'])
def test_refine_noise_and_plan_cem_policy_gd_on_the_device(aggregate, monkeypatch):
    from metrpo_amd import planning as P
    case = pick('fused', 'swimmer', B=33, T=11, stop=True)
    d = PC.case_data(case)
    eng = engine(case)
    S, N, T, lr, clip = 3, 11, case.T, 0.05, 2.0
    states = torch.as_tensor(d['init'], dtype=torch.float32, device=eng.device)
    n_dev = torch.as_tensor(d['noise'], dtype=torch.float32, device=eng.device)               # [T, S * N, na]
    cand = n_dev.reshape(T, S, N, -1).permute(1, 2, 0, 3).contiguous()
    kw = dict(gamma=case.gamma, aggregate=aggregate, noise_in_std=case.in_std)
    out = P.refine_noise(eng, states, cand, 1, lr, noise_clip=clip, optimizer='sgd', **kw)
    assert eng.last_score_policy_actions_grad_kernel() == 'fused'
    g = eng.score_policy_actions_grad(states, n_dev, gamma=case.gamma, noise_in_std=case.in_std, want=('grad', 'ret'))
    want = torch.clamp(n_dev + lr * P.aggregate_heads_grad(g['ret'], g['grad'], aggregate), -clip, clip)
    assert torch.equal(P._device_major(out['last']), want)                                    # bit for bit
    assert torch.equal(out['initial_score'].reshape(-1), P.aggregate_heads(g['ret'], aggregate))
    assert torch.all(out['score'] >= out['initial_score'])
    # no host read inside: Adam steps and a whole plan, nothing synchronised or read back until the caller does
    torch.cuda.synchronize()
    counts = dict(sync=0, item=0, cpu=0)
    real_sync, real_item, real_cpu = torch.cuda.synchronize, torch.Tensor.item, torch.Tensor.cpu

    def counted(key, fn):
        def wrapper(*a, **k2):
            counts[key] += 1
            return fn(*a, **k2)
        return wrapper
    monkeypatch.setattr(torch.cuda, 'synchronize', counted('sync', real_sync))
    monkeypatch.setattr(torch.Tensor, 'item', counted('item', real_item))
    monkeypatch.setattr(torch.Tensor, 'cpu', counted('cpu', real_cpu))
    adam = P.refine_noise(eng, states, cand, 3, lr, noise_clip=clip, **kw)
    gen = lambda: torch.Generator(device=eng.device).manual_seed(0)
    plans = [P.plan_cem_policy_gd(eng, states, 5, 16, 4, 2, grad_steps=2, grad_lr=lr, refine=rf, gamma=case.gamma, aggregate=aggregate, generator=gen())
             for rf in ('elites', 'all')]
    inside = dict(counts)
    torch.cuda.synchronize()
    assert inside == dict(sync=0, item=0, cpu=0) and counts['sync'] == 1
    monkeypatch.undo()
    assert torch.all(adam['score'] >= adam['initial_score']) and torch.isfinite(adam['noise']).all() and adam['noise'].abs().max() <= clip
    assert bool((adam['score'] > adam['initial_score']).any())                                # ascent: some candidate improved
    sc = P.score_noise_sequences(eng, states, adam['noise'], **kw)
    torch.testing.assert_close(sc, adam['score'], rtol=1e-5, atol=1e-5)                       # the kept iterate scores what was recorded
    pol = P.aggregate_heads(eng.score_policy_actions(states, None, T=5, gamma=case.gamma)['ret'], aggregate)
    plain = P.plan_cem_policy(eng, states, 5, 16, 4, 2, gamma=case.gamma, aggregate=aggregate, generator=gen())
    for plan in plans:
        assert torch.isfinite(plan['noise']).all() and torch.isfinite(plan['best_score']).all()
        assert torch.all(plan['best_score'] >= plan['policy_score'])                          # never below the policy under the scorer
        torch.testing.assert_close(plan['policy_score'], pol, rtol=1e-5, atol=1e-5)           # delta = 0 is the policy itself
        assert torch.all(plan['history'][0] >= plain['history'][0])                           # the same draws, refined before the refit: keep-best
    zero = P.plan_cem_policy_gd(eng, states, 5, 16, 4, 2, grad_steps=0, gamma=case.gamma, aggregate=aggregate, generator=gen())
    for k in plain:
        assert torch.equal(zero[k], plain[k]), k


# ---- 10. the controller with noise-gradient steps as a data-collection policy ------------------------------------------------------------------------------------
def test_example_loop_collects_with_noise_gradient_refined_shooting():
    """examples/me_trpo_loop.py --shooting --shooting-policy-prior --shooting-noise-grad-steps 1 at tests/test_gpu_score_actions.py's smallest settings,
    in a fresh child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import importlib.util, json, sys; sys.path.insert(0, %r);"
            "spec = importlib.util.spec_from_file_location('me_trpo_loop', %r); mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod);"
            "hist = mod.main(['--outer', '2', '--K', '3', '--T', '20', '--traj', '40', '--n-envs', '200', '--policy-iters', '6', '--model-passes', '6',"
            " '--quiet', '--shooting', '--shooting-policy-prior', '--shooting-noise-grad-steps', '1']);"
            "print('HIST ' + json.dumps([[float(h['n_data']), float(h['real_cost']), float(h['model_val']), float(h['est_cost'])] for h in hist]))"
            % (root, os.path.join(root, 'examples', 'me_trpo_loop.py')))
    res = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:]
    import json
    hist = json.loads(next(l for l in res.stdout.splitlines() if l.startswith('HIST '))[5:])
    assert len(hist) == 2 and hist[1][0] > hist[0][0] > 0 and np.isfinite(np.asarray(hist)).all()
