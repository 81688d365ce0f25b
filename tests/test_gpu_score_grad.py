"""GPU tests of metrpo_score_actions_grad (csrc/score_actions_grad.hip): the gradient of every head's predicted return with respect to supplied action
sequences, against the float64 restatement tests/score_grad_ref.py on the cases of tests/score_grad_cases.py (drawn clear of every relu / clip / cost /
done kink), between its two paths, against metrpo_score_actions, and under metrpo_amd.planning.refine_actions.

Bounds, all from tests/tolerances.py, none new:
  grad, lam0  per head rel-L2 <= BPTT_GRAD_REL_L2 (one-step 1e-5 x T <= 30 chained fp32 Jacobians: this chain), and per time step and per candidate by
              block_bound(BPTT_GRAD_REL_L2, block, whole), so one wrong step or row cannot hide in the whole;
  ret         sum_t gamma^t (atol + rtol |r_t|) with REWARD / LONG_RUN rows (tests/test_gpu_score_actions.py's rule); CROSS_KERNEL against score_actions;
  len         exact.
Worst shares observed are recorded in DESIGN.md section 1 (row f5g)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as Hh
import tolerances as TOL
import score_actions_ref as SA
import score_grad_cases as SC

pytestmark = pytest.mark.gpu

ROW = TOL.BPTT_GRAD_REL_L2
WANT = ('grad', 'ret', 'len', 'grad_mean', 'lam0')


def cpu(t):
    return t.detach().cpu().numpy()


_engines = {}


def engine(case):
    key = SC.shape_key(case)
    if key not in _engines:
        dm, theta, _, _ = SC.problem(case)
        _engines[key] = Hh.engine_of(case.env, case.K, case.dh, (32, 32), dm, theta, dyn_act=case.act)
    return _engines[key]


def fused_shape(case):
    return case.env in SC.FUSED_ENVS and len(case.dh) == 2 and max(case.dh) <= 64 and case.act == 'relu'


def run(case, d=None, force_generic=None, chunk=0, want=WANT, actions=None, init=None):
    d = SC.case_data(case) if d is None else d
    eng = engine(case)
    force = (case.path == 'generic') if force_generic is None else force_generic
    a_dev = torch.as_tensor(d['actions'] if actions is None else actions, dtype=torch.float32, device=eng.device)
    before = a_dev.clone()
    out = eng.score_actions_grad(np.asarray(d['init'] if init is None else init, np.float32), a_dev, gamma=case.gamma, stop_at_done=case.stop, want=want,
                                 force_generic=force, chunk=chunk)
    kernel = eng.last_score_actions_grad_kernel()
    assert kernel == ('fused' if (fused_shape(case) and not force) else 'generic')
    assert torch.equal(a_dev, before)                                                 # d_actions is never written
    return {k: cpu(v) for k, v in out.items()}


def head_order_mean(grad):
    """(sum_k grad_k) / K in fp32, summed in head order"""
    s = np.zeros(grad.shape[1:], np.float32)
    for k in range(grad.shape[0]):
        s = s + grad[k]
    return s / np.float32(grad.shape[0])


# ---- 1. either path against the restatement, at the tile and workgroup edges --------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.CASES, ids=[c.id for c in SC.CASES])
def test_against_the_restatement(case):
    """Worst shares observed over the table (MI355X): recorded in DESIGN.md row f5g."""
    d = SC.case_data(case)
    assert d['accepted'] == case.B
    ref = SC.reference(d)
    got = run(case, d)
    K, T, B = case.K, case.T, case.B
    dm = d['dm']
    assert got['grad'].shape == (K, T, B, dm.na) and got['lam0'].shape == (K, B, dm.ns) and got['grad_mean'].shape == (T, B, dm.na)
    use = SC.shares(got, ref, case)
    print("%s: grad %.3g whole, %.3g per step, %.3g per candidate; lam0 %.3g whole, %.3g per candidate; ret %.3g of their bounds" % ((case.id,) + tuple(use)))
    assert np.array_equal(got['len'], ref['len'])
    assert use.max() <= 1.0, use
    # exact zeros: a clipped action, and every step behind a candidate's last counted step
    clipped = np.abs(d['actions']) > 1
    assert np.all(got['grad'][:, clipped] == 0)
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


# ---- 2. Ant: what lies behind a candidate's end does not reach what lies in front of it ------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_ant_gradient_in_front_of_the_end_is_the_truncated_case(path):
    case = next(c for c in SC.CASES if c.path == path and c.variant == 'ant_plant' and c.T == 11)
    d = SC.case_data(case)
    ref = SC.reference(d)
    full = run(case, d)
    Tc = 6
    ended = ref['len'] <= Tc                                                          # [K, B]: over by step Tc
    assert ended.any() and (~ended).any() and ((ref['len'] > 1) & ended).any()
    trunc = run(case._replace(T=Tc), d, actions=d['actions'][:Tc])
    assert np.array_equal(trunc['len'][ended], full['len'][ended]) and np.array_equal(trunc['ret'][ended], full['ret'][ended])
    for k in range(case.K):
        b = np.flatnonzero(ended[k])
        assert np.array_equal(full['grad'][k][:Tc, b], trunc['grad'][k][:, b])        # bit for bit: zeros came back from behind the end
        assert np.all(full['grad'][k][Tc:, b] == 0)
        assert np.array_equal(full['lam0'][k][b], trunc['lam0'][k][b])


# ---- 3. ret / len are metrpo_score_actions' ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', [c.id for c in SC.CASES if c.T == 11 and c.dh == (64, 64)])
def test_ret_and_len_against_score_actions(cid):
    case = SC.BY_ID[cid]
    d = SC.case_data(case)
    ref = SC.reference(d)
    got = run(case, d, want=('grad', 'ret', 'len'))
    eng = engine(case)
    sa = eng.score_actions(np.asarray(d['init'], np.float32), np.asarray(d['actions'], np.float32), gamma=case.gamma, stop_at_done=case.stop,
                           want=('ret', 'len'), force_generic=case.path == 'generic')
    assert np.array_equal(got['len'], cpu(sa['len']))
    bnd = SA.bound(ref['rew'], case.gamma, lambda t: TOL.CROSS_KERNEL)
    print("%s: ret against score_actions uses %.3g of the bound" % (cid, float((np.abs(got['ret'] - cpu(sa['ret'])) / bnd).max())))
    assert np.all(np.abs(got['ret'].astype(np.float64) - cpu(sa['ret'])) <= bnd)


# ---- 4. chunking changes no bit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('env', ['swimmer', 'ant'])
def test_chunked_calls_equal_the_unchunked_call(path, env):
    case = next(c for c in SC.CASES if c.path == path and c.env == env and c.B == 33 and c.T == 11 and c.stop)
    whole = run(case)
    for chunk in (16, 17, 1000):
        part = run(case, chunk=chunk)
        for w in WANT:
            assert np.array_equal(whole[w], part[w]), (chunk, w)


# ---- 5. guard cells, oversized outputs, repeated calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('B', [17, 1])
def test_no_write_outside_the_outputs(path, B):
    """Each output sits in the middle of a larger allocation: G guard cells in front of it and a NaN (-77 for len) tail behind it stay put."""
    case = next(c for c in SC.CASES if c.path == path and c.env == 'swimmer' and c.B == B and c.K == 5)
    d = SC.case_data(case)
    eng = engine(case)
    dev = eng.device
    K, T, G = case.K, case.T, 7
    ns, na = d['dm'].ns, d['dm'].na
    n = {'grad': K * T * B * na, 'ret': K * B, 'len': K * B, 'grad_mean': T * B * na, 'lam0': K * B * ns}
    fill = lambda w: -77 if w == 'len' else float('nan')
    buf = {w: torch.full((G + n[w] + G,), fill(w), dtype=torch.int32 if w == 'len' else torch.float32, device=dev) for w in WANT}
    a_dev = torch.as_tensor(d['actions'], dtype=torch.float32, device=dev)
    init = np.asarray(d['init'], np.float32)
    force = path == 'generic'
    # `out` tensors larger than needed (the tail belongs to them): only the front is written
    out = eng.score_actions_grad(init, a_dev, gamma=case.gamma, want=WANT, force_generic=force, out={w: buf[w][G:] for w in WANT})
    plain = eng.score_actions_grad(init, a_dev, gamma=case.gamma, want=WANT, force_generic=force)
    again = eng.score_actions_grad(init, a_dev, gamma=case.gamma, want=WANT, force_generic=force)
    torch.cuda.synchronize()
    for w in WANT:
        edge = torch.cat([buf[w][:G], buf[w][G + n[w]:]])
        assert torch.all(edge == -77) if w == 'len' else torch.all(torch.isnan(edge)), w
        body = buf[w][G:G + n[w]]
        assert not torch.any(body == -77) if w == 'len' else not torch.any(torch.isnan(body)), w      # every cell of the output was written
        assert torch.equal(body, plain[w].reshape(-1)) and torch.equal(plain[w], again[w]), w         # repeated calls are bit-identical
        assert out[w].data_ptr() == buf[w][G:].data_ptr()


def test_a_small_call_after_a_large_one():
    small = next(c for c in SC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.B == 17 and c.K == 5)
    large = next(c for c in SC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.B == 33 and c.T == 11 and c.stop)
    assert SC.shape_key(small) == SC.shape_key(large)
    for force in (False, True):
        first = run(small, force_generic=force)
        run(large, force_generic=force)                                               # grows the workspace and leaves it full of another case's states
        second = run(small, force_generic=force)
        for w in WANT:
            assert np.array_equal(first[w], second[w]), w


# ---- 6. a call changes nothing else --------------------------------------------------------------------------------------------------------------------------
def test_a_score_actions_grad_call_changes_nothing_else():
    """The body of tests/test_gpu_score_actions.py::test_a_score_actions_call_changes_nothing_else, with the sibling reporters"""
    import test_gpu_model_error as TM
    _, dm, theta, pdims, pool, Os, As, Rs = TM.problem('swimmer')
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
    sibs = lambda: (eng.last_rollout_actions_kernel(), eng.last_disagreement_kernel(), eng.last_score_actions_kernel())
    assert sibs() == ('fused', 'generic', 'fused') and eng.last_score_actions_grad_kernel() is None
    for force in (False, True):
        eng.score_actions_grad(pool[:8].astype(np.float32), acts, gamma=0.99, want=WANT, force_generic=force)
        assert eng.last_score_actions_grad_kernel() == ('generic' if force else 'fused')
    torch.cuda.synchronize()
    after = state()
    for b, a in zip(before, after):
        assert torch.equal(b, a) if torch.is_tensor(b) else b == a
    assert eng.last_rollout_kernel() == kernel and eng.rollout_note() == note and sibs() == ('fused', 'generic', 'fused')
    t2 = roll()                                                                           # the Philox state: the same seed draws the same rollout
    assert torch.equal(o1, t2.obs) and torch.equal(r1, t2.rew) and torch.equal(a1, t2.act)


# ---- 7. the ABI's argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_errors():
    import metrpo_amd
    from metrpo_amd import _lib
    lib = _lib.lib
    case = next(c for c in SC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.K == 5)
    eng, dm = engine(case), SC.problem(case)[0]
    dev = eng.device
    B, T, S, K, ns, na = 4, 2, 2, dm.K, dm.ns, dm.na
    init, act = torch.zeros(S, ns, device=dev), torch.zeros(T, B, na, device=dev)
    grad = torch.full((K, T, B, na), 555.0, device=dev); gm = torch.full((T, B, na), 555.0, device=dev); lam = torch.full((K, B, ns), 555.0, device=dev)
    ret = torch.full((K, B), 555.0, device=dev); ln = torch.full((K, B), -55, dtype=torch.int32, device=dev)
    outs = (grad, gm, lam, ret)

    def args(**kw):
        a = _lib.ScoreActionsGradArgs()
        a.B, a.T, a.S, a.stop_at_done, a.gamma = B, T, S, 1, 0.99
        a.d_init_obs, a.d_actions, a.d_grad, a.d_ret, a.d_len, a.d_grad_mean, a.d_lam0 = (init.data_ptr(), act.data_ptr(), grad.data_ptr(), ret.data_ptr(),
                                                                                         ln.data_ptr(), gm.data_ptr(), lam.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.metrpo_score_actions_grad(eng._ctx, C.byref(a), eng._stream())
    err = lambda: lib.metrpo_last_error(eng._ctx)
    assert lib.metrpo_score_actions_grad(None, C.byref(args()), eng._stream()) == -2 and lib.metrpo_last_score_actions_grad_kernel(None) == -2
    assert lib.metrpo_score_actions_grad(eng._ctx, None, eng._stream()) == -2 and b'score_actions_grad: args NULL' in err()
    for name in ('d_init_obs', 'd_actions', 'd_grad'):
        assert call(args(**{name: None})) == -2 and b'score_actions_grad: required pointer' in err()      # METRPO_ENULL
    assert call(args(B=-1)) == -1 and b'score_actions_grad: bad B/T' in err()                              # METRPO_EINVAL
    assert call(args(T=-1)) == -1 and b'bad B/T' in err()
    for bad in (0, -1, 3):
        assert call(args(S=bad)) == -1 and b'must be at least 1 and divide B' in err()
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert call(args(gamma=bad)) == -1 and b'score_actions_grad: gamma is not finite' in err()
    assert call(args(chunk=-1)) == -1 and b'chunk must not be negative' in err()
    for kw in (dict(B=0), dict(T=0), dict(B=0, d_grad=None)):                            # B == 0 or T == 0: OK, nothing written
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert all(torch.all(t == 555.0) for t in outs) and torch.all(ln == -55)
    for kw in (dict(d_ret=None), dict(d_len=None), dict(d_grad_mean=None), dict(d_lam0=None), dict(d_ret=None, d_len=None, d_grad_mean=None, d_lam0=None),
               dict(force_generic=1, d_ret=None, d_lam0=None), dict(chunk=3), dict()):   # the optional outputs may be left out, each on its own
        assert call(args(**kw)) == 0
    torch.cuda.synchronize()
    assert not any(torch.any(t == 555.0) for t in outs) and not torch.any(ln == -55)
    # dynamics must be set, the policy need not be
    bare = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_score_actions_grad(bare._ctx, C.byref(args()), bare._stream()) == -5 and b'metrpo_set_dynamics' in lib.metrpo_last_error(bare._ctx)
    assert bare.last_score_actions_grad_kernel() is None
    bare.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    o2 = bare.score_actions_grad(init, act, gamma=0.99, want=WANT)                         # no metrpo_set_policy: theta is never read
    o1 = eng.score_actions_grad(init, act, gamma=0.99, want=WANT)
    for w in WANT:
        assert torch.equal(o1[w], o2[w])
    # the host method's own checks
    with pytest.raises(ValueError, match=r'init_obs: expected \[S, 10\]'):
        eng.score_actions_grad(torch.zeros(S, ns + 1), act)
    with pytest.raises(ValueError, match=r'actions: expected \[T, B, 2\] with B a multiple of 3'):
        eng.score_actions_grad(torch.zeros(3, ns), act)
    with pytest.raises(ValueError, match='want'):
        eng.score_actions_grad(init, act, want=('grad', 'hessian'))
    with pytest.raises(ValueError, match='chunk'):
        eng.score_actions_grad(init, act, chunk=-2)
    one = eng.score_actions_grad(torch.zeros(ns), act)                                     # [ns]: one start state; the default want
    assert set(one) == {'grad', 'ret'} and one['grad'].shape == (K, T, B, na)


# ---- 8. refine_actions on the device ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('aggregate', ['mean', ('pessimistic', 0.5)], ids=['mean', 'pessimistic'])
def test_refine_actions_on_the_device(aggregate, monkeypatch):
    from metrpo_amd import planning as P
    case = next(c for c in SC.CASES if c.path == 'fused' and c.env == 'swimmer' and c.B == 33 and c.T == 11 and c.stop)
    d = SC.case_data(case)
    eng = engine(case)
    S, N, T, lr = 3, 11, case.T, 0.05
    states = torch.as_tensor(d['init'], dtype=torch.float32, device=eng.device)
    a_dev = torch.as_tensor(d['actions'], dtype=torch.float32, device=eng.device)             # [T, S * N, na]
    cand = a_dev.reshape(T, S, N, -1).permute(1, 2, 0, 3).contiguous()
    out = P.refine_actions(eng, states, cand, 1, lr, optimizer='sgd', gamma=case.gamma, aggregate=aggregate)
    assert eng.last_score_actions_grad_kernel() == 'fused'
    g = eng.score_actions_grad(states, a_dev, gamma=case.gamma, want=('grad', 'ret'))
    want = torch.clamp(a_dev + lr * P.aggregate_heads_grad(g['ret'], g['grad'], aggregate), -1.0, 1.0)
    assert torch.equal(P._device_major(out['last']), want)                                    # bit for bit
    assert torch.equal(out['initial_score'].reshape(-1), P.aggregate_heads(g['ret'], aggregate))
    assert torch.all(out['score'] >= out['initial_score'])
    # no host read inside: three Adam steps, nothing synchronised or read back until the caller does
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
    adam = P.refine_actions(eng, states, cand, 3, lr, gamma=case.gamma, aggregate=aggregate)
    plan = P.plan_cem_gd(eng, states, 5, 16, 4, 2, grad_steps=2, grad_lr=lr, gamma=case.gamma, aggregate=aggregate,
                         generator=torch.Generator(device=eng.device).manual_seed(0))
    inside = dict(counts)
    torch.cuda.synchronize()
    assert inside == dict(sync=0, item=0, cpu=0) and counts['sync'] == 1
    monkeypatch.undo()
    assert torch.all(adam['score'] >= adam['initial_score']) and torch.isfinite(adam['actions']).all()
    assert bool((adam['score'] > adam['initial_score']).any())                                # ascent: some candidate improved
    sc = P.score_action_sequences(eng, states, adam['actions'], gamma=case.gamma, aggregate=aggregate)
    torch.testing.assert_close(sc, adam['score'], rtol=1e-5, atol=1e-5)                       # the kept iterate scores what was recorded
    assert torch.isfinite(plan['actions']).all() and torch.isfinite(plan['best_score']).all()


# ---- 9. the controller with gradient steps as a data-collection policy -------------------------------------------------------------------------------------------
def test_example_loop_collects_with_gradient_refined_shooting():
    """examples/me_trpo_loop.py --shooting --shooting-grad-steps 2 at tests/test_gpu_score_actions.py's smallest settings"""
    import importlib.util, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('me_trpo_loop', os.path.join(root, 'examples', 'me_trpo_loop.py'))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    hist = mod.main(['--outer', '2', '--K', '3', '--T', '20', '--traj', '40', '--n-envs', '200', '--policy-iters', '6', '--model-passes', '6',
                     '--quiet', '--shooting', '--shooting-grad-steps', '2'])
    assert len(hist) == 2 and hist[1]['n_data'] > hist[0]['n_data'] > 0
    assert all(np.isfinite([h['real_cost'], h['model_val'], h['est_cost']]).all() for h in hist)
