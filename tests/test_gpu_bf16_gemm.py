"""The bf16 layer GEMM and its weight image (csrc/rollout_bf16.hip) on their own, through the diagnostics hook Engine.debug_gemm_bf16: all six
k_gemm_bf16<A type, C type, BN> instantiations at the edges of their tiling -- rows, columns, the k tiles, the pad columns of a bf16 output, the
col >= ldc skip of the 128-column tile -- every activation, one X for all heads and one per head, lda > Kp, the pick rule on both sides of its CU-count
threshold, and k_bf16_wimage read back bit for bit (bf16_gemm_cases.py holds the table and the float64 side; test_bf16_gemm_cases.py checks both on the CPU).

Per case: the form the library reports equals the Python restatement of the rule and the grid; on dyadic operands an f32 output equals the float64
result and a bf16 output bf16_round of it BIT FOR BIT, tanh excepted (the project's allowance for one tanh layer, TOL.STEP['atol'], after the identity
form gave the exact pre-activation on the same operands); on fp32 normals |got - ref| <= (n + 2) u (|A| @ |W| + |bias|) per cell for an f32 output and
bf16_round(ref - bound) <= got <= bf16_round(ref + bound) for a bf16 one; pad columns hold 0x0000; no cell outside the stated output is written, every
cell inside is; the operands are left as they were; a second call returns the same bits.  pytest -s prints the worst share of the float bound per group."""
import numpy as np
import pytest
import torch
import helpers as Hh
import bf16_gemm_cases as G

pytestmark = pytest.mark.gpu

BY_GROUP = G.cases_by_group()
GROUPS = sorted(BY_GROUP) + ['threshold']


@pytest.fixture(scope='module')
def eng():
    return Hh.make_engine('swimmer', 3, (64, 64), (32, 32), seed=3)[0]


@pytest.fixture(scope='module')
def n_cu(eng):
    c = G.IMAGE_CASES[0]
    return run(eng, c, G.build(c))[0]['n_cu']


def _raw(a):
    return a.view(np.int16) if a.dtype == np.uint16 else a


def run(eng, c, p):
    """one call on fresh device copies of p.bufs -> (reported form, C as the array type of p.bufs['C'], operands unchanged)"""
    dev = dict((n, torch.from_numpy(_raw(b)).to(eng.device)) for n, b in p.bufs.items())
    form = eng.debug_gemm_bf16(c.op, **dict(G.device_fields(c, p), **dev))
    torch.cuda.synchronize()
    same = all(np.array_equal(ubits(dev[n].cpu().numpy()), ubits(_raw(b))) for n, b in p.bufs.items() if n != 'C')      # (bits: the gaps hold NaN)
    return form, dev['C'].cpu().numpy().view(p.bufs['C'].dtype), same


def ubits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check(eng, c, n_cu):
    """-> (reported form, worst share of the f32 float bound, cells of a bf16 float output off bf16_round(ref), cells held to an interval)"""
    what = G.case_id(c)
    p = G.build(c)
    e = G.expect(c, p)
    form, got, same = run(eng, c, p)
    assert form == G.want_form(c, n_cu), what
    assert same, what + ': an operand was written'
    init = p.bufs['C']
    cell = got[e.idx]
    miss = e.idx[ubits(cell) == ubits(init[e.idx])]
    assert miss.size == 0, '%s: %d of %d cells not written, flat indices %s ..' % (what, miss.size, e.idx.size, miss[:8])
    outside = np.ones(got.size, bool); outside[e.idx] = False
    assert np.array_equal(ubits(got)[outside], ubits(init)[outside]), what + ': written outside the output'
    share, off = 0.0, 0
    if c.op == 'image':
        assert np.array_equal(cell, e.val), '%s: %d of %d cells differ' % (what, (cell != e.val).sum(), cell.size)
    else:
        bf = c.ct == 'bf16'
        x = (G.from_bits16(cell) if bf else cell).astype(np.float64)
        if bf:
            assert not np.any(cell[e.pad]), what + ': a pad column is not 0x0000'
        if e.exact:
            want = G.bits16(e.val.astype(np.float32)) if bf else e.val.astype(np.float32).view(np.uint32)
            assert np.array_equal(ubits(cell), want), '%s: %d of %d cells differ from the exact result, worst %g' % (
                what, (ubits(cell) != want).sum(), cell.size, np.nanmax(np.abs(x - e.val)))
        else:
            beyond = ~((x >= e.lo) & (x <= e.hi))
            real = ~e.pad
            if bf:      # a cell off bf16_round(ref): the device's f32 value lay across the rounding boundary between the two, at least that far from ref
                r = G.bf16_round(e.centre.astype(np.float32)).astype(np.float64)
                moved = real & (x != r)
                off = int(moved.sum())
                share = float((np.abs((x + r) / 2 - e.centre)[moved] / e.bound[moved]).max()) if off else 0.0
            else:
                share = float((np.abs(x - e.centre)[real] / e.bound[real]).max())
            print('    %s: worst share of the bound %.3f%s' % (what, share, ' (%d of %d cells off bf16_round(ref))' % (off, real.sum()) if bf else ''))
            assert not beyond.any(), '%s: %d of %d cells beyond the bound, worst |got - ref| %g' % (what, beyond.sum(), x.size, np.nanmax(np.abs(x - e.centre)))
            if c.kind != 'float':
                share = 0.0                                            # (tanh: the share of an allowance, not of a derived bound)
    form2, again, _ = run(eng, c, p)
    assert form2 == form and np.array_equal(ubits(again), ubits(got)), what + ': a second call differs'
    return form, share, off, (0 if e.exact else int((~e.pad).sum()))


_RAN = {}


def ran(eng, n_cu, group):
    """the cases of a group, run once per module: [(case, reported form, share, off, n)]"""
    if group not in _RAN:
        out = []
        for c in (G.threshold_cases(n_cu) if group == 'threshold' else BY_GROUP[group]):
            if c.op == 'gemm' and c.act == 2:      # the exact pre-activation first, on the same operands and the same tile
                check(eng, c._replace(act=0), n_cu)
            out.append((c, ) + check(eng, c, n_cu))
        _RAN[group] = out
    return _RAN[group]


@pytest.mark.parametrize('group', GROUPS)
def test_group_against_float64(eng, n_cu, group):
    res = ran(eng, n_cu, group)
    fl = [r for r in res if r[0].kind == 'float']
    print('%s: %d cases; float: worst share of the bound %.3f, %d of %d bf16 cells off bf16_round(ref)' % (
        group, len(res), max([r[2] for r in fl] or [0.0]), sum(r[3] for r in fl), sum(r[4] for r in fl if r[0].ct == 'bf16')))


def test_cases_reach_every_instantiation(eng, n_cu):
    reached = set()
    for group in GROUPS:
        for r in ran(eng, n_cu, group):
            c, form = r[0], r[1]
            if c.op == 'gemm':
                reached.add((c.at, c.ct, form['bn'], 'rule' if c.bn == 0 else 'forced'))
    assert {k[:3] for k in reached if k[3] == 'forced'} == {(at, ct, bn) for at, ct in G.PAIRS for bn in (64, 128)}
    lo, hi = ran(eng, n_cu, 'threshold')
    assert lo[0].bn == 0 and hi[0].bn == 0 and lo[1]['gx'] * lo[1]['gy'] * lo[1]['gz'] // 2 == n_cu - 1 and hi[1]['gx'] * hi[1]['gy'] * hi[1]['gz'] == n_cu
    assert (lo[1]['bn'], hi[1]['bn']) == (64, 128)                   # both outcomes of the rule, one tile apart
    rule = {(c.N, form['bn']) for g in ('f32-bf16-rule64', 'bf16-f32-rule64') for c, form in (r[:2] for r in ran(eng, n_cu, g))}
    assert rule == {(64, 64), (65, 64)}
    assert ('f32', 'bf16', 128, 'rule') in reached and ('f32', 'bf16', 64, 'rule') in reached and ('bf16', 'f32', 64, 'rule') in reached


def test_rejects_what_launch_bf16_layers_does_not_pass(eng):
    from metrpo_amd._lib import MetrpoError
    f = torch.zeros(4096, device=eng.device)
    h = torch.zeros(8192, dtype=torch.int16, device=eng.device)
    l0 = dict(a_bf16=0, c_bf16=1, bn=0, M=4, N=8, Kd=8, Kp=64, heads=1, lda=8, ldc=64, act=1, sA=0, sW=512, sB=8, sC=256, A=f, W=h, bias=f, C=h)
    mid = dict(l0, a_bf16=1, Kd=64, lda=64, A=h)
    out = dict(mid, c_bf16=0, ldc=8, C=f)
    assert eng.debug_gemm_bf16('gemm', **l0)['bn'] == 64 and eng.debug_gemm_bf16('gemm', **mid)['bn'] == 64 and eng.debug_gemm_bf16('gemm', **out)['bn'] == 64
    for base, kw in ((l0, dict(c_bf16=0, ldc=8, C=f)),                 # (f32, f32) is not instantiated
                     (l0, dict(Kd=4)), (l0, dict(lda=6, Kd=6)), (l0, dict(sA=34)), (l0, dict(Kp=128)), (l0, dict(ldc=8)), (l0, dict(ldc=128)),
                     (l0, dict(act=3)), (l0, dict(act=-1)), (l0, dict(bn=32)), (l0, dict(bn=128)), (l0, dict(M=0)), (l0, dict(N=0)), (l0, dict(heads=0)),
                     (l0, dict(Kp=72)), (l0, dict(sW=516)), (l0, dict(bias=None)), (l0, dict(A=None)),
                     (mid, dict(lda=56)), (mid, dict(lda=68)), (mid, dict(Kd=8)), (mid, dict(sA=4)), (out, dict(ldc=64)), (out, dict(a_bf16=2))):
        with pytest.raises(MetrpoError, match='debug_gemm_bf16'):
            eng.debug_gemm_bf16('gemm', **dict(base, **kw))
    img = dict(N=8, Kd=8, Kp=64, heads=1, sW=64, sC=512, W=f, C=h)
    assert eng.debug_gemm_bf16('image', **img) == dict(bn=0, gx=2, gy=1, gz=1, n_cu=eng.debug_gemm_bf16('gemm', **l0)['n_cu'])
    for kw in (dict(Kp=128), dict(Kp=32), dict(Kd=0), dict(N=0), dict(heads=0), dict(sW=-1), dict(W=None), dict(C=None)):
        with pytest.raises(MetrpoError, match='debug_gemm_bf16'):
            eng.debug_gemm_bf16('image', **dict(img, **kw))
    with pytest.raises(MetrpoError, match='unknown op'):
        eng.debug_gemm_bf16(2, **img)
    torch.cuda.synchronize()


def test_hook_leaves_the_context_alone():
    eng, dm, theta, pdims, pool = Hh.make_engine('half_cheetah', 3, (128, 128), (32, 32), seed=3)
    gen = torch.Generator(device=eng.device).manual_seed(7)
    rnd = lambda *s: torch.rand(*s, generator=gen, device=eng.device)
    eng.set_train_adam(rnd(eng.K, eng.dyn_param_count) - 0.5, rnd(eng.K, eng.dyn_param_count), 5)
    eng.set_policy_adam(rnd(eng.P) - 0.5, rnd(eng.P), 9)
    eng.set_dyn_precision('bf16')
    rng = np.random.RandomState(1)
    B, T, H = 32, 2, 2
    kw = dict(eps=rng.randn(T, B, dm.na), model_idx=rng.randint(eng.K, size=(T, B)), reset_idx=rng.randint(len(pool), size=(T + 1, B)),
              reset_model=rng.randint(eng.K, size=(T + 1, B)))
    def roll():
        tr = eng.rollout(B, T, H, 'step_rand', pool, **kw)
        return [x.clone() for x in (tr.obs, tr.act, tr.rew, tr.last_obs)]
    first = roll()
    assert eng.last_rollout_kernel() == 'gemm-bf16' and eng.last_bf16_layers() == [64, 64, 64]

    def state():
        m, v, t = eng.get_train_adam()
        pm, pv, pt = eng.get_policy_adam()
        return ([eng.get_policy(), eng.get_dynamics(), m, v, pm, pv],
                (t, pt, eng.last_rollout_kernel(), eng.rollout_note(), eng.last_bf16_layers(), eng.dyn_precision, eng.retired_workspaces(), eng.last_rollout_launch()))
    before, scalars = state()
    for c in (G.gemm_case('f32', 'bf16', 128, 129, 136, K=20, heads=3, seed=1), G.gemm_case('bf16', 'f32', 0, 33, 65, K=100, Kp=128, heads=3, seed=2),
              G.image_case(65, 33, 3, 3)):
        run(eng, c, G.build(c))
    after, scalars2 = state()
    assert scalars2 == scalars
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert all(torch.equal(x, y) for x, y in zip(first, roll()))      # ... and the context's own image and workspaces serve the next rollout as before
