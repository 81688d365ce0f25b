"""Subsampled Fisher-vector products ([rllab] ConjugateGradientOptimizer(subsample_factor < 1)): the device gather metrpo_subsample_batch, the
TRPO update with a separate FVP batch (metrpo_trpo_update_fvp / _fvp_begin) on every update family, and the optimiser that drives them.

Shapes: Swimmer 2 x 32 (fused MFMA and generic kernels) and Humanoid 100-50-25 (fused three-layer kernels and the GEMM path), N a few thousand;
sub-batch sizes m straddle each family's sample tile -- 16 for the two fused families (k_policy_mfma / k_f3_*: tiles of 16 samples), the PT the
library reports for the generic kernels (Engine.last_update_launch), 16 and 64 rows for the GEMM path's row tiles -- at 1, tile - 1, tile,
tile + 1 and several tiles plus a remainder.  Float64 side: tests/subsample_ref.py over the oracle's functions; bounds: tests/tolerances.py.
No test here sends an out-of-range index to the device; the gather's clamp is read on the CPU (tests/test_subsample_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import subsample_ref as R
from metrpo_amd.optimizer import ConjugateGradientOptimizer
from test_gpu_engine import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# family -> env, policy, set_update_path argument, the family Engine.last_update_launch names, N, seed of the data
FAMILIES = {'mfma': ('swimmer', (32, 32), True, 'mfma', 3001, 21), 'generic': ('swimmer', (32, 32), False, 'generic', 3001, 21),
            'fused3': ('humanoid', (100, 50, 25), True, 'fused3', 2003, 25), 'gemm': ('humanoid', (100, 50, 25), 'gemm', 'gemm', 2003, 25)}
M_UPDATE = {'mfma': 16 * 40 + 5, 'generic': 128 * 5 + 7, 'fused3': 16 * 40 + 5, 'gemm': 64 * 10 + 5}      # several tiles and a remainder
_DATA, _ENG = {}, {}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def data_of(family):
    env, ph, path, name, N, seed = FAMILIES[family]
    if (env, N, seed) not in _DATA:
        dm, th, pdims, obs, act, adv, om, ols = Hh.update_data(env, N, seed=seed, pol_hidden=ph)
        _DATA[env, N, seed] = dict(dm=dm, th=th, pdims=pdims, obs=obs, act=act, adv=adv, om=om, ols=ols, N=N)
    return _DATA[env, N, seed]


def engine_of(family):
    """One engine per family; every test sets theta itself."""
    env, ph, path, name, N, seed = FAMILIES[family]
    d = data_of(family)
    if family not in _ENG:
        eng = Hh.engine_of(env, 2, (64, 64), ph, d['dm'], d['th'])
        assert eng.set_update_path(path) == path
        _ENG[family] = eng
    _ENG[family].set_policy(d['th'])
    return _ENG[family], d


def batch_of(eng, d, ls='rows', valid=None, n_global=None, obs=None):
    return eng.make_batch(d['obs'] if obs is None else obs, d['act'], d['adv'], d['om'], d['ols'] if ls == 'rows' else d['ols'][0], valid=valid, n_global=n_global)


def tile_edges(family, eng, d):
    """m = 1, tile - 1, tile, tile + 1, several tiles + remainder, for every sample tile of the family."""
    if family == 'generic':
        eng.fvp(batch_of(eng, d), np.ones(eng.P))
        tiles = [eng.last_update_launch()['pt']]
        assert tiles[0] in (32, 64, 128)
    else:
        tiles = {'mfma': [16], 'fused3': [16], 'gemm': [16, 64]}[family]
    ms = {1}
    for t in tiles:
        ms |= {t - 1, t, t + 1, 5 * t + 3}
    return sorted(ms)


def index_vectors(N, m, seed):
    rng = np.random.RandomState(seed)
    rand = rng.permutation(N)[:m]
    dup = rng.randint(0, N, size=m); dup[m // 2:] = dup[:m - m // 2]              # duplicates (every index of the first half twice when m > 1)
    desc = np.sort(rng.permutation(N)[:m])[::-1].copy()
    return dict(random=rand, duplicates=dup, descending=desc)


# ---- 1. the gather is exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env', ['swimmer', 'humanoid'])
def test_gather_equals_index_select(env):
    family = 'mfma' if env == 'swimmer' else 'fused3'
    eng, d = engine_of(family)
    N = d['N']
    valid = np.ones(N, np.uint8); valid[::3] = 0
    t = lambda a, dt=torch.float32: torch.as_tensor(a, device=eng.device).to(dt)
    obs, om, ols, vt = t(d['obs']), t(d['om']), t(d['ols'] + np.arange(N)[:, None] * 1e-3), t(valid, torch.uint8)
    for m in (1, 255, 256, 257, 1500):                                           # the gather's own pass of 256 rows, and past it
        for kind, idx in index_vectors(N, m, 7 + m).items():
            it = torch.as_tensor(idx, device=eng.device).long()
            for ls_form, use_valid in (('rows', True), ('bcast', False)):
                src = eng.make_batch(obs, d['act'], d['adv'], om, ols if ls_form == 'rows' else ols[0], valid=vt if use_valid else None)
                sub = eng.subsample_batch(src, idx)
                got = eng.batch_tensors(sub)
                assert int(sub.N) == m and not sub.d_act and not sub.d_adv, (kind, m)
                assert torch.equal(got['obs'], obs.index_select(0, it)) and torch.equal(got['old_mean'], om.index_select(0, it)), (kind, m, ls_form)
                if ls_form == 'rows':
                    assert sub.old_log_std_stride == eng.na and torch.equal(got['old_log_std'], ols.index_select(0, it)), (kind, m)
                else:                                                            # a broadcast old_log_std stays the source's pointer
                    assert sub.old_log_std_stride == 0 and sub.d_old_log_std == src.d_old_log_std
                if use_valid:
                    want = vt.index_select(0, it)
                    assert torch.equal(got['valid'], want)
                    assert float(sub.valid_count.item()) == float(want.sum().item()) and sub.inv_n_global == 1.0 / float(want.sum().item())
                else:
                    assert not sub.d_valid and float(sub.valid_count.item()) == m and sub.inv_n_global == 1.0 / m
    eng.comm_check()                                                             # no index was clamped


def test_second_call_with_larger_m_grows_the_workspace():
    eng, d = engine_of('generic')
    src = batch_of(eng, d)
    obs = torch.as_tensor(d['obs'], device=eng.device).float()
    n0, _ = eng.retired_workspaces(sweep=True)
    small = eng.subsample_batch(src, np.arange(10))
    p_small = small.d_obs
    n1, _ = eng.retired_workspaces()
    big_idx = np.arange(d['N'])[::-1].copy()
    big = eng.subsample_batch(src, np.concatenate([big_idx, big_idx, big_idx]))       # m = 3 N: larger than any sub-batch of this engine before
    n2, _ = eng.retired_workspaces()
    assert n2 == n1 + 1 and big.d_obs != p_small                                 # outgrown, retired (not freed inside the entry point)
    it = torch.as_tensor(np.concatenate([big_idx, big_idx, big_idx]), device=eng.device).long()
    assert torch.equal(eng.batch_tensors(big)['obs'], obs.index_select(0, it))
    again = eng.subsample_batch(src, np.arange(10))                              # fits: same workspace, new contents
    assert again.d_obs == big.d_obs and eng.retired_workspaces()[0] == n2
    assert torch.equal(eng.batch_tensors(again)['obs'], obs[:10])


# ---- 2. FVP on the gathered sub-batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_fvp_on_gathered_rows(family):
    eng, d = engine_of(family)
    src = batch_of(eng, d)
    v = np.random.RandomState(3).randn(eng.P)
    fails = []
    for m in tile_edges(family, eng, d):
        idx = index_vectors(d['N'], m, 100 + m)['random']
        sub = eng.subsample_batch(src, idx)
        got = eng.fvp(sub, v).clone()
        rep = eng.last_update_launch()
        assert rep['family'] == FAMILIES[family][3] and rep['op'] == 1, rep                   # the uncached OP_FVP of the family
        ind = eng.make_batch(d['obs'][idx], d['act'][idx], d['adv'][idx], d['om'][idx], d['ols'][idx])     # built independently: index_select + make_batch
        assert torch.equal(got, eng.fvp(ind, v)), (family, m)                    # same kernel, same data, same order
        ref = O.fisher_vector_product(d['th'], d['pdims'], d['obs'][idx], v, reg_coeff=0.0)
        share = rel_l2(cpu(got), ref) / TOL.FVP_REL_L2
        print('%s m=%d FVP_REL_L2: %.3g of the bound' % (family, m, share))
        if not share <= 1.0:
            fails.append((m, share))
    assert not fails, (family, fails)


# ---- 3. fused update with fvp_batch == host loop == oracle ------------------------------------------------------------------------------------
def _check_update(out, ref, theta_new, d, what):
    g, dd = cpu(out['g']) if torch.is_tensor(out['g']) else out['g'], cpu(out['d']) if torch.is_tensor(out['d']) else out['d']
    assert rel_l2(g, ref['g']) <= TOL.GRAD_REL_L2, what
    cos = dd.dot(ref['d']) / (np.linalg.norm(dd) * np.linalg.norm(ref['d']))
    print('%s: cos defect %.3g, beta rel %.3g' % (what, 1 - cos, abs(out['beta'] - ref['beta']) / ref['beta']))
    assert cos >= TOL.CG_COS, (what, cos)
    assert abs(out['beta'] - ref['beta']) <= TOL.STEP_SCALE_RTOL * ref['beta'], what
    assert out['accepted'] == ref['accepted'] and out['n_backtrack'] == ref['n_backtrack'], (what, out['n_backtrack'], ref['n_backtrack'])
    assert abs(out['loss'] - ref['loss']) <= TOL.POST_UPDATE_RTOL * abs(ref['loss']) and abs(out['kl'] - ref['kl']) <= TOL.POST_UPDATE_RTOL * ref['kl'], what
    step_ref = ref['theta_new'] - d['th']
    assert rel_l2(theta_new - d['th'], step_ref) <= TOL.THETA_STEP_REL_L2, what


def _reference(family, idx, valid=None, obs=None):
    d = data_of(family)
    ref = R.cg_optimize_sub(d['th'], d['pdims'], d['obs'] if obs is None else obs, d['act'], d['adv'], d['om'], d['ols'], idx=idx, valid=valid)
    assert ref['accepted'] and ref['clear'], (family, ref['trials'], ref['loss_before'])      # the oracle alone accepts, away from every tie
    return ref


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_fused_update_equals_host_loop_and_oracle(family):
    eng, d = engine_of(family)
    idx = index_vectors(d['N'], M_UPDATE[family], 11)['random']
    ref = _reference(family, idx)
    batch = batch_of(eng, d, ls='bcast')
    theta0 = eng.get_policy().clone()
    runs = {}
    host = ConjugateGradientOptimizer(fused=False); host.update_opt(leq_constraint=(None, 0.01))
    runs['host'] = host.optimize(eng, batch, subsample_indices=idx)
    th_host = cpu(eng.get_policy())
    _check_update(runs['host'], ref, th_host, d, family + '/host')
    for name, kw in (('fused', {}), ('explicit', dict(explicit_final_hvp=True)), ('deferred', dict(spec_trials=2))):
        eng.set_policy(theta0)
        sub = eng.subsample_batch(batch, idx)
        out = eng.trpo_update(batch, max_kl=0.01, want_vectors=True, fvp_batch=sub, **kw)
        if name == 'deferred':
            assert out is None
            out = eng.trpo_update_end()
        th = cpu(eng.get_policy())
        _check_update(out, ref, th, d, family + '/' + name)
        # ... and the host loop over the same kernels: same accepted trial, the CG direction within the fused-vs-host figures
        dh, df = runs['host']['d'], cpu(out['d'])
        assert df.dot(dh) / (np.linalg.norm(df) * np.linalg.norm(dh)) >= TOL.CG_COS
        assert abs(out['beta'] - runs['host']['beta']) <= TOL.STEP_SCALE_RTOL * runs['host']['beta']
        assert out['n_backtrack'] == runs['host']['n_backtrack'] and out['accepted'] == runs['host']['accepted']
        assert abs(out['loss'] - runs['host']['loss']) <= TOL.POST_UPDATE_RTOL * abs(runs['host']['loss'])
        assert abs(out['kl'] - runs['host']['kl']) <= TOL.POST_UPDATE_RTOL * runs['host']['kl']
        runs[name] = out
    # the optimiser's own fused form routes to the same entry point
    eng.set_policy(theta0)
    opt = ConjugateGradientOptimizer(); opt.update_opt(leq_constraint=(None, 0.01))
    o = opt.optimize(eng, batch, subsample_indices=idx)
    assert o['beta'] == runs['fused']['beta'] and o['n_backtrack'] == runs['fused']['n_backtrack'] and o['kl'] == runs['fused']['kl']
    eng.comm_check()


# ---- 4. it really subsamples ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['mfma', 'generic'])
def test_subsampled_direction_differs_from_full_batch(family):
    """Half the rows' observations x 10 (old means and actions follow, so the batch is still one the policy produced), Hx on rows of that half only."""
    eng, d0 = engine_of(family)
    N = d0['N']
    obs = d0['obs'].copy(); obs[N // 2:] *= 10.0                                 # the Fisher matrix of the second half is another one
    obs = obs.astype(np.float32).astype(np.float64)
    om = O.policy_mean(d0['th'], d0['pdims'], obs).astype(np.float32).astype(np.float64)
    act = (om + (d0['act'] - d0['om'])).astype(np.float32).astype(np.float64)
    d = dict(d0, obs=obs, om=om, act=act)
    idx = N // 2 + np.random.RandomState(5).permutation(N - N // 2)[:M_UPDATE['mfma']]
    batch = batch_of(eng, d)
    theta0 = eng.get_policy().clone()
    full = eng.trpo_update(batch, max_kl=0.01, want_vectors=True)
    th_full = cpu(eng.get_policy())
    eng.set_policy(theta0)
    sub = eng.trpo_update(batch, max_kl=0.01, want_vectors=True, fvp_batch=eng.subsample_batch(batch, idx))
    th_sub = cpu(eng.get_policy())
    ref_full = R.cg_optimize_sub(d['th'], d['pdims'], obs, act, d['adv'], om, d['ols'], idx=None)
    ref_sub = R.cg_optimize_sub(d['th'], d['pdims'], obs, act, d['adv'], om, d['ols'], idx=idx)
    assert ref_full['accepted'] and ref_full['clear'] and ref_sub['accepted'] and ref_sub['clear']
    _check_update(full, ref_full, th_full, d, family + '/full')
    _check_update(sub, ref_sub, th_sub, d, family + '/sub')
    assert torch.equal(full['g'], sub['g'])                                      # the gradient sees the whole batch either way
    df, ds = cpu(full['d']), cpu(sub['d'])
    cos = df.dot(ds) / (np.linalg.norm(df) * np.linalg.norm(ds))
    assert 1.0 - cos > 100 * (1.0 - TOL.CG_COS), cos                             # far outside what CG_COS allows
    assert abs(full['beta'] - sub['beta']) > 100 * TOL.STEP_SCALE_RTOL * full['beta']
    # with a factor below 1 the optimiser draws for itself, reproducibly from its seed
    betas = []
    for _ in range(2):
        eng.set_policy(theta0)
        opt = ConjugateGradientOptimizer(subsample_factor=0.25, seed=9); opt.update_opt(leq_constraint=(None, 0.01))
        betas.append(opt.optimize(eng, batch)['beta'])
    assert betas[0] == betas[1] and betas[0] != full['beta']


# ---- 5. the default path is untouched -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_without_a_sub_batch_the_update_is_todays(family):
    import ctypes as C
    from metrpo_amd import _lib
    eng, d = engine_of(family)
    batch = batch_of(eng, d)
    theta0 = eng.get_policy().clone()
    base = eng.trpo_update(batch, max_kl=0.01, want_vectors=True)
    th_base, last_base = eng.get_policy().clone(), eng.last_update_launch()

    def same(out, what):
        assert torch.equal(eng.get_policy(), th_base) and torch.equal(out['g'], base['g']) and torch.equal(out['d'], base['d']), what
        for k in ('loss_before', 'loss', 'kl', 'beta', 'n_backtrack', 'accepted', 'cg_iters_run'):
            assert out[k] == base[k], (what, k)
        assert eng.last_update_launch() == last_base, what

    p = _lib.TrpoParams()
    p.max_kl, p.cg_iters, p.reg_coeff, p.backtrack_ratio, p.max_backtracks, p.residual_tol = 0.01, 10, 1e-5, 0.8, 15, 1e-10
    for fvp in (None, batch):                                                    # NULL and the batch itself through the new entry point
        eng.set_policy(theta0)
        diag = _lib.TrpoDiag()
        g = torch.empty(eng.P, dtype=torch.float64, device=eng.device); dd = torch.empty_like(g)
        eng._chk(_lib.lib.metrpo_trpo_update_fvp(eng._ctx, C.byref(batch), C.byref(fvp) if fvp is not None else None, C.byref(p), C.byref(diag),
                                                 C.c_void_p(g.data_ptr()), C.c_void_p(dd.data_ptr()), eng._stream()))
        same(dict(g=g, d=dd, loss_before=diag.loss_before, loss=diag.loss, kl=diag.kl, beta=diag.beta, n_backtrack=diag.n_backtrack,
                  accepted=bool(diag.accepted), cg_iters_run=diag.cg_iters_run), 'fvp_batch=%s' % ('NULL' if fvp is None else 'batch'))
    eng.set_policy(theta0)
    opt = ConjugateGradientOptimizer(subsample_factor=1.0); opt.update_opt(leq_constraint=(None, 0.01))
    o = opt.optimize(eng, batch)
    assert torch.equal(eng.get_policy(), th_base) and o['beta'] == base['beta'] and o['kl'] == base['kl']
    if family != 'gemm':                                                         # launch count: cg_iters product kernels, as before
        eng.set_policy(theta0); eng.set_option('TIME_FVP', '1')
        try:
            eng.trpo_update(batch, max_kl=0.01)
        finally:
            eng.set_option('TIME_FVP', None)
        assert eng.fvp_kernel_us()[1] == 10


# ---- 6. sharded ---------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_subsample_their_own_shares(tmp_path):
    """2 processes on cuda:0 (3 with this one) over the one-shot exchange: each rank gathers its own rows of its half; theta is bit-identical on both
    (asserted by the helper) and within MULTI_RANK_THETA of one rank whose fvp_batch is the two sub-batches in rank order."""
    out_file = str(tmp_path / 'sub_ranks.npz')
    world, port = 2, 29641
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(HERE, '_two_rank_subsample.py'), out_file]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY='0')
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
             for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=330)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    assert all(pr.returncode == 0 for pr in procs), '\n'.join(l[-3000:] for l in logs)
    many = np.load(out_file)
    eng, d = engine_of('mfma')
    N = d['N'] - 1                                                               # (an even N: two equal shares)
    idx = np.concatenate([rank_indices(N, 0), N // 2 + rank_indices(N, 1)])
    sl = slice(0, N)
    batch = eng.make_batch(d['obs'][sl], d['act'][sl], d['adv'][sl], d['om'][sl], d['ols'][0])
    one = eng.trpo_update(batch, max_kl=0.01, want_vectors=True, fvp_batch=eng.subsample_batch(batch, idx))
    th = cpu(eng.get_policy())
    assert int(many['n_backtrack']) == one['n_backtrack'] and bool(many['accepted']) and one['accepted']
    assert abs(float(many['beta']) - one['beta']) <= TOL.STEP_SCALE_RTOL * one['beta']
    step = np.abs(th - d['th']).max()
    np.testing.assert_allclose(many['theta'], th, rtol=0, atol=TOL.MULTI_RANK_THETA * step + 1e-7)


def rank_indices(N, rank):
    """The rows rank `rank` draws from its share of N // 2 samples (shared with tests/_two_rank_subsample.py)."""
    return np.random.RandomState(40 + rank).permutation(N // 2)[:16 * 20 + 3]


# ---- 7. masked batch ----------------------------------------------------------------------------------------------------------------------------
def test_masked_ant_batch_uses_the_gathered_valid_count():
    N, m = 2500, 16 * 30 + 7
    dm, th, pdims, obs, act, adv, om, ols = Hh.update_data('ant', N, seed=27)
    eng = Hh.engine_of('ant', 2, (64, 64), (32, 32), dm, th)
    assert eng.set_update_path(True) is True
    valid = np.ones(N, np.uint8); valid[::5] = 0; valid[-40:] = 0                # unfinished paths at the end of the batch, as the sampler leaves them
    keep = valid.astype(bool)
    adv = adv.copy(); adv[keep] = O.center_advantages(adv[keep]); adv = adv.astype(np.float32).astype(np.float64)
    idx = np.random.RandomState(8).permutation(N)[:m]
    assert 0 < keep[idx].sum() < m
    ref = R.cg_optimize_sub(th, pdims, obs, act, adv, om, ols, idx=idx, valid=valid)
    assert ref['accepted'] and ref['clear'] and ref['n_fvp_rows'] == int(keep[idx].sum())
    batch = eng.make_batch(obs, act, adv, om, ols[0], valid=valid)
    d = dict(th=th)
    for fused in (True, False):
        eng.set_policy(th)
        opt = ConjugateGradientOptimizer(fused=fused); opt.update_opt(leq_constraint=(None, 0.01))
        out = opt.optimize(eng, batch, subsample_indices=idx)
        if fused:                                                                # (the fused form reports no vectors through the optimiser: take them from the engine)
            eng.set_policy(th)
            sub = eng.subsample_batch(batch, idx)
            assert sub.inv_n_global == 1.0 / float(keep[idx].sum())
            out = eng.trpo_update(batch, max_kl=0.01, want_vectors=True, fvp_batch=sub)
        _check_update(out, ref, cpu(eng.get_policy()), d, 'ant/' + ('fused' if fused else 'host'))
    with pytest.raises(ValueError, match='valid'):
        eng.subsample_batch(batch, np.arange(0, N, 5)[:50])                      # only invalid rows


# ---- 8. from a params file, through the inner loop -------------------------------------------------------------------------------------------------
def test_from_params_runs_the_inner_loop_with_a_subsample_factor():
    import json
    import metrpo_amd
    from metrpo_amd import early_stop
    p = json.load(open(os.path.join(HERE, 'golden', 'params_swimmer.json')))
    p['n_models'] = 2
    p['dynamics_model']['hidden_layers'] = [64, 64]
    po = p['policy_opt_params']
    po.update(T=10, log_every=1, max_iters=3, num_iters_threshold=2)
    po['trpo'].update(batch_size=1000, subsample_factor=0.1)
    s = metrpo_amd.from_params(p, seed=3)
    opt = s.algo.optimizer
    assert isinstance(s.algo, metrpo_amd.TRPO) and opt._subsample_factor == 0.1 and s.shapes['trpo_ext'] == dict(subsample_factor=0.1)
    dm, _, _, pool = O.make_problem('swimmer', K=2, dyn_hidden=(64, 64), pol_hidden=(32, 32), seed=4)
    s.engine.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    theta0 = s.engine.get_policy().clone()
    out = early_stop.optimize_policy(s.algo, pool[:50].astype(np.float32), **dict(s.optimize_policy_kwargs, mode='no_early', max_iters=2))
    d = opt.last_diag
    assert out is not None and d is not None and np.isfinite(d['loss_before']) and np.isfinite(d['beta'])
    assert opt._gen is not None and opt._gen.device.type == 'cuda'                # the draw was made on the device
    assert not torch.equal(s.engine.get_policy(), theta0) or not d['accepted']
    s.engine.comm_check()
