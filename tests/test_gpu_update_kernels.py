"""Every instantiation of the policy-update kernels (csrc/policy_mfma.hip: 5 environments x gradient / FVP / loss-KL / VPG / PPO; policy_fused3.hip;
the generic k_loss_grad / k_fvp / k_loss_kl of policy_update.hip at sample tiles 128, 64 and 32; the GEMM path policy_gemm.hip on widths it pads,
stacks and splits) against float64 at the tile edges: one lane, a partial tile, one tile, a tile plus one sample, more tiles than waves, two
blocks, the second half of the 7 : 6 tile deal; with no `valid` pointer, valid[::7] = 0, an invalid first / last sample and whole tile, and
exactly one valid sample; in the per-sample and the broadcast form of old_log_std.  Case table and references: tests/update_cases.py (checked on
the CPU by tests/test_update_cases.py).  Bounds: the rows LOSS_RTOL, KL_ATOL / KL_RTOL, GRAD_REL_L2, FVP_REL_L2 of tests/tolerances.py on the
whole vector, and tolerances.block_bound on every variable W_l, b_l, log_std of each gradient and FVP.
That a case runs on the kernel it names is asserted from what the library reports of its launches (Engine.last_update_launch), here and in
test_cases_reach_every_instantiation.  Out of scope: the Adam tails, the VJP; the cached FVP (OP_FVPC), the CG tails and the
line search are held by tests/test_gpu_trpo_solve.py, on the same case table.

Observed on an MI355X (worst share of each bound over the file, per family): profiles/r10_update_kernels.txt."""
import json
import os

import numpy as np
import pytest
import torch
import tolerances as TOL
import vpg_ref
import update_cases as U
from helpers import engine_of
from test_gpu_engine import rel_l2

pytestmark = pytest.mark.gpu
OPS = {0: 'grad', 1: 'fvp', 2: 'losskl', 3: 'fvpc', 4: 'vpg', 5: 'ppo'}        # UpdOp (csrc/metrpo_internal.h), as last_update_launch reports it
_ENGINES, _DERIVED, _LAUNCHES, _WORST = {}, {}, {}, {}


def cpu(t):
    return t.detach().cpu().numpy().astype(np.float64)


def engine_for(case, d):
    """One engine per (family, env, policy shape): the update kernels read only theta and the batch, so the cases share it and set their own theta."""
    key = (case.family, case.env, case.ph)
    if key not in _ENGINES:
        eng = engine_of(case.env, 2, (64, 64), case.ph, d['dm'], d['th'])
        path, expect = U.PATHS[case.family]
        assert eng.set_update_path(path) == path
        _ENGINES[key] = eng
    return _ENGINES[key]


def _probe_rows(eng, N):
    """Partial rows (= blocks) of a gradient launch on N samples, from the library's own report (the data do not matter: zeros)."""
    z = lambda *s: torch.zeros(*s, device=eng.device)
    eng.loss_grad(eng.make_batch(z(N, eng.ns), z(N, eng.na), z(N), z(N, eng.na), z(eng.na)))
    return eng.last_update_launch()['nrows']


def derive_n(case, eng):
    """The N of a symbolic case from reported launches, not from a copy of the launch rule."""
    if isinstance(case.nspec, int):
        return case.nspec
    key = (case.family, case.env, case.ph, case.nspec)
    if key in _DERIVED:
        return _DERIVED[key]
    kind, arg = case.nspec
    n = None
    if kind == 'full':                                      # generic kernels: 2 tiles of `arg` samples per CU and a partial one
        n = 2 * arg * torch.cuda.get_device_properties(eng.device).multi_processor_count + 3
    else:
        for tiles in range(2, 200):                         # N = 16 (tiles - 1) + 1: the smallest N of that tile count; its last tile is partial
            rows = _probe_rows(eng, 16 * (tiles - 1) + 1)
            if kind == 'two_blocks' and rows == 2:
                n = 16 * (tiles - 1) + 1; break
            # wave 4 of the last block starts at tile 4 (rows - 1) + 4 rows (k_policy_mfma: first_tile): it exists from 8 rows - 3 tiles on
            if kind == 'deal' and rows >= arg and tiles >= 8 * rows - 3:
                n = 16 * (tiles - 1) + 1; break
    assert n is not None and n <= 70000, (case.id, n)
    _DERIVED[key] = n
    return n


def run_ops(eng, d):
    """Every operation of the case on the device -> ({(op, log_std form): float64 array}, {op: reported launch})."""
    mk = lambda ls, valid: eng.make_batch(d['obs'], d['act'], d['adv'], d['om'], ls, valid=valid)
    out, rep = {}, {}
    eng.set_policy(d['th'])
    for form, ls in (('rows', d['ols']), ('bcast', d['ols'][0])):
        b = mk(ls, d['valid'])
        out['loss_grad', form] = cpu(eng.loss_grad(b)); rep['loss_grad'] = eng.last_update_launch()
        out['loss_kl_old', form] = cpu(eng.loss_kl(b)); rep['loss_kl_old'] = eng.last_update_launch()
        out['loss_kl_trial', form] = cpu(eng.loss_kl(b, d['th2'])); rep['loss_kl_trial'] = eng.last_update_launch()
        out['vpg', form] = cpu(eng.vpg_loss_grad(b)); rep['vpg'] = eng.last_update_launch()
        if form == 'rows':                                  # (reads no old distribution) a call of its own: the uncached OP_FVP
            out['fvp', form] = cpu(eng.fvp(b, d['v'])); rep['fvp'] = eng.last_update_launch()
    eng.set_policy(d['th2'])
    for form, ls in (('rows', d['ols']), ('bcast', d['ols'][0])):
        b = mk(ls, d['valid_ppo'])
        for i, ent in enumerate(U.ENT_COEFFS):
            out['ppo%d' % i, form] = cpu(eng.ppo_loss_grad(b, U.CLIP_LR, ent)); rep['ppo%d' % i] = eng.last_update_launch()
    torch.cuda.synchronize()
    return out, rep


def _note(family, row, share):
    """Worst share of each bound, per family; with METRPO_TOL_REPORT set also written next to the other reports."""
    _WORST.setdefault(family, {})
    _WORST[family][row] = max(_WORST[family].get(row, 0.0), float(share))
    if os.environ.get('METRPO_TOL_REPORT'):
        json.dump(_WORST, open(os.environ['METRPO_TOL_REPORT'] + '.update_kernels', 'w'), indent=1, sort_keys=True)


def _check_reports(case, rep):
    fam = {'mfma': 'mfma', 'fused3': 'fused3', 'generic': 'generic', 'gemm': 'gemm'}[case.family]
    want_op = {'loss_grad': 0, 'fvp': 1, 'loss_kl_old': 2, 'loss_kl_trial': 2, 'vpg': 4, 'ppo0': 5, 'ppo1': 5}
    for name, r in rep.items():
        assert r['family'] == fam and r['op'] == want_op[name], (case.id, name, r)


@pytest.mark.parametrize('case', U.CASES, ids=[c.id for c in U.CASES])
def test_update_kernels_match_float64(case):
    from metrpo_amd._lib import MetrpoError
    d0 = U.case_data(case, 1) if not isinstance(case.nspec, int) else None
    try:
        eng = engine_for(case, d0 or U.case_data(case))
    except MetrpoError as e:                                # a policy without a hidden layer may be refused, by name
        assert case.ph == () and str(e).split(':')[0] in ('unsupported configuration', 'invalid argument'), e
        return
    N = derive_n(case, eng)
    d = U.case_data(case, N)
    assert eng.update_path(N) == U.PATHS[case.family][1]
    assert d['removed'] <= U.CAP * d['n_valid'] and (N > 129 or d['removed'] == 0), (d['removed'], d['n_valid'])
    ref = U.references(d)
    out, rep = run_ops(eng, d)
    _LAUNCHES[case.id] = (N, rep)
    _check_reports(case, rep)
    fused = case.family in ('mfma', 'fused3')
    pd, fails = d['pdims'], []

    def hold(name, share, what=''):
        _note(case.family, name, share)
        print('%s %s%s: %.3g of the bound' % (case.id, name, what, share))
        if not share <= 1.0:
            fails.append((name, what, share))

    for form in ('rows', 'bcast'):
        for op in ('loss_grad', 'vpg', 'ppo0', 'ppo1'):
            got, (loss, g) = out[op, form], ref[op]
            hold('LOSS_RTOL', abs(got[0] - loss) / (TOL.LOSS_RTOL * max(1.0, abs(loss))), ' %s/%s' % (op, form))
            worst, where, whole = U.vector_use(got[1:], g, TOL.GRAD_REL_L2, pd)
            hold('GRAD_REL_L2', whole, ' %s/%s' % (op, form))
            hold('GRAD_REL_L2 per block', worst, ' %s/%s %s' % (op, form, where))
        for op in ('loss_kl_old', 'loss_kl_trial'):
            got, (loss, kl) = out[op, form], ref[op]
            hold('LOSS_RTOL', abs(got[0] - loss) / (TOL.LOSS_RTOL * max(1.0, abs(loss))), ' %s/%s' % (op, form))
            hold('KL', abs(got[1] - kl) / max(TOL.KL_ATOL, TOL.KL_RTOL * abs(kl)), ' %s/%s' % (op, form))
    worst, where, whole = U.vector_use(out['fvp', 'rows'], ref['fvp'], TOL.FVP_REL_L2, pd)
    hold('FVP_REL_L2', whole)
    hold('FVP_REL_L2 per block', worst, ' ' + where)
    rel_l2(out['loss_grad', 'rows'][1:], ref['loss_grad'][1])          # (the suite's own per-call-site report of the gradient figure)
    if fused:                                               # the broadcast form hoists the exponentials of old_log_std: the same fp32 values
        for op in ('loss_grad', 'loss_kl_old', 'loss_kl_trial', 'vpg', 'ppo0', 'ppo1'):
            assert np.array_equal(out[op, 'rows'], out[op, 'bcast']), (case.id, op)
    assert not fails, (case.id, N, fails)


@pytest.mark.parametrize('family', sorted(U.PATHS))
def test_clamped_log_std_slot_is_exactly_zero(family):
    """One log_std below log(1e-6): its VPG and PPO gradient entries are exactly 0.0 (no surrogate share, no entropy share), the others are not;
    the VPG gradient still matches its reference (the PPO ratios are meaningless at std = 1e-6, as in test_gpu_ppo.py)."""
    case = next(c for c in U.CASES if c.family == family and c.nspec == (65 if family == 'gemm' else 129) and c.mask == 'seven' and len(c.ph) > 1)
    d = U.case_data(case)
    eng = engine_for(case, d)
    na = d['pdims'][-1]
    th = d['th'].copy(); th[-na] = -20.0
    eng.set_policy(th)
    loss, g = vpg_ref.loss_grad(th, d['pdims'], d['obs'], d['act'], d['adv'], valid=d['valid'])
    assert g[-na] == 0.0
    for ls in (d['ols'], d['ols'][0]):
        b = eng.make_batch(d['obs'], d['act'], d['adv'], d['om'], ls, valid=d['valid'])
        got = cpu(eng.vpg_loss_grad(b))
        assert got[-na] == 0.0 and np.all(got[len(got) - na + 1:] != 0.0)
        assert abs(got[0] - loss) <= TOL.LOSS_RTOL * max(1.0, abs(loss))
        assert U.vector_use(got[1:], g, TOL.GRAD_REL_L2, d['pdims'])[0] <= 1.0
        for ent in U.ENT_COEFFS + (0.05,):
            got = cpu(eng.ppo_loss_grad(b, U.CLIP_LR, ent))
            assert got[-na] == 0.0


def test_cases_reach_every_instantiation():
    """From what the library reports of the launches of the table's cases (those test_update_kernels_match_float64 already made in this process;
    the others are launched here, without their references): every fused 2 x 32 kernel except the cached FVP, the generic kernels at each of
    their sample tiles, one and several partial rows in every family that has them, the GEMM path with one split and with more than 64."""
    from metrpo_amd._lib import MetrpoError
    seen = {}
    for case in U.CASES:
        if case.mask != 'none' and case.id not in _LAUNCHES:
            continue                                        # (the launch does not depend on the mask)
        if case.id not in _LAUNCHES:
            try:
                eng = engine_for(case, U.case_data(case, 1))
            except MetrpoError:
                continue
            N = derive_n(case, eng)
            _LAUNCHES[case.id] = (N, run_ops(eng, U.case_data(case, N))[1])
        N, rep = _LAUNCHES[case.id]
        _check_reports(case, rep)
        seen[case.id] = (case, N, rep)
    reps = [(c, N, name, r) for c, N, rep in seen.values() for name, r in rep.items()]
    fused = {(r['table'], r['op']) for c, N, name, r in reps if r['family'] == 'mfma'}
    assert fused == {(t, op) for t in range(len(U.FUSED_ENVS)) for op in (0, 1, 2, 4, 5)}, sorted(fused)
    for t, env in enumerate(U.FUSED_ENVS):                  # the table index belongs to the environment the case names
        assert {c.env for c, N, name, r in reps if r['family'] == 'mfma' and r['table'] == t} == {env}
    pts = {(c.ph, name.rstrip('01'), r['pt']) for c, N, name, r in reps if r['family'] == 'generic'}
    assert {pt for _, _, pt in pts} == {128, 64, 32}, sorted(pts)
    assert ((32, 32), 'fvp', 128) in pts and ((100, 50, 25), 'fvp', 64) in pts and ((256, 128), 'fvp', 32) in pts, sorted(pts)
    for fam in ('mfma', 'fused3', 'generic'):
        rows = {r['nrows'] for c, N, name, r in reps if r['family'] == fam}
        assert 1 in rows and max(rows) >= 2, (fam, sorted(rows))
    # the derived sizes: two blocks; waves 4 - 7 of one block and of each of two blocks own a tile
    for c, N, rep in seen.values():
        if c.nspec == ('two_blocks', 0):
            assert rep['loss_grad']['nrows'] == 2 and N % 16 != 0
        if isinstance(c.nspec, tuple) and c.nspec[0] == 'deal':
            assert rep['loss_grad']['nrows'] >= c.nspec[1] and (N + 15) // 16 >= 8 * rep['loss_grad']['nrows'] - 3 and N % 16 != 0
        if isinstance(c.nspec, tuple) and c.nspec[0] == 'full':
            assert rep['fvp']['nrows'] * rep['fvp']['pt'] * 1 < N and rep['fvp']['nrows'] >= 2
    gemm = [r for c, N, name, r in reps if r['family'] == 'gemm']
    assert any(r['splits'] == 1 for r in gemm) and any(r['splits'] > 64 for r in gemm), sorted({r['splits'] for r in gemm})
    assert all(r['kchunk'] % 16 == 0 and r['kchunk'] >= 16 for r in gemm)
    assert {len(c.ph) for c, N, name, r in reps if r['family'] == 'gemm'} >= {1, 2, 3, 4}
    print('reached:', json.dumps({f: sorted({(r['op'], r['table'], r['pt'], r['nrows'], r['splits'], r['kchunk']) for c, N, n, r in reps if r['family'] == f})
                                  for f in ('mfma', 'fused3', 'generic', 'gemm')}))
