"""Head-split form of the cooperative rollout kernel (8 waves, two per SIMD, on one tile: rollout_coop_kernel.h) against the 4-wave form it
re-distributes.  Every (head, col-block) unit keeps its instruction order, its LDS slots and the four-term partial sum; only the wave that runs it
changes -- so every case runs the same rollout twice on one engine, set_coop_split(False) (4 waves) and set_coop_split(True) (8 waves), and compares every
output tensor byte for byte: obs, act, mean, rew, done, tpath, last_obs, last_ts, last_model.  No tolerance applies anywhere in this file."""
import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import helpers as Hh

pytestmark = pytest.mark.gpu

N_POOL = 257
FIELDS = ('obs', 'act', 'mean', 'rew', 'done', 'tpath', 'last_obs')
_ENGINES = {}


def _problem(env, K):
    """One engine per (env, K), shared by the cases (the comparison is between two launches of the same engine)."""
    key = (env, K)
    if key not in _ENGINES:
        eng, dm, theta, pdims, pool = Hh.make_engine(env, K, (64, 64), (32, 32), seed=11, n_pool=N_POOL)
        _ENGINES[key] = (eng, dm, torch.tensor(pool, dtype=torch.float32, device=eng.device))
    return _ENGINES[key]


def _supplied(dm, K, B, T, seed):
    d = Hh.draws(np.random.RandomState(seed), K, B, T, dm.ns, dm.na, N_POOL)
    return {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in d.items()}


def _run(eng, pool, B, T, H, mode, split, seed=5, supplied=None, chunks=None, determ=False):
    """-> dict of CPU tensors.  `chunks`: lengths summing to T, continued through resume (init_obs / init_ts / init_model) and t0."""
    eng.set_coop_split(split)
    dev = eng.device
    lts, lmd = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    parts, resume, t0 = [], None, 0
    for Tc in (chunks or (T,)):
        kw = {k: v[t0:t0 + Tc + (1 if k.startswith('reset') else 0)] for k, v in (supplied or {}).items()}
        tr = eng.rollout(B, Tc, H, mode, pool, determ=determ, seed=seed, t0=t0, resume=resume, last_state=(lts, lmd), **kw)
        assert eng.last_rollout_kernel() == 'mfma-cooperative', (eng.last_rollout_kernel(), eng.rollout_note())
        assert eng.last_coop_waves() == (8 if split else 4), eng.last_coop_waves()
        parts.append({k: getattr(tr, k).clone() for k in FIELDS})
        resume = (tr.last_obs.clone(), lts.clone(), lmd.clone())
        t0 += Tc
    assert t0 == T
    out = {k: torch.cat([q[k] for q in parts], 0).cpu() for k in FIELDS if k != 'last_obs'}
    out['last_obs'] = parts[-1]['last_obs'].cpu()
    out['last_ts'], out['last_model'] = lts.cpu(), lmd.cpu()
    eng.set_coop_split(True)
    return out


def _same(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k].view(torch.uint8) if a[k].dtype != torch.uint8 else a[k], b[k].view(torch.uint8) if b[k].dtype != torch.uint8 else b[k]), \
            '%s: %s differs between the 4-wave and the 8-wave form (%d elements)' % (what, k, int((a[k] != b[k]).sum()))


def _ab(env, K, B, T, H, mode, **kw):
    eng, dm, pool = _problem(env, K)
    four = _run(eng, pool, B, T, H, mode, False, **kw)
    eight = _run(eng, pool, B, T, H, mode, True, **kw)
    _same(four, eight, '%s K%d B%d T%d H%d %s' % (env, K, B, T, H, mode))
    assert torch.isfinite(eight['obs']).all() and torch.isfinite(eight['rew']).all()
    return four, eight


# tile edges: one env, one full tile, one tile + one env, two tiles + one env
@pytest.mark.parametrize('B', [1, 16, 17, 33])
def test_tile_edges(B):
    _ab('swimmer', 5, B, 5, 100, 'step_rand')


# head-group shapes 1+1, 1+2, 2+2, 2+3 on every env in scope, Philox draws; H = 3 with T = 7: horizon resets inside the launch
@pytest.mark.parametrize('K', [2, 3, 4, 5])
@pytest.mark.parametrize('env', ['swimmer', 'hopper', 'snake'])
def test_head_groups_every_env_with_resets(env, K):
    four, _ = _ab(env, K, 33, 7, 3, 'step_rand')
    assert int(four['done'].sum()) == 2 * 33


@pytest.mark.parametrize('mode', list(O.SAM_MODES))
def test_every_sampling_mode_philox(mode):
    _ab('snake', 5, 33, 7, 3, mode)


@pytest.mark.parametrize('mode', list(O.SAM_MODES))
def test_every_sampling_mode_supplied_draws(mode):
    """eps, model_idx, sel_noise, reset_idx and reset_model supplied: the DRAWS instantiations."""
    eng, dm, pool = _problem('hopper', 5)
    _ab('hopper', 5, 33, 7, 3, mode, supplied=_supplied(dm, 5, 33, 7, 21))


@pytest.mark.parametrize('env,K', [('swimmer', 5), ('swimmer', 3), ('snake', 4), ('hopper', 2)])
def test_supplied_draws_head_groups(env, K):
    eng, dm, pool = _problem(env, K)
    _ab(env, K, 17, 7, 3, 'model_mean_std', supplied=_supplied(dm, K, 17, 7, 22))


def test_deterministic_policy():
    _ab('swimmer', 5, 17, 5, 3, 'eps_rand', determ=True)


@pytest.mark.parametrize('supplied', [False, True])
@pytest.mark.parametrize('env', ['swimmer', 'hopper'])
def test_chunked_continuation_equals_one_call(env, supplied):
    """T = 3 then T = 4 through init_obs / init_ts / init_model (and t0) against one call of T = 7, on both forms."""
    eng, dm, pool = _problem(env, 5)
    sup = _supplied(dm, 5, 33, 7, 23) if supplied else None
    one4, one8 = _ab(env, 5, 33, 7, 3, 'eps_rand', supplied=sup)
    two4, two8 = _ab(env, 5, 33, 7, 3, 'eps_rand', supplied=sup, chunks=(3, 4))
    _same(one8, two8, 'chunked 8-wave'); _same(one4, two4, 'chunked 4-wave')


@pytest.mark.parametrize('T', [3, 7])
@pytest.mark.parametrize('short', [0, 15])
def test_migrating_tiles(T, short):
    """One tile more than CUs: the tile-steps are dealt out evenly, tiles change workgroups at different step offsets (hand-over slots in HBM), and
    with `short` the last tile is partial.  The bounded wait must not have given up: the sticky rollout error stays clear."""
    eng, dm, pool = _problem('swimmer', 5)
    if eng.get_option('NO_RESIDENT') is not None:
        pytest.skip('device shared with other compute processes: the launch rule does not select the migrating schedule')
    n_cu = eng.schedulable_cus()
    B = 16 * (n_cu + 1) - short
    _ab('swimmer', 5, B, T, 2, 'step_rand')
    eng.comm_check()                                                # raises if a hand-over wait timed out (scal[S_ROLLERR])
    assert eng.rollout_note() == ''


@pytest.mark.parametrize('env,K', [('swimmer', 1), ('ant', 5), ('half_cheetah', 5), ('hopper', 6)])
def test_out_of_scope_shapes_keep_the_4_wave_kernel(env, K):
    eng, dm, pool = _problem(env, K)
    eng.rollout(33, 3, 3, 'step_rand', pool, seed=1)
    assert eng.last_rollout_kernel() == 'mfma-cooperative' and eng.last_coop_waves() == 4


def test_switch_forces_the_4_wave_form_and_two_per_cu_is_untouched():
    eng, dm, pool = _problem('swimmer', 5)
    eng.rollout(33, 3, 3, 'step_rand', pool, seed=1)
    assert eng.last_coop_waves() == 8                               # the default wherever the rule launches one workgroup per CU
    eng.set_coop_split(False)
    eng.rollout(33, 3, 3, 'step_rand', pool, seed=1)
    assert eng.last_coop_waves() == 4
    eng.set_coop_split(True)
    eng.set_rollout_variant(2)                                      # two workgroups per CU: never the head-split form
    eng.rollout(33, 3, 3, 'step_rand', pool, seed=1)
    assert eng.last_coop_waves() == 4
    eng.set_rollout_variant(0)
    eng.rollout(33, 3, 3, 'step_rand', pool, seed=1)
    assert eng.last_coop_waves() == 8
