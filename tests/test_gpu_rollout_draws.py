"""Production draws of every rollout kernel family against the documented Philox stream (csrc/device_common.h), restated in NumPy by
tests/rollout_draws_ref.py.  Every case runs Engine.rollout with NO draw tensor (or with exactly one withheld: the mixed mode of metrpo.h), builds
the restated draws of the same (seed, stream_offset, t0) and checks, against the device's trajectory,
  * pool rows, bit for bit: obs[0] and the state behind every done[t, b] are the rows reset_idx names (pool of 1000 distinct rows: no power of two);
  * heads: last_model is the cur_model the restated reset_model implies; done / tpath are the oracle's (free-running for horizon-terminated envs);
  * normals: z = (act - mean) / exp(log_std) against the restated eps within TOL.PHILOX_NORMAL;
  * the step, teacher-forced: helpers.oracle_rollout on the restated draws and the device's observations -> mean, act, rew, next state within the
    family's row of tests/tolerances.py (STEP, WIDE from 128 hidden units).  The comparison itself is tests/rollout_check.py (_device_run, _check).  The K heads of make_problem differ by ~1e-2: a wrong step_rand / eps_rand
    head, a wrong noise chunk or a swapped sine is off by orders.

Widening of the step tolerances by the draws' own error (the device's Box-Muller uses __logf / __sincosf): a normal may be off by PHILOX_NORMAL, so
act by PHILOX_NORMAL exp(log_std) -- the multiplier the oracle applies.  That action error reaches the next state and the reward through the clip
(1-Lipschitz) and the dynamics, whose Jacobian with respect to the action has norm < 1 on the fixtures (output layer x 0.1, diff_std ~ 0.1), and the
rewards' control costs (coefficients <= 0.1): the same figure is added to both.  model_mean_std adds PHILOX_NORMAL x the heads' standard deviation
to the next state.  Where the restated radius is below 2^-6 (left out of the normals check; at most 1e-3 of a case's normals) the addition grows as
2^-6 / r, as the error does.  Nothing is added where the draw was supplied or the policy is deterministic."""
import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import helpers as Hh
import tolerances as TOL
import rollout_draws_ref as R
from rollout_check import _device_run, _check              # the comparison itself: shared with tests/test_gpu_rollout_edges.py

pytestmark = pytest.mark.gpu

N_POOL = 1000
HUMANOID_POL = (100, 50, 25)


def seed_of(i):
    """64-bit seeds with both halves non-zero (the key's high word is seed >> 32)."""
    return ((0x9E3779B9 + 7919 * i) << 32) | (0x7F4A7C15 + 977 * i)


class Problem(object):
    def __init__(self, env, K, hidden, pol=(32, 32), mseed=7):
        self.env, self.K, self.hidden = env, K, tuple(hidden)
        self.eng, self.dm, theta, self.pdims, self.pool = Hh.make_engine(env, K, hidden, pol, seed=mseed, n_pool=N_POOL)
        if env == 'ant':                                           # some envs start near the lower z bound: state-dependent dones inside the call
            self.pool[::3, 2] = 0.21; self.dm.diff_mean[2] = -0.02
            dm = self.dm
            self.eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
        self.th = theta.astype(np.float32).astype(np.float64)
        self.pool32 = self.pool.astype(np.float32).astype(np.float64)
        assert len({r.tobytes() for r in self.pool32}) == N_POOL    # distinct rows: a pool row identifies its index
        self.tol = TOL.STEP if max(hidden) < 128 else TOL.WIDE
        self.pool_t = torch.tensor(self.pool, dtype=torch.float32, device=self.eng.device)


def _production(p, B, T, H, mode, kernel, seed, label, stream_offset=0, determ=False, force_generic=False, chunks=None):
    dev = _device_run(p, B, T, H, mode, kernel, seed, stream_offset, determ, force_generic, chunks=chunks)
    dr, rad = R.rollout_draws(seed, stream_offset, 0, B, T, p.K, N_POOL, p.dm.ns, p.dm.na)
    _check(p, dev, dr, rad, B, T, H, mode, determ, label)
    return dev


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the generic kernel (the specification's other half): smallest shapes that reach every branch -- a ragged block, resets inside the call
GB, GT, GH = 77, 7, 3
ENVS = ['swimmer', 'hopper', 'snake', 'half_cheetah', 'ant', 'humanoid']       # na 2, 3, 4, 6, 8, 21 (1 .. 11 policy-noise chunks); ns 10 .. 55 (3 .. 14)


@pytest.mark.parametrize('i,sam_mode', list(enumerate(O.SAM_MODES)))
def test_generic_every_sam_mode(i, sam_mode):
    p = Problem('swimmer', 3 if i % 2 else 5, (64, 64))
    _production(p, GB, GT, GH, sam_mode, 'generic', seed_of(100 + i), 'generic/swimmer/' + sam_mode, force_generic=True)


@pytest.mark.parametrize('sam_mode', ['step_rand', 'model_mean_std'])
@pytest.mark.parametrize('i,env', list(enumerate(ENVS)))
def test_generic_every_env(i, env, sam_mode):
    p = Problem(env, 5 if i % 2 else 3, (64, 64))
    _production(p, GB, GT, GH, sam_mode, 'generic', seed_of(10 + 2 * i + (sam_mode == 'step_rand')), 'generic/%s/%s' % (env, sam_mode), force_generic=True)


def test_generic_deterministic_policy_ignores_the_noise_chunks():
    p = Problem('hopper', 3, (64, 64))
    _production(p, GB, GT, GH, 'step_rand', 'generic', seed_of(30), 'generic/determ', determ=True, force_generic=True)


def test_generic_env_counter_carries_into_its_high_word():
    p = Problem('half_cheetah', 5, (64, 64))
    _production(p, GB, GT, GH, 'eps_rand', 'generic', seed_of(31), 'generic/offset', stream_offset=2 ** 32 - 40, force_generic=True)


@pytest.mark.parametrize('env,sam_mode', [('hopper', 'eps_rand'), ('ant', 'step_rand')])
def test_generic_chunked_call_equals_the_draws_of_one_long_call(env, sam_mode):
    p = Problem(env, 5, (64, 64))
    _production(p, GB, 10, GH, sam_mode, 'generic', seed_of(32), 'generic/chunked/' + env, force_generic=True, chunks=(5, 5))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# mixed mode (metrpo.h: any draw tensor may be NULL -> Philox): each tensor withheld in turn, the other four supplied
WITHHELD = [('eps', 'step_rand'), ('model_idx', 'step_rand'), ('sel_noise', 'model_mean_std'), ('reset_idx', 'eps_rand'), ('reset_model', 'eps_rand')]


@pytest.mark.parametrize('family', ['generic', 'mfma-cooperative'])
@pytest.mark.parametrize('i,withheld,sam_mode', [(i, w, m) for i, (w, m) in enumerate(WITHHELD)])
def test_mixed_mode_withheld_tensor_is_drawn_and_supplied_ones_are_used(i, withheld, sam_mode, family):
    p = Problem('hopper', 5, (64, 64))
    B, T, H, seed = GB, GT, GH, seed_of(40 + i)
    if family != 'generic':
        assert p.eng.set_rollout_variant(0) == 2
    given = Hh.draws(np.random.RandomState(50 + i), p.K, B, T, p.dm.ns, p.dm.na, N_POOL)
    given = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in given.items() if k != withheld}
    dev = _device_run(p, B, T, H, sam_mode, family, seed, force_generic=family == 'generic', supplied=given)
    dr, rad = R.rollout_draws(seed, 0, 0, B, T, p.K, N_POOL, p.dm.ns, p.dm.na)
    assert not np.array_equal(dr[withheld], Hh.draws(np.random.RandomState(50 + i), p.K, B, T, p.dm.ns, p.dm.na, N_POOL)[withheld])
    dr.update({k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in given.items()})
    _check(p, dev, dr, rad, B, T, H, sam_mode, False, 'mixed/%s/-%s' % (family, withheld), own=(withheld,))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the fast families, at the smallest shape each dispatch rule admits (the shapes of their own test files)
MFMA_VARIANTS = [('mfma-head-per-wave', 1), ('mfma-cooperative', 0), ('mfma-cooperative', 2)]


@pytest.mark.parametrize('env,sam_mode', [('swimmer', 'step_rand'), ('hopper', 'model_mean_std'), ('ant', 'eps_rand'), ('ant', 'step_rand')])
@pytest.mark.parametrize('kernel,variant', MFMA_VARIANTS)
def test_mfma_kernels_at_2x64(kernel, variant, env, sam_mode):
    p = Problem(env, 5, (64, 64))
    assert p.eng.set_rollout_variant(variant) == (1 if variant == 1 else 2)
    _production(p, GB, GT, GH, sam_mode, kernel, seed_of(60 + variant + 3 * ENVS.index(env)), '%s/v%d/%s/%s' % (kernel, variant, env, sam_mode))


@pytest.mark.parametrize('env,sam_mode', [('ant', 'step_rand'), ('hopper', 'model_mean_std')])
def test_cooperative_chunked_call_equals_the_draws_of_one_long_call(env, sam_mode):
    """The cooperative kernel produces its draws one step ahead and counts steps from the chunk's t0."""
    p = Problem(env, 5, (64, 64))
    assert p.eng.set_rollout_variant(0) == 2
    _production(p, GB, 10, GH, sam_mode, 'mfma-cooperative', seed_of(33), 'coop/chunked/' + env, chunks=(5, 5))


def test_cooperative_six_heads():
    p = Problem('hopper', 6, (64, 64))
    _production(p, GB, GT, GH, 'model_mean_std', 'mfma-cooperative', seed_of(80), 'coop/K6')


def test_cooperative_tiles_handed_over():
    """More env tiles than CUs on the one-workgroup-per-CU form (K > 5): tiles migrate, and every env keeps its own counter."""
    p = Problem('swimmer', 7, (64, 64))
    n_cu = torch.cuda.get_device_properties(p.eng.device).multi_processor_count
    _production(p, 16 * (n_cu + 9), 4, 3, 'step_rand', 'mfma-cooperative', seed_of(81), 'coop/handover')
    assert p.eng.rollout_note() == ''


@pytest.mark.parametrize('sam_mode', ['step_rand', 'model_mean_std'])
def test_tile_gemm_at_hidden_96(sam_mode):
    p = Problem('half_cheetah', 4, (96, 96))
    assert p.eng.set_rollout_variant(0) == 3
    _production(p, 70, 7, 3, sam_mode, 'gemm-stepwise', seed_of(82), 'tile-gemm-96/' + sam_mode)


@pytest.mark.parametrize('sam_mode', ['step_rand', 'model_mean_std'])
@pytest.mark.parametrize('kernel', ['gemm-streamk', 'streamk-persistent'])
def test_stream_k_stepwise_and_persistent(kernel, sam_mode):
    p = Problem('half_cheetah', 4, (256, 256))
    p.eng.set_option('STREAMK', '1'); p.eng.set_rollout_variant(1)
    if kernel == 'gemm-streamk':
        p.eng.set_option('NO_PERSIST', '1')
    _production(p, 270, 7, 3, sam_mode, kernel, seed_of(83), '%s/%s' % (kernel, sam_mode))


@pytest.mark.parametrize('sam_mode', ['step_rand', 'eps_rand'])
def test_policy_gemm_prestep(sam_mode):
    p = Problem('humanoid', 3, (128, 128), HUMANOID_POL)
    assert p.eng.set_rollout_variant(0) == 3
    p.eng.set_option('METRPO_PRE_GEMM', '1')
    _production(p, 90, 6, 4, sam_mode, 'gemm-stepwise', seed_of(84), 'pre-gemm/' + sam_mode)


@pytest.mark.parametrize('hid,B,sam_mode', [(512, 100, 'step_rand'), (512, 5, 'eps_rand'), (1024, 100, 'eps_rand'), (1024, 5, 'step_rand')])
def test_resident(hid, B, sam_mode):
    p = Problem('swimmer', 5 if hid == 512 else 3, (hid, hid))
    _production(p, B, 7, 7 if B == 5 else 3, sam_mode, 'resident', seed_of(85), 'resident/%d/B%d/%s' % (hid, B, sam_mode))


@pytest.mark.parametrize('merged', [True, False])
@pytest.mark.parametrize('env,K,hidden,H,R,sam_mode', [('swimmer', 5, (512, 512), 6, 3, 'step_rand'), ('hopper', 2, (128, 128, 128), 5, 2, 'model_mean_std'),
                                                    ('half_cheetah', 3, (256, 192), 4, 3, 'eps_rand')])
def test_gemm_rounds_side_by_side(env, K, hidden, H, R, sam_mode, merged):
    """T = R H from a reset, horizon-only env: the rounds start from k_round_init_all (merged) / k_round_init (one stream per round)."""
    p = Problem(env, K, hidden)
    assert p.eng.set_rollout_variant(1) == 3
    if not merged:
        p.eng.set_option('METRPO_NO_MERGED_ROUNDS', '1')
    _production(p, 100, R * H, H, sam_mode, 'gemm-stepwise', seed_of(86), 'rounds/%s/%s/%s' % ('merged' if merged else 'streams', env, sam_mode))


@pytest.mark.parametrize('sam_mode', ['step_rand', 'eps_rand'])
def test_resident_rounds_side_by_side(sam_mode):
    p = Problem('swimmer', 5, (512, 512))
    p.eng.set_option('METRPO_RESIDENT_WS', '32')
    _production(p, 100, 9, 3, sam_mode, 'resident', seed_of(87), 'rounds/resident/' + sam_mode)
