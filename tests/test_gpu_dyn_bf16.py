"""The opt-in bf16-operand dynamics forward of metrpo_rollout (include/metrpo.h metrpo_set_dyn_precision, csrc/rollout_bf16.hip; family 7,
'gemm-bf16') against its NumPy restatement tests/dyn_bf16_ref.py.  Reference model: training.py:218-269 (the forward, with the residual of :257),
env_helpers.py:597-635 (the step around it); the operand rounding itself is this library's extension.

  * exact arithmetic: sparse small-integer nets on a dyadic grid (dyn_bf16_ref.exact_rollout, self-checked on the CPU in tests/test_dyn_bf16_ref.py):
    any summation order gives the same f32 bits, so d_obs and d_last_obs must equal the restatement's BITS over T = 3 free-running steps.  Every case
    asserts the column tile of each layer from the host's note (Engine.last_bf16_layers) against the pick rule; four cases are sized from the CU count so
    that their hidden layers run the 128-column tile with column and row edges inside it (the kernels on their own: tests/test_gpu_bf16_gemm.py).
  * rounding mode: inputs on and next to bf16 ties routed straight to the output; truncation and round-half-up each give other bits.
  * random Xavier nets: per-head rel-L2 of s' - s against the rounded float64 restatement.  The bound is MEASURED: 8 x the distance between a float32-
    accumulating NumPy emulation in another summation order and the restatement, on the same case (dyn_bf16_ref.random_bound).  Figures of the emulation
    (worst head, B = 4097, K = 3 half-cheetah nets): hidden (128, 128) 1.79e-5 -> bound 1.43e-4; hidden (512, 512) 8.28e-6 -> bound 6.62e-5.  The
    restatement with truncation lies 8.0e-3 / 3.9e-3 away, the unrounded float64 model 1.8e-3 / 9.3e-4: 12.8 / 14.1 bounds at the least
    (tests/test_dyn_bf16_ref.py asserts >= 10).  The case has 4097 rows, not 129: dyn_bf16_ref.random_case says why (the case was enlarged, not the bound).
  * nothing else moves: everything outside the matrix products, every draw, and every other entry point return the bits they return under F32.
"""
import numpy as np
import pytest
import torch
from oracle import metrpo_oracle as O
import dyn_bf16_ref as R
import bf16_gemm_cases as BG
import helpers as Hh
import tolerances as TOL

pytestmark = pytest.mark.gpu


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine_for(env, dm, theta, acts='relu'):
    import metrpo_amd
    hidden = tuple(W.shape[2] for W in dm.Ws[:-1])
    ph = (100, 50, 25) if env == 'humanoid' else (32, 32)
    eng = metrpo_amd.Engine(env, dm.K, hidden, ph, dyn_act=acts)
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_policy(theta)
    return eng


# B in {1, 17, 64, 129}; hidden (128, 128), (144, 136), (100, 72), (128, 64, 128); swimmer (drop 2), half-cheetah (drop 1, clipped reward), ant (is_done + reset),
# humanoid (ns = 55, the 100-50-25 pre-kernel); K in {1, 5}; step_rand / model_mean / model_med
EXACT = [('swimmer', 1, (128, 128), 1, 'step_rand'), ('swimmer', 5, (144, 136), 17, 'model_med'), ('half_cheetah', 5, (100, 72), 64, 'step_rand'),
         ('half_cheetah', 1, (128, 64, 128), 129, 'model_mean'), ('ant', 5, (128, 128), 129, 'step_rand'), ('ant', 5, (100, 72), 17, 'model_mean'),
         ('ant', 1, (144, 136), 64, 'model_med'), ('humanoid', 5, (144, 136), 64, 'model_med'), ('humanoid', 1, (128, 64, 128), 17, 'step_rand'),
         ('humanoid', 5, (128, 128), 129, 'model_mean'), ('swimmer', 5, (100, 72), 129, 'model_mean'), ('half_cheetah', 5, (128, 128), 1, 'model_med')]
# The 128-column tile (gemm_bf16_pick: N > 64 and K * ceil(B / 128) * ceil(N / 128) >= CU count) with column edges inside the tile (136 = 128 + 8: the
# col >= ldc skip; 200 = 128 + 72) and a row edge (B = 128 r + 1).  The B below serve 256 CUs; the test enlarges them where the device has more.  Each has
# a twin at B = 129, which stays on the 64-column tile throughout.
WIDE_B = 1024
EXACT_WIDE = [('half_cheetah', 5, (136, 200), 3329, 'step_rand'), ('swimmer', 5, (200, 136), 3457, 'model_mean'), ('humanoid', 3, (256, 136), 5633, 'model_med'),
              ('ant', 5, (136, 200), 3329, 'step_rand')]
EXACT += EXACT_WIDE + [(env, K, hidden, 129, mode) for env, K, hidden, B, mode in EXACT_WIDE]


@pytest.mark.parametrize('env,K,hidden,B,sam_mode', EXACT)
def test_exact_arithmetic_bit_for_bit(env, K, hidden, B, sam_mode):
    T, H = 3, 2                                                    # every env is reset from the pool behind step 1 (supplied rows); ant also ends by itself
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    wide = B > WIDE_B
    if wide:                                                       # enough row tiles for the narrowest hidden layer's grid to reach the CU count, plus one row
        B = max(B, 128 * -(-n_cu // (K * min(-(-N // 128) for N in hidden))) + 1)
    dm, theta, pdims, pool, dr, ref = R.exact_rollout(env, K, hidden, B, T, H, sam_mode, seed=3)
    eng = engine_for(env, dm, theta)
    eng.set_dyn_precision('bf16')
    tr = eng.rollout(B, T, H, sam_mode, pool, determ=True, model_idx=dr['model_idx'], reset_idx=dr['reset_idx'], reset_model=dr['reset_model'])
    assert eng.last_rollout_kernel() == 'gemm-bf16' and eng.rollout_note() == ''
    tiles = eng.last_bf16_layers()                                 # the column tile of every layer, as the host noted it
    assert tiles == [BG.want_form(BG.gemm_case('bf16', 'f32', 0, B, N, K=64, Kp=64, heads=K), n_cu)['bn'] for N in hidden + (dm.ns, )]
    assert tiles == ([128] * len(hidden) + [64] if wide else [64] * (len(hidden) + 1))
    assert np.array_equal(bits(tr.obs), bits(ref['obs']))
    assert np.array_equal(bits(tr.last_obs), bits(ref['last_obs']))
    assert np.array_equal(bits(tr.act), bits(ref['act'])) and np.array_equal(bits(tr.mean), bits(ref['act']))
    assert np.array_equal(tr.done.cpu().numpy().astype(bool), ref['done']) and np.array_equal(tr.tpath.cpu().numpy(), ref['tpath'])
    np.testing.assert_allclose(tr.rew.cpu().numpy().astype(np.float64), ref['rew'], **TOL.REWARD)
    if env == 'ant':
        assert ref['done'][0].any() or ref['done'][2].any() or B == 1      # an env-made termination off the horizon's steps


def test_rounding_mode_bit_for_bit():
    """Identity hidden layers with one weight of 1 per column route input j to hidden unit j to output dim j: out[j] = bf16(x[j]).  The swimmer's inputs
    x[0 .. 7] = s[2 .. 9] sit on bf16 ties of both parities, one f32 step above and below them, in both signs and at three binades."""
    env, B = 'swimmer', 64
    ns, na, n_drop = O.ENV_SPECS[env]
    nin, hid = ns + na - n_drop, 128
    W0 = np.zeros((1, nin, hid)); W1 = np.zeros((1, hid, hid)); W2 = np.zeros((1, hid, ns))
    for j in range(nin):
        W0[0, j, j] = 1.0; W1[0, j, j] = 1.0
    for j in range(ns):
        W2[0, j, j] = 1.0
    dm = O.DynamicsEnsemble([W0, W1, W2], [np.zeros((1, hid)), np.zeros((1, hid)), np.zeros((1, ns))], ['identity', 'identity'], np.zeros(ns + na),
                            np.ones(ns + na), np.zeros(ns), np.full(ns, 0.5), n_drop, ns, na)
    even, odd = np.float32(1 + 2.0 ** -8), np.float32(1 + 2.0 ** -7 + 2.0 ** -8)
    near = [np.nextafter(even, np.float32(2)), np.nextafter(even, np.float32(0)), np.nextafter(odd, np.float32(2)), np.nextafter(odd, np.float32(0))]
    vals = np.array([sg * sc * v for v in [even, odd] + near for sg in (1.0, -1.0) for sc in (1.0, 0.25, 4.0)], np.float32)
    rng = np.random.RandomState(2)
    pool = rng.choice(vals, size=(B, ns)).astype(np.float64)
    pdims = O.policy_dims(ns, (32, 32), na)
    theta = np.zeros(O.policy_num_params(pdims)); theta[-2 * na:-na] = [0.5, -0.25]
    idx = dict(model_idx=np.zeros((1, B), np.int64), reset_idx=np.tile(np.arange(B), (2, 1)), reset_model=np.zeros((2, B), np.int64))
    refs = {m: R.rollout_ref(dm, theta, pdims, env, pool, B, 1, 5, 'step_rand', mode=m, **idx)['last_obs'] for m in ('rne', 'trunc', 'half_up')}
    eng = engine_for(env, dm, theta, acts='identity')
    eng.set_dyn_precision('bf16')
    tr = eng.rollout(B, 1, 5, 'step_rand', pool, determ=True, **idx)
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    assert np.array_equal(bits(tr.obs[0]), bits(pool))
    assert np.array_equal(bits(tr.last_obs), bits(refs['rne']))
    for m in ('trunc', 'half_up'):                                 # each of the other two modes fails this case, in a good share of its elements
        assert np.mean(bits(refs[m]) != bits(refs['rne'])) > 0.1


def test_rounding_of_weights_and_hidden_activations_bit_for_bit():
    """The other two rounding sites, pinned on ties as the input conversion is above: the weight image (k_bf16_wimage) and the hidden activations in the
    layer epilogue.  Swimmer, states and clipped actions +-1 (exact), identity hidden layers of 128 units:
      units 0 .. 9:    h1 = x_j + delta_j with an f32 bias delta_j that lands the ACTIVATION on a bf16 tie of either parity, one f32 step beside it, in
                       both signs (where the signs of x_j and delta_j agree; elsewhere the sum is representable and says nothing); weight 1 behind it
      units 10 .. 19:  h1 = x_j, then h2 = x_j * bf16(w_j) with a tie-valued WEIGHT w_j (both parities, beside a tie, both signs, two binades)
    Output dim d reads unit d for d < 5 and unit 10 + d for d >= 5; diff_std = 1/2.  Truncation and round-half-up each give other bits in either group."""
    env, B = 'swimmer', 64
    ns, na, n_drop = O.ENV_SPECS[env]
    nin, hid = ns + na - n_drop, 128
    e, o, u = 2.0 ** -8, 2.0 ** -7 + 2.0 ** -8, 2.0 ** -23
    delta = np.array([e, o, -e, -o, e + u, o - u, -(e - u), -(o + u), e, -o], np.float32)
    even, odd = np.float32(1 + e), np.float32(1 + o)
    w = np.array([even, odd, -even, -odd, np.nextafter(even, np.float32(2)), np.nextafter(odd, np.float32(0)), np.float32(0.25) * even, np.float32(-4) * odd,
                  np.nextafter(even, np.float32(0)), np.nextafter(odd, np.float32(2))], np.float32)
    W0 = np.zeros((1, nin, hid)); b0 = np.zeros((1, hid)); W1 = np.zeros((1, hid, hid)); W2 = np.zeros((1, hid, ns))
    for j in range(nin):
        W0[0, j, j] = 1.0; b0[0, j] = delta[j]; W1[0, j, j] = 1.0
        W0[0, j, 10 + j] = 1.0; W1[0, 10 + j, 10 + j] = w[j]
    for d in range(ns):
        W2[0, d if d < 5 else 10 + d, d] = 1.0
    dm = O.DynamicsEnsemble([W0, W1, W2], [b0, np.zeros((1, hid)), np.zeros((1, ns))], ['identity', 'identity'], np.zeros(ns + na), np.ones(ns + na),
                            np.zeros(ns), np.full(ns, 0.5), n_drop, ns, na)
    pool = np.random.RandomState(4).choice([-1.0, 1.0], size=(B, ns))
    pdims = O.policy_dims(ns, (32, 32), na)
    theta = np.zeros(O.policy_num_params(pdims)); theta[-2 * na:-na] = [1.5, -1.0]          # clipped to +1, -1
    idx = dict(model_idx=np.zeros((1, B), np.int64), reset_idx=np.tile(np.arange(B), (2, 1)), reset_model=np.zeros((2, B), np.int64))
    refs = {m: R.rollout_ref(dm, theta, pdims, env, pool, B, 1, 5, 'step_rand', mode=m, **idx)['last_obs'] for m in ('rne', 'trunc', 'half_up')}
    eng = engine_for(env, dm, theta, acts='identity')
    eng.set_dyn_precision('bf16')
    tr = eng.rollout(B, 1, 5, 'step_rand', pool, determ=True, **idx)
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    assert np.array_equal(bits(tr.last_obs), bits(refs['rne']))
    for m in ('trunc', 'half_up'):
        diff = bits(refs[m]) != bits(refs['rne'])
        assert diff[:, :5].mean() > 0.1 and diff[:, 5:].mean() > 0.1, (m, diff[:, :5].mean(), diff[:, 5:].mean())


def test_sampler_stops_at_the_stop_step_and_issues_no_chunk_behind_it():
    """obtain_samples on an early-terminating env (Ant) with rollout_precision = bf16: the layer GEMMs do not look at the stop flag, so the sampler polls
    it between chunks as it does for the f32 step-wise GEMM family (vectorized_sampler.py:60,104: the loop condition after every step).  The stop step
    is the first at which the completed paths' samples reach batch_size -- recomputed here from one whole bf16 rollout with the sampler's own seed --
    the returned trajectory is that rollout's prefix bit for bit, and the last chunk issued is the one that holds the stop step."""
    import metrpo_amd
    env, K, B, H, batch, chunk = 'ant', 3, 32, 10, 200, 3
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, (128, 128), (32, 32), seed=41)
    pool[::3, 2] = 0.21; dm.diff_mean[2] = -0.02                  # some envs end by themselves
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_dyn_precision('bf16')
    policy = metrpo_amd.GaussianMLPPolicy(eng, init_std=1.0, seed=0)
    eng.set_policy(theta)
    nne = metrpo_amd.NeuralNetEnv(env=metrpo_amd.InitStatePool(pool, dm.na), inner_env=None, cost_np=env, dynamics_in=None, dynamics_outs=eng, sam_mode='step_rand')
    algo = metrpo_amd.TRPO(env=nne, policy=policy, baseline=metrpo_amd.LinearFeatureBaseline(), batch_size=batch, max_path_length=H, step_size=0.01,
                           sampler_args=dict(n_envs=B))
    algo.sampler_chunk = chunk
    calls, orig = [], eng.rollout

    def spy(B_, T_, H_, sam_mode, pool_, **kw):
        calls.append((kw.get('t0', 0), T_, kw.get('seed'), pool_))
        return orig(B_, T_, H_, sam_mode, pool_, **kw)
    eng.rollout = spy
    algo.start_worker()
    paths = algo.obtain_samples(0)
    eng.rollout = orig
    assert eng.last_rollout_kernel() == 'gemm-bf16' and eng.rollout_path() == 7
    T_first, T_max = -(-batch // B), -(-batch // B) + H
    whole = orig(B, T_max, H, 'step_rand', calls[0][3], seed=calls[0][2])
    done, tpath = whole.done.cpu().numpy().astype(np.int64), whole.tpath.cpu().numpy().astype(np.int64)
    cum = np.cumsum((done * (tpath + 1)).sum(axis=1))
    t_stop = int(np.argmax(cum >= batch))
    assert cum[t_stop] >= batch and T_first <= t_stop + 1 <= T_max - chunk            # the stop step leaves whole chunks behind it unissued
    assert done[:t_stop + 1].sum() > B * ((t_stop + 1) // H)                         # envs ended by themselves, not only at the horizon
    assert paths.traj.T == t_stop + 1
    assert torch.equal(paths.traj.obs, whole.obs[:t_stop + 1]) and torch.equal(paths.traj.rew, whole.rew[:t_stop + 1])
    issued = calls[-1][0] + calls[-1][1]
    assert [c[0] for c in calls] == [0] + list(range(T_first, issued, chunk))
    assert t_stop + 1 <= issued < t_stop + 1 + chunk, (t_stop, issued, calls)          # nothing behind the chunk that holds the stop step


_RANDOM = {}


def _random(hidden):
    if hidden not in _RANDOM:
        _RANDOM[hidden] = R.random_bound(hidden)
    return _RANDOM[hidden]


@pytest.mark.parametrize('hidden', R.RANDOM_HIDDEN)
def test_random_nets_within_the_measured_bound(hidden):
    bound, fig, (dm, s, ac), ref = _random(hidden)
    env, B, K = 'half_cheetah', s.shape[0], dm.K
    pdims = O.policy_dims(dm.ns, (32, 32), dm.na)
    theta = np.zeros(O.policy_num_params(pdims))                  # mean 0, log_std 0: the action is the supplied draw itself
    eng = engine_for(env, dm, theta)
    eng.set_dyn_precision('bf16')
    rows = np.tile(np.arange(B), (2, 1))
    worst = 0.0
    for k in range(K):
        tr = eng.rollout(B, 1, 10, 'step_rand', s, eps=ac[None], model_idx=np.full((1, B), k), reset_idx=rows, reset_model=np.zeros((2, B), np.int64))
        assert eng.last_rollout_kernel() == 'gemm-bf16'
        assert np.array_equal(bits(tr.obs[0]), bits(s)) and np.array_equal(bits(tr.act[0]), bits(ac))
        got = tr.last_obs.cpu().numpy().astype(np.float64) - s.astype(np.float64)
        rel = np.linalg.norm(got - ref[k]) / np.linalg.norm(ref[k])
        print('hidden %s head %d: rel-L2 %.3e (emulation %.3e, bound %.3e)' % (hidden, k, rel, fig, bound))
        worst = max(worst, rel)
    assert worst <= bound, (worst, bound)


def _pair(env='half_cheetah', K=3, hidden=(128, 128), seed=31, ph=(32, 32)):
    eng, dm, theta, pdims, pool = Hh.make_engine(env, K, hidden, ph, seed=seed)
    eng.set_rollout_variant(1)                                     # the step-wise families also where the resident kernel applies
    return eng, dm, theta, pdims, pool


def _all(tr):
    return [x.clone() for x in (tr.obs, tr.act, tr.mean, tr.rew, tr.done, tr.tpath, tr.last_obs)]


def test_outside_the_matrix_products_nothing_moves():
    env, K, B, T, H = 'half_cheetah', 3, 70, 6, 3
    eng, dm, theta, pdims, pool = _pair(env, K)
    dr = Hh.draws(np.random.RandomState(4), K, B, T, dm.ns, dm.na, len(pool))
    dr32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in dr.items()}
    f = _all(eng.rollout(B, T, H, 'step_rand', pool, **dr32))
    fam = eng.last_rollout_kernel()
    assert eng.dyn_precision == 'f32' and fam in ('gemm-stepwise', 'gemm-streamk', 'streamk-persistent')
    eng.set_dyn_precision('bf16')
    assert eng.dyn_precision == 'bf16' and eng.rollout_path() == 7
    b = _all(eng.rollout(B, T, H, 'step_rand', pool, **dr32))
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    for x, y in zip(f[:3], b[:3]):                                 # row 0 of obs / act / mean
        assert torch.equal(x[0], y[0])
    assert torch.equal(f[4], b[4]) and torch.equal(f[5], b[5])     # done (the horizon's pattern) and tpath
    assert torch.equal(f[0][H], b[0][H])                           # the reset rows (supplied pool rows)
    assert not torch.equal(f[0][1], b[0][1])                       # ... and the rounded operands do show in the states
    np.testing.assert_allclose(b[0][1].cpu().numpy(), f[0][1].cpu().numpy(), rtol=0, atol=5e-3)
    # a run that draws for itself: same Philox blocks -> the same actions from the same first states
    eng.set_dyn_precision('f32')
    fs = _all(eng.rollout(B, T, H, 'step_rand', pool, seed=9))
    eng.set_dyn_precision('bf16')
    bs_ = _all(eng.rollout(B, T, H, 'step_rand', pool, seed=9))    # (T = 2 H without supplied draws: the rounds side by side as one batch)
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    assert torch.equal(fs[0][0], bs_[0][0]) and torch.equal(fs[1][0], bs_[1][0]) and torch.equal(fs[2][0], bs_[2][0])
    assert torch.equal(fs[0][H], bs_[0][H]) and torch.equal(fs[4], bs_[4]) and torch.equal(fs[5], bs_[5])
    # back to F32: the default rollout bit for bit, on the family it ran on before
    eng.set_dyn_precision('f32')
    again = _all(eng.rollout(B, T, H, 'step_rand', pool, **dr32))
    assert eng.last_rollout_kernel() == fam
    for x, y in zip(f, again):
        assert torch.equal(x, y)


def test_other_entry_points_keep_their_f32_bits():
    env, K, B = 'half_cheetah', 3, 40
    eng, dm, theta, pdims, pool = _pair(env, K)
    rng = np.random.RandomState(8)
    s = pool[:B].astype(np.float32); a = rng.uniform(-1, 1, size=(B, dm.na)).astype(np.float32)
    acts = rng.uniform(-1.2, 1.2, size=(4, B, dm.na)).astype(np.float32)
    x = np.concatenate([s, a], axis=1); y = (rng.randn(B, dm.ns) * 0.1).astype(np.float32)
    import metrpo_amd
    Os = (rng.randn(5, 5, dm.ns) * 0.1).astype(np.float32); Rs = rng.randn(5, 4).astype(np.float32)      # recorded trajectories of the model diagnostic

    def everything():
        out = list(eng.step(s, a, 'model_mean'))
        out.append(eng.validation_cost(s, 5, 0.99))
        out += list(eng.bptt_grad(s, 4, 0.99))
        out.append(eng.eval_losses(x, y))
        out += list(eng.rollout_actions(s, acts, 'model_mean'))
        for model in (-1, 1):                                      # the diagnostic runs metrpo_rollout inside: on the f32 models whatever the setting
            me = metrpo_amd.model_error.model_error(eng, Os, None, Rs, [1, 3], model=model)
            out += [me['state_diff'], me['cost_diff'], me['sums']]
            assert eng.last_rollout_kernel() != 'gemm-bf16'
        torch.cuda.synchronize()
        return [o.clone() for o in out]
    ref = everything()
    eng.set_dyn_precision('bf16')
    eng.rollout(B, 2, 5, 'step_rand', pool, seed=1)                # the bf16 image exists and has been used
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    got = everything()
    assert eng.dyn_precision == 'bf16' and len(ref) == len(got) == 16
    for r_, g_ in zip(ref, got):
        assert torch.equal(r_, g_)
    eng.rollout(B, 2, 5, 'step_rand', pool, seed=1)
    assert eng.last_rollout_kernel() == 'gemm-bf16'                # ... and the setting is still in force behind the diagnostic


def test_chunked_rollout_equals_the_whole_one():
    env, K, B, H = 'half_cheetah', 3, 70, 2
    eng, dm, theta, pdims, pool = _pair(env, K)
    eng.set_dyn_precision('bf16')
    dr = Hh.draws(np.random.RandomState(5), K, B, 3, dm.ns, dm.na, len(pool))
    dr32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in dr.items()}
    whole = _all(eng.rollout(B, 3, H, 'eps_rand', pool, **dr32))
    ts, model = torch.zeros(B, dtype=torch.int32, device='cuda'), torch.zeros(B, dtype=torch.int32, device='cuda')
    c1 = eng.rollout(B, 2, H, 'eps_rand', pool, last_state=(ts, model), **{k: v[:3] if k.startswith('reset') else v[:2] for k, v in dr32.items()})
    c1 = _all(c1)
    c2 = eng.rollout(B, 1, H, 'eps_rand', pool, t0=2, resume=(c1[6], ts, model), last_state=(ts, model),
                     **{k: v[2:4] if k.startswith('reset') else v[2:3] for k, v in dr32.items()})
    assert eng.last_rollout_kernel() == 'gemm-bf16'
    c2 = _all(c2)
    for i in range(6):
        assert torch.equal(whole[i][:2], c1[i]) and torch.equal(whole[i][2:], c2[i])
    assert torch.equal(whole[6], c2[6])


def test_set_dynamics_model_between_two_bf16_rollouts_is_seen():
    env, K, B = 'half_cheetah', 2, 33
    eng, dm, theta, pdims, pool = _pair(env, K)
    eng.set_dyn_precision('bf16')
    kw = dict(determ=True, model_idx=np.ones((1, B), np.int64), reset_idx=np.tile(np.arange(B), (2, 1)), reset_model=np.zeros((2, B), np.int64))
    a = eng.rollout(B, 1, 5, 'step_rand', pool, **kw).last_obs.clone()
    flat0 = np.concatenate([np.concatenate([W[0].ravel(), b[0].ravel()]) for W, b in zip(dm.Ws, dm.bs)])
    eng.set_dynamics_model(1, flat0)                               # head 1 := head 0
    b = eng.rollout(B, 1, 5, 'step_rand', pool, **kw).last_obs.clone()
    kw['model_idx'] = np.zeros((1, B), np.int64)
    c = eng.rollout(B, 1, 5, 'step_rand', pool, **kw).last_obs.clone()
    assert not torch.equal(a, b) and torch.equal(b, c)


def test_api():
    import metrpo_amd
    from metrpo_amd._lib import lib
    eng, dm, theta, pdims, pool = _pair()
    ctx = eng._ctx
    names = eng.option_names()
    assert lib.metrpo_abi_version() == 4
    assert lib.metrpo_get_dyn_precision(ctx) == 0                  # METRPO_DYN_F32
    assert lib.metrpo_set_dyn_precision(ctx, 2) == -1 and lib.metrpo_set_dyn_precision(ctx, -1) == -1      # METRPO_EINVAL
    assert lib.metrpo_get_dyn_precision(ctx) == 0
    assert lib.metrpo_set_dyn_precision(None, 1) == -2 and lib.metrpo_get_dyn_precision(None) == -2          # METRPO_ENULL
    assert lib.metrpo_set_dyn_precision(ctx, 1) == 0 and lib.metrpo_get_dyn_precision(ctx) == 1
    assert lib.metrpo_set_dyn_precision(ctx, 0) == 0 and lib.metrpo_get_dyn_precision(ctx) == 0
    with pytest.raises(ValueError, match='fp16'):
        eng.set_dyn_precision('fp16')
    small = metrpo_amd.Engine('swimmer', 5, (64, 64), (32, 32))
    assert lib.metrpo_set_dyn_precision(small._ctx, 1) == -4       # METRPO_EUNSUPPORTED
    msg = lib.metrpo_last_error(small._ctx).decode()
    assert '64x64' in msg and 'ns = 10' in msg, msg
    assert lib.metrpo_get_dyn_precision(small._ctx) == 0 and small.dyn_precision == 'f32'
    with pytest.raises(metrpo_amd._lib.MetrpoError, match='64x64'):
        small.set_dyn_precision('bf16')
    narrow = metrpo_amd.Engine('swimmer', 2, (8, 8), (32, 32))     # below the GEMM path's widths: the thread-per-env family
    assert lib.metrpo_set_dyn_precision(narrow._ctx, 1) == -4 and '8x8' in lib.metrpo_last_error(narrow._ctx).decode()
    assert eng.option_names() == names and len(names) == 25 and not any('PREC' in n or 'BF16' in n for n in names)


def test_from_params_applies_the_key():
    import json, os
    import metrpo_amd
    from conftest import GOLDEN
    p = json.load(open(os.path.join(GOLDEN, 'params_swimmer.json')))
    assert metrpo_amd.from_params(p).engine.dyn_precision == 'f32'
    p['dynamics_model']['rollout_precision'] = 'bf16'
    s = metrpo_amd.from_params(p)
    assert s.engine.dyn_precision == 'bf16' and s.shapes['dyn_ext'] == dict(rollout_precision='bf16')
    p['dynamics_model']['hidden_layers'] = [64, 64]
    with pytest.raises(metrpo_amd._lib.MetrpoError, match='64x64'):
        metrpo_amd.from_params(p)
