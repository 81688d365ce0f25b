#!/usr/bin/env python3
"""Time metrpo_rollout with the dynamics forward on bf16 operands (Engine.set_dyn_precision('bf16'), csrc/rollout_bf16.hip, family 'gemm-bf16') against the
f32 default dispatch of the SAME library and context, at the per-GPU shares of BASELINE's C2 / C3 / C4 and at the params-file shapes (B = 100, 2 x 512 and
2 x 1024), and measure what the rounded operands do to a trajectory.

Timing: one engine per shape, the precision switched between calls; medians of --rounds interleaved rounds (CUDA events around --reps back-to-back
rollouts of T steps, after two warm-up calls per side), [min, max] over the rounds.  The large shares run T = --steps steps of their horizon (the step
time does not depend on the step index), the params-file shapes their whole batch (rounds x H steps: the rounds run side by side there).  Next to every
bf16 figure: the achieved fraction of the bf16 matrix issue rate, 2 K B sum_l(n_l n_l+1) flop per step over CUs x 4 SIMDs x 1024 flop per cycle
(one 32x32x16 instruction per 32 cycles per SIMD) x the clock (--clock-mhz, default the MI355X's 2400 MHz peak) -- of the WHOLE step, pre-step and closing kernels included.
The feature earns its place where f32 / bf16 exceeds 1 by more than the pair's spread.

--sampler: VectorizedSampler.obtain_samples at the C3 share (Ant ends early: chunks + the stop rule; the step-wise GEMM families, bf16 included, poll the
stop flag between chunks), whole calls timed on the host.

Trajectories: the C2-shaped synthetic nets (half-cheetah, K = 5, 2 x 1024), the same supplied draws under F32 and BF16, H = 200: rel-L2 of the state
at t = 1, 10, 50 and the relative difference of the batch-mean return.  A documented figure for users deciding whether to switch, not an assertion.

Usage: dyn_bf16_time.py [--out FILE] [--rounds 7] [--reps 3] [--steps 50] [--shapes C2,C3,C4,p512,p1024] [--no-traj] [--sampler] [--clock-mhz 2400]"""
import sys, os, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import metrpo_amd
from metrpo_amd import synthetic

# name: (what, env, K, dynamics hidden, policy hidden, B, H, rounds of the params-file batch or 0)
SHAPES = {
    'C2': ('C2 per-GPU share (10000 / 4)', 'half_cheetah', 5, (1024, 1024), (32, 32), 2500, 200, 0),
    'C3': ('C3 per-GPU share (20000 / 8)', 'ant', 10, (512, 512), (32, 32), 2500, 500, 0),
    'C4': ('C4 per-GPU share (50000 / 8)', 'humanoid', 20, (1024, 1024, 1024), (100, 50, 25), 6250, 1000, 0),
    'p512': ('params-swimmer.json (B = 100, 2 x 512)', 'swimmer', 5, (512, 512), (32, 32), 100, 200, 3),
    'p1024': ('params-half-cheetah.json (B = 100, 2 x 1024)', 'half_cheetah', 5, (1024, 1024), (32, 32), 100, 100, 5),
}


def make(env, K, hidden, ph):
    eng = metrpo_amd.Engine(env, K, hidden, ph)
    Ws, bs, norm = synthetic.make_dynamics(env, K, hidden, seed=1)
    eng.set_dynamics_layers(Ws, bs, norm['in_mean'], norm['in_std'], norm['diff_mean'], norm['diff_std'])
    eng.set_policy(metrpo_amd.xavier_policy_theta(eng.ns, ph, eng.na))
    return eng


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


def time_shape(name, a, peak):
    what, env, K, hidden, ph, B, H, R = SHAPES[name]
    T = R * H if R else min(H, a.steps)
    eng = make(env, K, hidden, ph)
    pool = torch.as_tensor(synthetic.make_pool(env), device=eng.device)
    out = eng.alloc_trajectory(B, T, H)
    seed = [0]

    def run(prec):
        def fn():
            eng.set_dyn_precision(prec)
            seed[0] += 1
            eng.rollout(B, T, H, 'step_rand', pool, seed=seed[0], out=out)
        return fn
    fam = {}
    for prec in ('f32', 'bf16'):
        run(prec)(); run(prec)(); torch.cuda.synchronize()
        fam[prec] = eng.last_rollout_kernel()
    t = {'f32': [], 'bf16': []}
    for _ in range(a.rounds):                                  # interleaved rounds: drift of the clock hits both sides alike
        for prec in ('f32', 'bf16'):
            t[prec].append(timed(run(prec), a.reps))
    t = {k: np.array(v) for k, v in t.items()}
    md = {k: float(np.median(v)) for k, v in t.items()}
    spread = max(t['f32'].max() - t['f32'].min(), t['bf16'].max() - t['bf16'].min())
    dims = [eng.ns + eng.na - eng.n_drop] + list(hidden) + [eng.ns]
    flop = 2.0 * K * B * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1)) * T
    gain = md['f32'] - md['bf16']
    verdict = 'bf16 faster by more than the spread' if gain > spread else ('bf16 slower by more than the spread' if -gain > spread else 'within the spread')
    f = lambda k: "%10.1f us [%.1f, %.1f]" % (md[k], t[k].min(), t[k].max())
    return ["%s: %s, K = %d, hidden %s, B = %d, T = %d steps (H = %d)" % (name, what, K, 'x'.join(map(str, hidden)), B, T, H),
            "  f32 default (%s)%s  %s   %.1f us / step   %.1f TF" % (fam['f32'], ' ' * (20 - len(fam['f32'])), f('f32'), md['f32'] / T, flop / md['f32'] * 1e-6),
            "  bf16 (%s)%s         %s   %.1f us / step   %.1f TF = %.3f of the bf16 issue rate" % (fam['bf16'], ' ' * (20 - len(fam['bf16'])), f('bf16'), md['bf16'] / T,
                                                                                                 flop / md['bf16'] * 1e-6, flop / (md['bf16'] * 1e-6) / peak),
            "  f32 / bf16 %.2f x; spread of the pair %.1f us, difference %.1f us: %s" % (md['f32'] / md['bf16'], spread, gain, verdict)]


def trajectories():
    what, env, K, hidden, ph, B, H, _ = SHAPES['C2']
    eng = make(env, K, hidden, ph)
    pool = synthetic.make_pool(env)
    rng = np.random.RandomState(3)
    dr = dict(eps=rng.randn(H, B, eng.na).astype(np.float32), model_idx=rng.randint(K, size=(H, B)), reset_idx=rng.randint(len(pool), size=(H + 1, B)),
              reset_model=rng.randint(K, size=(H + 1, B)))
    res = {}
    for prec in ('f32', 'bf16'):
        eng.set_dyn_precision(prec)
        tr = eng.rollout(B, H, H, 'step_rand', pool, **dr)
        res[prec] = (tr.obs.double().cpu().numpy(), tr.rew.double().cpu().numpy())
    (of, rf), (ob, rb) = res['f32'], res['bf16']
    lines = ["trajectories under the same supplied draws, F32 against BF16: %s nets, K = %d, hidden %s, B = %d, H = %d, step_rand" % (env, K, 'x'.join(map(str, hidden)), B, H)]
    for t in (1, 10, 50):
        lines.append("  state at t = %-3d rel-L2 %.3e   (rel-L2 of the displacement from the start state %.3e)" % (
            t, np.linalg.norm(ob[t] - of[t]) / np.linalg.norm(of[t]), np.linalg.norm(ob[t] - of[t]) / np.linalg.norm(of[t] - of[0])))
    ret_f, ret_b = rf.sum(axis=0).mean(), rb.sum(axis=0).mean()
    lines.append("  batch-mean return over H = %d: f32 %.6f, bf16 %.6f, relative difference %.3e" % (H, ret_f, ret_b, abs(ret_b - ret_f) / abs(ret_f)))
    return lines


def sampler_c3(a):
    """VectorizedSampler.obtain_samples at the C3 share (Ant ends early: chunked rollouts, the stop rule of vectorized_sampler.py:60,104), batch_size = B H:
    host-timed whole calls (the loop reads the stop flag / the stop step on the host), interleaved rounds."""
    import time
    what, env, K, hidden, ph, B, H, _ = SHAPES['C3']
    eng = make(env, K, hidden, ph)
    policy = metrpo_amd.GaussianMLPPolicy(eng, init_std=1.0, seed=0)
    nne = metrpo_amd.NeuralNetEnv(env=metrpo_amd.InitStatePool(synthetic.make_pool(env), eng.na), inner_env=None, cost_np=env, dynamics_in=None, dynamics_outs=eng,
                                  sam_mode='step_rand')
    algo = metrpo_amd.TRPO(env=nne, policy=policy, baseline=metrpo_amd.LinearFeatureBaseline(), batch_size=B * H, max_path_length=H, step_size=0.01,
                           sampler_args=dict(n_envs=B))
    algo.reuse_trajectory_buffers = True
    algo.start_worker()
    t, steps, fam = {'f32': [], 'bf16': []}, {}, {}
    for rnd in range(a.rounds + 1):                            # round 0 warms up
        for prec in ('f32', 'bf16'):
            eng.set_dyn_precision(prec)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            paths = algo.obtain_samples(rnd)
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                t[prec].append(dt)
            steps[prec], fam[prec] = paths.traj.T, eng.last_rollout_kernel()
    t = {k: np.array(v) for k, v in t.items()}
    f = lambda k: "%9.2f ms [%.2f, %.2f], %d steps kept, family %s" % (float(np.median(t[k])), t[k].min(), t[k].max(), steps[k], fam[k])
    spread = max(t['f32'].max() - t['f32'].min(), t['bf16'].max() - t['bf16'].min())
    return ["obtain_samples at the C3 share (Ant, K = %d, hidden %s, %d envs, H = %d, batch_size %d; chunked, stop rule; host-timed, %d interleaved rounds):" % (
                K, 'x'.join(map(str, hidden)), B, H, B * H, a.rounds),
            "  f32 default  %s" % f('f32'), "  bf16         %s" % f('bf16'),
            "  f32 / bf16 %.2f x; spread of the pair %.2f ms" % (float(np.median(t['f32'])) / float(np.median(t['bf16'])), spread)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--shapes', default='C2,C3,C4,p512,p1024')
    ap.add_argument('--no-traj', action='store_true')
    ap.add_argument('--sampler', action='store_true', help='also time VectorizedSampler.obtain_samples at the C3 share (Ant)')
    ap.add_argument('--clock-mhz', type=float, default=2400.0)
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    clock = a.clock_mhz * 1e6                                  # Hz (the MI355X's peak engine clock unless given)
    peak = prop.multi_processor_count * 4 * 1024.0 * clock
    lines = ["# metrpo_rollout, dynamics forward on bf16 operands against the f32 default dispatch of the same library and context.  %d interleaved rounds of %d" % (a.rounds, a.reps),
             "# back-to-back rollouts, CUDA events, 2 warm-up calls per side; medians and [min, max] over the rounds.  Device: %s, %d CUs at %.0f MHz:" % (
                 prop.name, prop.multi_processor_count, clock * 1e-6),
             "# bf16 issue rate %.0f TF (one 32x32x16 matrix instruction per 32 cycles per SIMD).  TF figures: dynamics-layer flop over the whole rollout time." % (peak * 1e-12)]
    for name in a.shapes.split(','):
        lines += time_shape(name, a, peak)
        print("\n".join(lines[-4:]), flush=True)
    if a.sampler:
        lines += sampler_c3(a)
        print("\n".join(lines[-4:]), flush=True)
    if not a.no_traj:
        lines += trajectories()
        print("\n".join(lines[-5:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
