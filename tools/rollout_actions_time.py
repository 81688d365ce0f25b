#!/usr/bin/env python3
"""Time metrpo_rollout_actions (csrc/rollout_actions.hip) and the model diagnostic's known_actions mode that runs on it, at the size of the reference's
commented-out call (model_based_rl.py:619-651): swimmer, C1 nets (K = 5, 2x64 dynamics, 2x32 policy), n = 50 recorded trajectories of T = 100 steps, the
ten horizons (1, 3, 5, 7, 10, 12, 15, 18, 20, 100) -> W = 5000 windows rolled out for hmax = 100 steps.

Timed, as medians of interleaved rounds (CUDA events around `reps` back-to-back calls, after warm-up), [min, max] over the rounds:
  known          metrpo_model_error, known_actions = 1, ensemble mean: window gather + action gather + the fused supplied-action rollout + k_pred_error
  known/parent   the same call in the PARENT's library (--parent-lib), same process, same rounds: hmax x (action gather + metrpo_step's kernel)
  policy         the same call with known_actions = 0 (the policy's actions through metrpo_rollout): the parent's path, unchanged -- the yardstick
  parts of `known`: compare (k_pred_error on a caller-made trajectory), gather (metrpo_model_error_windows), ract-mean (metrpo_rollout_actions alone);
                 the action gather is what is left
  ract-mean / ract-head   the new kernel alone at B = W, T = hmax: model_mean | eps_rand with uniform_model = 0 (one head)
  roll-mean / roll-head   metrpo_rollout at the same B, T: deterministic policy, resumed from the same states, model_mean with all heads | eps_rand, the
                 env's own head only (eval_all_heads = 0)
  loop / loop/parent      the step-loop path against the parent's: the known call at an off-table shape (--loop-hidden, default 128: thread-per-env kernel
                 once per step; the parent adds an action gather per step), n and T as given by --loop-n / --loop-T
--parent-lib: libmetrpo.so of the parent commit, or this commit's objects with the parent's model_error.hip in place of model_error.o (the known_actions
branch is the only code of that call this commit changes; launch_step and its kernel are untouched):
    git show <parent>:me-trpo_amd/csrc/model_error.hip > /tmp/model_error_parent.hip
    cd me-trpo_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -I. -c /tmp/model_error_parent.hip -o /tmp/model_error_parent.o
    hipcc --offload-arch=gfx950 -shared -fPIC $(ls *.o | grep -v '^model_error.o$') /tmp/model_error_parent.o -ldl -lpthread -o ../../tools/_variants/parent_model_error.so
Usage: rollout_actions_time.py [--out FILE] [--parent-lib SO] [--reps N] [--rounds R] [--n 50] [--T 100]"""
import sys, os, argparse, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np, torch
import metrpo_amd
from metrpo_amd import _lib, model_error as M
from oracle import metrpo_oracle as O
import model_error_ref as R


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                   # us


class ParentCtx(object):
    """A context of another build of the library (the parent's), with the ensemble and policy of `eng` copied in on the device."""

    def __init__(self, path, eng, dm, theta):
        self.lib = lib = C.CDLL(path)
        for name in ('metrpo_create', 'metrpo_destroy', 'metrpo_set_dynamics', 'metrpo_set_policy', 'metrpo_model_error', 'metrpo_last_error'):
            fn = getattr(lib, name); fn.restype, fn.argtypes = _lib.SYMBOLS[name]
        d = _lib.Dims()
        d.env, d.ns, d.na, d.n_models = _lib.ENV_IDS[eng.env_name], eng.ns, eng.na, eng.K
        d.dyn_n_hidden, d.n_drop, d.pol_n_hidden = len(eng.dyn_hidden), eng.n_drop, len(eng.pol_hidden)
        for i, h in enumerate(eng.dyn_hidden): d.dyn_hidden[i], d.dyn_act[i] = h, _lib.ACTS['relu']
        for i, h in enumerate(eng.pol_hidden): d.pol_hidden[i] = h
        self.ctx = C.c_void_p()
        assert lib.metrpo_create(C.byref(self.ctx), eng.device.index, C.byref(d)) == 0
        f = lambda x: torch.as_tensor(np.asarray(x, np.float32), device=eng.device).contiguous()
        self.keep = [eng.get_dynamics().contiguous(), f(dm.in_mean), f(dm.in_std), f(dm.diff_mean), f(dm.diff_std), f(theta)]
        p = [C.c_void_p(t.data_ptr()) for t in self.keep]
        assert lib.metrpo_set_dynamics(self.ctx, p[0], p[1], p[2], p[3], p[4], eng._stream()) == 0
        assert lib.metrpo_set_policy(self.ctx, p[5], eng._stream()) == 0
        torch.cuda.synchronize()

    def model_error(self, x, st):
        rc = self.lib.metrpo_model_error(self.ctx, C.byref(x), st)
        assert rc == 0, self.lib.metrpo_last_error(self.ctx)


def setup(env, K, hidden, n, T, parent_lib):
    dm, theta, pdims, pool = O.make_problem(env, K=K, dyn_hidden=hidden, pol_hidden=(32, 32), seed=0, n_pool=max(n, 64))
    dm = dm.astype(np.float32).astype(np.float64); theta = theta.astype(np.float32).astype(np.float64)
    eng = metrpo_amd.Engine(env, K, hidden, (32, 32))
    eng.set_dynamics_layers(dm.Ws, dm.bs, dm.in_mean, dm.in_std, dm.diff_mean, dm.diff_std)
    eng.set_policy(theta)
    Os, As, Rs = R.recorded_trajectories(dm, theta, pdims, env, pool, n, T, seed=0)
    par = ParentCtx(parent_lib, eng, dm, theta) if parent_lib else None
    return eng, par, dm, Os, As, Rs


def me_args(dev, eng, Os, As, Rs, hs):
    n, T = Rs.shape
    W, n_h = n * T, len(hs)
    d = lambda x: torch.as_tensor(x, device=dev).contiguous()
    t = dict(Os=d(Os), As=d(As), Rs=d(Rs), sd=torch.empty(n_h, W, eng.ns, dtype=torch.float32, device=dev), cd=torch.empty(n_h, W, dtype=torch.float32, device=dev),
             va=torch.empty(n_h, W, dtype=torch.uint8, device=dev), sums=torch.empty(n_h, 4, dtype=torch.float64, device=dev), h=(C.c_int32 * n_h)(*hs))

    def args(known=0, traj=None):
        x = _lib.ModelErrorArgs()
        x.d_Os, x.d_As, x.d_Rs, x.n, x.T, x.hs, x.n_h, x.model, x.known_actions = t['Os'].data_ptr(), t['As'].data_ptr(), t['Rs'].data_ptr(), n, T, t['h'], n_h, -1, known
        x.d_state_diff, x.d_cost_diff, x.d_valid, x.d_sums = t['sd'].data_ptr(), t['cd'].data_ptr(), t['va'].data_ptr(), t['sums'].data_ptr()
        if traj is not None:
            x.d_dbg_obs, x.d_dbg_rew, x.d_dbg_done, x.d_dbg_last_obs = traj.obs.data_ptr(), traj.rew.data_ptr(), traj.done.data_ptr(), traj.last_obs.data_ptr()
        return x
    return t, args


def rounds_of(sides, rounds, reps):
    for _, fn, _ in sides: fn(); fn()
    t = {k: [] for k, _, _ in sides}
    for _ in range(rounds):                                    # interleaved rounds: drift of the clock hits all sides alike
        for k, fn, div in sides:
            t[k].append(timed(fn, max(1, reps // div)))
    return {k: np.array(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--loop-hidden', type=int, default=128)
    ap.add_argument('--loop-n', type=int, default=50)
    ap.add_argument('--loop-T', type=int, default=100)
    a = ap.parse_args()
    env, K, n, T = 'swimmer', 5, a.n, a.T
    hs = [h for h in M.TIMESTEPS if h <= T]
    hmax, W = hs[-1], n * T
    eng, par, dm, Os, As, Rs = setup(env, K, (64, 64), n, T, a.parent_lib)
    dev, st = eng.device, eng._stream()
    t, args = me_args(dev, eng, Os, As, Rs, hs)
    call = lambda x: _lib.check(_lib.lib.metrpo_model_error(eng._ctx, C.byref(x), st), eng._ctx)
    init = M.model_error_windows(eng, t['Os'])
    ts0 = torch.zeros(W, dtype=torch.int32, device=dev); md0 = torch.zeros(W, dtype=torch.int32, device=dev)
    traj = eng.alloc_trajectory(W, hmax, hmax + 1)
    roll_mean = lambda: eng.rollout(W, hmax, hmax + 1, 'model_mean', init, determ=True, eval_all_heads=True, out=traj, resume=(init, ts0, md0))
    roll_head = lambda: eng.rollout(W, hmax, hmax + 1, 'eps_rand', init, determ=True, eval_all_heads=False, out=traj, resume=(init, ts0, md0))
    roll_mean(); torch.cuda.synchronize()
    i, tt = np.divmod(np.arange(W), T)
    acts = torch.as_tensor(np.ascontiguousarray(np.stack([As[i, np.minimum(tt + s, T - 1)] for s in range(hmax)], axis=0)), device=dev)     # [hmax, W, na]
    out = (torch.empty(hmax + 1, W, eng.ns, dtype=torch.float32, device=dev), torch.empty(hmax, W, dtype=torch.float32, device=dev),
           torch.empty(hmax, W, dtype=torch.uint8, device=dev))
    ract_mean = lambda: eng.rollout_actions(init, acts, 'model_mean', out=out)
    ract_head = lambda: eng.rollout_actions(init, acts, 'eps_rand', model=0, out=out)
    a_known, a_policy, a_cmp = args(known=1), args(), args(traj=traj)
    sides = [('known', lambda: call(a_known), 1), ('policy', lambda: call(a_policy), 1), ('compare', lambda: call(a_cmp), 1),
             ('gather', lambda: _lib.check(_lib.lib.metrpo_model_error_windows(eng._ctx, C.c_void_p(t['Os'].data_ptr()), n, T, C.c_void_p(init.data_ptr()), st), eng._ctx), 1),
             ('ract-mean', ract_mean, 1), ('ract-head', ract_head, 1), ('roll-mean', roll_mean, 1), ('roll-head', roll_head, 1)]
    if par:
        sides.append(('known/parent', lambda: par.model_error(a_known, st), 5))
    call(a_known); torch.cuda.synchronize()
    path = eng.last_rollout_actions_kernel()
    sums_new = t['sums'].cpu().numpy().copy()
    agree = None
    if par:
        par.model_error(a_known, st); torch.cuda.synchronize()
        sums_par = t['sums'].cpu().numpy()
        agree = float(np.max(np.abs(sums_new[:, 1:] - sums_par[:, 1:]) / np.abs(sums_par[:, 1:]))), bool(np.array_equal(sums_new[:, 0], sums_par[:, 0]))
    roll_head(); fam_head = eng.last_rollout_kernel(); roll_mean(); fam_mean = eng.last_rollout_kernel()
    r = rounds_of(sides, a.rounds, a.reps)
    md = {k: float(np.median(v)) for k, v in r.items()}
    fmt = lambda k: "%9.1f us [%.1f, %.1f]" % (md[k], r[k].min(), r[k].max())
    spread = lambda x, y: max(r[x].max() - r[x].min(), r[y].max() - r[y].min())
    lines = [
        "# metrpo_rollout_actions and metrpo_model_error(known_actions) at the reference's call size: %s, K = %d, 2x64 dynamics, 2x32 policy, n = %d, T = %d, horizons %s" % (env, K, n, T, tuple(hs)),
        "# W = %d windows x hmax = %d steps; supplied-action path: %s.  %d interleaved rounds of %d back-to-back calls (parent: %d), CUDA events, 2 warm-up calls each;" % (
            W, hmax, path, a.rounds, a.reps, max(1, a.reps // 5)),
        "# medians and [min, max] over the rounds.  Device: %s" % torch.cuda.get_device_name(0),
        "known_actions call, this commit                 %s" % fmt('known')]
    if par:
        lines += ["known_actions call, parent (same run)          %s   parent / this commit %.1f x; sums[1:] agree within %.2g relative, counts %s" % (
            fmt('known/parent'), md['known/parent'] / md['known'], agree[0], 'equal' if agree[1] else 'DIFFER')]
    rest = md['known'] - md['compare'] - md['gather'] - md['ract-mean']
    lines += [
        "policy-mode call, same commit (the yardstick)   %s   known / policy %.2f x (bar: 2.5 x); spread of the pair %.1f us" % (fmt('policy'), md['known'] / md['policy'], spread('known', 'policy')),
        "parts of the known_actions call:",
        "  k_pred_error alone (caller-made trajectory)   %s" % fmt('compare'),
        "  window gather alone                           %s" % fmt('gather'),
        "  metrpo_rollout_actions alone (model_mean)     %s" % fmt('ract-mean'),
        "  action gather = known - the three above       %9.1f us" % rest,
        "the new kernel alone against metrpo_rollout, B = %d, T = %d:" % (W, hmax),
        "  model_mean: rollout_actions                   %s" % fmt('ract-mean'),
        "              metrpo_rollout (%s)   %s   ratio %.2f x" % (fam_mean, fmt('roll-mean'), md['ract-mean'] / md['roll-mean']),
        "  one head:   rollout_actions (uniform_model)   %s" % fmt('ract-head'),
        "              metrpo_rollout (%s, eps_rand, own head only)   %s   ratio %.2f x" % (fam_head, fmt('roll-head'), md['ract-head'] / md['roll-head'])]
    # ---- the step loop against the parent's: an off-table shape ----
    del eng, par
    hid = (a.loop_hidden, a.loop_hidden)
    n2, T2 = a.loop_n, a.loop_T
    hs2 = [h for h in M.TIMESTEPS if h <= T2]
    eng2, par2, dm2, Os2, As2, Rs2 = setup(env, K, hid, n2, T2, a.parent_lib)
    t2, args2 = me_args(eng2.device, eng2, Os2, As2, Rs2, hs2)
    k2 = args2(known=1)
    st2 = eng2._stream()
    sides2 = [('loop', lambda: _lib.check(_lib.lib.metrpo_model_error(eng2._ctx, C.byref(k2), st2), eng2._ctx), 5)]
    if par2:
        sides2.append(('loop/parent', lambda: par2.model_error(k2, st2), 5))
    r2 = rounds_of(sides2, a.rounds, a.reps)
    path2 = eng2.last_rollout_actions_kernel()
    f2 = lambda k: "%9.1f us [%.1f, %.1f]" % (float(np.median(r2[k])), r2[k].min(), r2[k].max())
    lines += ["step-loop path (%s): known_actions call at hidden %dx%d, K = %d, n = %d, T = %d (hmax = %d)" % (path2, hid[0], hid[1], K, n2, T2, hs2[-1]),
              "  this commit                                   %s" % f2('loop')]
    if par2:
        lines += ["  parent (same run)                             %s   this commit / parent %.3f" % (f2('loop/parent'), float(np.median(r2['loop'])) / float(np.median(r2['loop/parent'])))]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
