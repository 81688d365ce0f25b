"""Thin tensor-level wrapper of one metrpo_ctx (one GPU).  torch is used for device memory and
streams only; all arithmetic happens in libmetrpo.so.  Every method enqueues on torch's current
stream of the engine's device."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import lib, check

METRPO_UNSET = -100            # include/metrpo.h: metrpo_get_option of a known key without a value

Trajectory = namedtuple('Trajectory', 'obs act rew mean done tpath last_obs B T H')
"""Time-major device tensors of one rollout: obs [T,B,ns], act [T,B,na] (unclipped), rew [T,B],
mean [T,B,na], done [T,B] uint8, tpath [T,B] int32, last_obs [B,ns]."""


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32(t, dev, shape=None):
    if t is None:
        return None
    t = torch.as_tensor(t, device=dev).to(torch.float32).contiguous()
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), "expected shape %s, got %s" % (shape, tuple(t.shape))
    return t


def _i32(t, dev, shape=None):
    if t is None:
        return None
    t = torch.as_tensor(t, device=dev).to(torch.int32).contiguous()
    if shape is not None:
        assert tuple(t.shape) == tuple(shape), "expected shape %s, got %s" % (shape, tuple(t.shape))
    return t


class Engine(object):
    """Owns the metrpo_ctx for one (env, ensemble shape, policy shape) on one GPU."""

    def __init__(self, env, n_models, dyn_hidden, pol_hidden, ns=None, na=None, n_drop=None, dyn_act='relu',
                 device=None, prediction_type='state_change', use_logit_weights=False):
        # the dynamics-model variants the reference defines but none of its six-env params files selects have no kernel here: say so by name
        # instead of silently evaluating the 'state_change' arithmetic (dynamics_model.prediction_type / .use_logit_weights of params-*.json)
        if prediction_type != 'state_change':
            raise ValueError("dynamics_model.prediction_type=%r is not implemented: only 'state_change' (training.py:257: s' = diff_mean + diff_std * out + s); "
                             "'second_derivative' (training.py:259-264) and the '*_goal' variants (training.py:265-268) have no kernel in this library"
                             % (prediction_type,))
        if use_logit_weights:
            raise ValueError("dynamics_model.use_logit_weights=True is not implemented (the sigmoid input gate of training.py:234-242, 212-213); "
                             "every shipped params file of the six envs sets it to false")
        if not torch.cuda.is_available():
            raise RuntimeError("metrpo_amd needs an AMD GPU (gfx950); there is no CPU fallback")
        self.env_name = env.replace('-', '_')
        specs = {'swimmer': (10, 2, 2), 'half_cheetah': (18, 6, 1), 'ant': (29, 8, 2), 'humanoid': (55, 21, 0),
                 'hopper': (11, 3, 0), 'snake': (14, 4, 2)}
        d_ns, d_na, d_drop = specs[self.env_name]
        self.ns, self.na = ns or d_ns, na or d_na
        self.n_drop = d_drop if n_drop is None else n_drop
        self.K = int(n_models)
        self.dyn_hidden, self.pol_hidden = list(dyn_hidden), list(pol_hidden)
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        acts = [dyn_act] * len(self.dyn_hidden) if isinstance(dyn_act, str) else list(dyn_act)
        d = _lib.Dims()
        d.env, d.ns, d.na, d.n_models = _lib.ENV_IDS[self.env_name], self.ns, self.na, self.K
        d.dyn_n_hidden, d.n_drop, d.pol_n_hidden = len(self.dyn_hidden), self.n_drop, len(self.pol_hidden)
        for i, h in enumerate(self.dyn_hidden):
            d.dyn_hidden[i], d.dyn_act[i] = h, _lib.ACTS[acts[i]]
        for i, h in enumerate(self.pol_hidden):
            d.pol_hidden[i] = h
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib.metrpo_create(C.byref(self._ctx), self.device.index, C.byref(d))
        check(rc, self._ctx if self._ctx else None)
        self.dyn_param_count = lib.metrpo_dyn_param_count(self._ctx)
        self.P = lib.metrpo_policy_param_count(self._ctx)
        self.pol_dims = [self.ns] + self.pol_hidden + [self.na]
        self.has_mfma_path = bool(lib.metrpo_has_mfma_path(self._ctx))
        self._cb_keepalive = None
        self.comm_world = 0                  # > 0 once comm_init attached an RCCL communicator

    def __del__(self):
        ctx = getattr(self, '_ctx', None)
        if ctx:
            lib.metrpo_destroy(ctx)
            self._ctx = None

    def set_rollout_variant(self, v):
        """Test hook: 0 = fastest rollout kernel available, 1 = head-per-wave MFMA kernel (for large nets: the step-wise
        GEMM path even where the resident kernel applies), 2 = cooperative kernel in its
        two-workgroups-per-CU instantiation at any batch size.  Returns the variant that
        will run: 3 step-wise GEMM (large nets), 2 cooperative-heads MFMA, 1 head-per-wave MFMA, 0 generic."""
        self._variant = int(v)
        return int(lib.metrpo_set_rollout_variant(self._ctx, int(v)))

    def set_update_path(self, use_mfma):
        """Test hook: False forces the generic (VALU) policy-update kernels, True selects the fastest path of the shape (fused
        MFMA kernels, else the GEMM path for large N), 'gemm' forces the GEMM path (policy_gemm.hip).  Returns True if the fused
        MFMA kernels are active, 'gemm' if the GEMM path is forced, else False."""
        code = 2 if use_mfma == 'gemm' else int(bool(use_mfma))
        r = int(lib.metrpo_set_update_path(self._ctx, code))
        return 'gemm' if r == 2 else bool(r)

    # ------------------------------------------------------------------ multi-GPU: RCCL communicator owned by the ctx
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes (ncclGetUniqueId) that rank 0 ships to the other ranks before every rank calls comm_init."""
        buf = C.create_string_buffer(128)
        check(lib.metrpo_comm_get_unique_id(buf), None)
        return buf.raw

    def comm_init(self, unique_id, world, rank):
        """Collective: attach an RCCL communicator; metrpo_trpo_update then issues its all-reduces itself (no host callback)."""
        assert len(unique_id) == 128
        with torch.cuda.device(self.device):
            self._chk(lib.metrpo_comm_init(self._ctx, C.c_char_p(unique_id), int(world), int(rank)))
        self.comm_world = int(world)

    def comm_destroy(self):
        self._chk(lib.metrpo_comm_destroy(self._ctx))
        self.comm_world = 0

    # ---- one-shot direct all-reduce over peer-mapped receive regions (comm.hip / xchg_device.h)
    IPC_BLOB_BYTES = 128

    def comm_ipc_export(self):
        """Allocate + zero this rank's receive region; -> 128 opaque bytes (IPC handle) to all-gather over the ranks."""
        buf = C.create_string_buffer(self.IPC_BLOB_BYTES)
        with torch.cuda.device(self.device):
            self._chk(lib.metrpo_comm_ipc_export(self._ctx, buf))
        return buf.raw

    def comm_ipc_attach(self, blobs, world, rank):
        """blobs: the ranks' export blobs concatenated in rank order.  Maps the peers' regions; from then on the sum all-reduces of the
        path are one-shot exchanges issued by libmetrpo.so (inside metrpo_trpo_update: in the tail of the reduction kernels)."""
        assert len(blobs) == self.IPC_BLOB_BYTES * int(world)
        with torch.cuda.device(self.device):
            self._chk(lib.metrpo_comm_ipc_attach(self._ctx, C.c_char_p(blobs), int(world), int(rank)))
        self.comm_world = int(world)

    def comm_ipc_detach(self):
        self._chk(lib.metrpo_comm_ipc_detach(self._ctx))
        if not lib.metrpo_comm_transport(self._ctx):
            self.comm_world = 0

    def comm_set_timeout_ms(self, ms):
        self._chk(lib.metrpo_comm_set_timeout_ms(self._ctx, int(ms)))

    def comm_transport(self):
        return {0: None, 1: 'rccl', 2: 'one-shot'}[int(lib.metrpo_comm_transport(self._ctx))]

    def comm_check(self):
        """Synchronise and raise if an exchange timed out (a rank that never arrived)."""
        self._chk(lib.metrpo_comm_check(self._ctx, self._stream()))

    def allreduce_sum_(self, t):
        """In-place sum of a float64 device tensor over the ranks of the attached communicator (stream-ordered)."""
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
        self._chk(lib.metrpo_allreduce_sum_f64(self._ctx, _ptr(t), t.numel(), self._stream()))
        return t

    def set_exclusive(self, exclusive):
        """False: other compute processes share this GPU (several ranks per device) -- the kernels whose workgroups wait on each other inside one
        launch (resident rollout / validation, migrating tiles) are never selected.  Default True."""
        self._chk(lib.metrpo_set_exclusive(self._ctx, int(bool(exclusive))))

    def set_dyn_precision(self, precision):
        """Operand precision of the dynamics forward inside rollout() (`metrpo_set_dyn_precision`): 'f32' (default, exact) or 'bf16' -- layer inputs and
        weights rounded to bf16 (nearest even), f32 accumulation, everything outside the matrix products unchanged (include/metrpo.h has the full
        semantics).  rollout() only: step, validation_cost, bptt_grad, training, eval_losses, model_error and rollout_actions stay f32.  Shapes outside
        the step-wise GEMM rollout families raise MetrpoError (the precision then stays 'f32').  Takes effect at the next rollout()."""
        if precision not in _lib.DYN_PRECISIONS:
            raise ValueError("dyn precision %r: one of %s" % (precision, sorted(_lib.DYN_PRECISIONS)))
        self._chk(lib.metrpo_set_dyn_precision(self._ctx, _lib.DYN_PRECISIONS[precision]))

    @property
    def dyn_precision(self):
        return {v: k for k, v in _lib.DYN_PRECISIONS.items()}[int(lib.metrpo_get_dyn_precision(self._ctx))]

    def set_option(self, key, value=None):
        """Variant / tuning switch of THIS engine (`metrpo_set_option`): `key` is one of `Engine.option_names()` (the former METRPO_<KEY> environment
        variables; the environment only fills the defaults when the engine is created), `value` a string / number, None unsets.  Read at the next launch."""
        self._chk(lib.metrpo_set_option(self._ctx, str(key).encode(), None if value is None else str(value).encode()))

    def get_option(self, key):
        """Current value of a switch as a string, None when unset."""
        buf = C.create_string_buffer(256)
        n = lib.metrpo_get_option(self._ctx, str(key).encode(), buf, 256)
        if n == METRPO_UNSET:                     # a known key without a value; an unknown key is METRPO_EINVAL and raises
            return None
        if n < 0:
            self._chk(n)
        return buf.value.decode()

    @staticmethod
    def option_names():
        out, i = [], 0
        while True:
            nm = lib.metrpo_option_name(i)
            if nm is None:
                return out
            out.append(nm.decode()); i += 1

    def schedulable_cus(self):
        """CUs that actually run this process's waves (a census kernel; CU masks and partitions count), measured once per engine."""
        return int(lib.metrpo_schedulable_cus(self._ctx, self._stream()))

    def probe_peaks(self):
        """Measured (f32 MFMA TFLOP/s, HBM copy GB/s) of this device: register-resident MFMA issue loop, 1 GiB streaming copy."""
        out = (C.c_double * 2)()
        self._chk(lib.metrpo_probe_peaks(self._ctx, out, self._stream()))
        return float(out[0]), float(out[1])

    def fvp_kernel_us(self):
        """Diagnostics: mean duration (us) and count of the Fisher-vector-product KERNEL launches recorded since the last call while option
        TIME_FVP was set (HIP events around the kernel itself inside the update's launch sequence)."""
        us, n = C.c_double(0.0), C.c_int32(0)
        self._chk(lib.metrpo_debug_fvp_us(self._ctx, C.byref(us), C.byref(n)))
        return float(us.value), int(n.value)

    def last_update_launch(self):
        """Diagnostics: what the last policy-update launch ran on, as the host noted it when it enqueued it: dict(family 'generic' | 'mfma' | 'gemm' |
        'fused3' (None before the first launch), op (the UpdOp as launched: 0 gradient, 1 FVP, 2 loss + KL, 3 cached FVP, 4 VPG, 5 PPO, 6 PPO with the KL penalty), table (index of the
        fused 2 x 32 kernel set, -1 elsewhere), pt (sample tile of the generic kernels), nrows (partial rows of the reduction), splits / kchunk (GEMM path))."""
        out = (C.c_int32 * 7)()
        self._chk(lib.metrpo_debug_last_update(self._ctx, out))
        d = dict(zip(('family', 'op', 'table', 'pt', 'nrows', 'splits', 'kchunk'), (int(x) for x in out)))
        d['family'] = {-1: None, 0: 'generic', 1: 'mfma', 2: 'gemm', 3: 'fused3'}[d['family']]
        return d

    def last_solve_launch(self):
        """Diagnostics: the Fisher-vector products of the last CG solve a trpo_update enqueued, as the host noted them: dict(family (as last_update_launch), op (1 FVP,
        3 cached FVP of the fused 2 x 32 kernels; -1: the solve made no product, -2: its products disagree), table, n_fvp (the explicit step-scale product included),
        cache_activations, publish_image, fused_tails (False: stand-alone CG kernels), fvp_batch (a separate FVP batch was in force))."""
        out = (C.c_int32 * 8)()
        self._chk(lib.metrpo_debug_last_solve(self._ctx, out))
        d = dict(zip(('family', 'op', 'table', 'n_fvp'), (int(x) for x in out[:4])))
        d['family'] = {-1: None, 0: 'generic', 1: 'mfma', 2: 'gemm', 3: 'fused3'}[d['family']]
        d.update(zip(('cache_activations', 'publish_image', 'fused_tails', 'fvp_batch'), (bool(x) for x in out[4:8])))
        return d

    def retired_workspaces(self, sweep=False):
        """Diagnostics: (count, bytes) of outgrown workspaces the context keeps until destroy (a launch entry point never frees: hipFree waits for every stream);
        sweep=True frees them now (synchronising)."""
        b = C.c_ulonglong(0)
        n = int(lib.metrpo_debug_ws_retired(self._ctx, C.byref(b), int(bool(sweep))))
        return n, int(b.value)

    def update_path(self, N):
        """Kernel family the policy update of an N-sample batch runs on: 'mfma' (fused), 'gemm' or 'generic'."""
        return {1: 'mfma', 2: 'gemm', 0: 'generic'}[int(lib.metrpo_update_path(self._ctx, int(N)))]

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, rc):
        check(rc, self._ctx)

    # ------------------------------------------------------------------ weights
    def set_dynamics(self, params, in_mean, in_std, diff_mean, diff_std):
        """params [K, dyn_param_count] (per model: W0,b0,...,Wout,bout, W row-major (n_in,n_out))."""
        dev = self.device
        p = _f32(params, dev, (self.K, self.dyn_param_count))
        a = _f32(in_mean, dev, (self.ns + self.na,)); b = _f32(in_std, dev, (self.ns + self.na,))
        c = _f32(diff_mean, dev, (self.ns,)); e = _f32(diff_std, dev, (self.ns,))
        self._chk(lib.metrpo_set_dynamics(self._ctx, _ptr(p), _ptr(a), _ptr(b), _ptr(c), _ptr(e), self._stream()))
        torch.cuda.current_stream(dev).synchronize()     # inputs may be temporaries

    def set_dynamics_layers(self, Ws, bs, in_mean, in_std, diff_mean, diff_std):
        """Ws[l]: [K, n_in, n_out], bs[l]: [K, n_out] -> packs the flat per-model layout."""
        parts = []
        for W, b in zip(Ws, bs):
            W = torch.as_tensor(W); b = torch.as_tensor(b)
            parts += [W.reshape(self.K, -1), b.reshape(self.K, -1)]
        self.set_dynamics(torch.cat([p.to(torch.float32) for p in parts], dim=1), in_mean, in_std, diff_mean, diff_std)

    def set_policy(self, theta):
        self._close_open_update()
        t = _f32(theta, self.device, (self.P,))
        self._chk(lib.metrpo_set_policy(self._ctx, _ptr(t), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def get_policy(self):
        self._close_open_update()
        out = torch.empty(self.P, dtype=torch.float32, device=self.device)
        self._chk(lib.metrpo_get_policy(self._ctx, _ptr(out), self._stream()))
        return out

    # ------------------------------------------------------------------ step-level API
    def policy_actions(self, obs, eps=None):
        dev = self.device
        obs = _f32(obs, dev); B = obs.shape[0]
        eps = _f32(eps, dev, (B, self.na))
        actions = torch.empty(B, self.na, dtype=torch.float32, device=dev)
        mean = torch.empty_like(actions)
        self._chk(lib.metrpo_policy_actions(self._ctx, _ptr(obs), _ptr(eps), B, _ptr(actions), _ptr(mean), self._stream()))
        return actions, mean

    def step(self, s, a, sam_mode, model_idx=None, noise=None, want_all=False):
        dev = self.device
        s = _f32(s, dev); B = s.shape[0]
        a = _f32(a, dev, (B, self.na))
        model_idx = _i32(model_idx, dev, (B,)); noise = _f32(noise, dev, (B, self.ns))
        s_next = torch.empty(B, self.ns, dtype=torch.float32, device=dev)
        rew = torch.empty(B, dtype=torch.float32, device=dev)
        done = torch.empty(B, dtype=torch.uint8, device=dev)
        nall = torch.empty(self.K, B, self.ns, dtype=torch.float32, device=dev) if want_all else None
        self._chk(lib.metrpo_step(self._ctx, _ptr(s), _ptr(a), B, _lib.SAM_MODES[sam_mode], _ptr(model_idx), _ptr(noise),
                                  _ptr(s_next), _ptr(rew), _ptr(done), _ptr(nall), self._stream()))
        return (s_next, rew, done, nall) if want_all else (s_next, rew, done)

    # ------------------------------------------------------------------ open-loop replay of supplied actions
    def rollout_actions(self, init_obs, actions, sam_mode='model_mean', model=None, model_idx=None, noise=None, force_step_loop=False, out=None):
        """metrpo_rollout_actions: T chained step() calls in one call -- init_obs [B, ns], actions [T, B, na] unclipped (clipped inside, never written).
        model: an int (eps_rand: every env uses that head) or a [B] int tensor (eps_rand: a head per env); model_idx [T, B] for step_rand, noise
        [T, B, ns] for model_mean_std.  -> (obs [T+1, B, ns] with row 0 = init_obs, rew [T, B], done [T, B] uint8), device tensors, nothing
        synchronised.  A done neither stops nor resets an env.  out = (obs, rew, done): write into these tensors instead (contiguous, at least that large)."""
        dev = self.device
        init_obs = _f32(init_obs, dev)
        if init_obs.dim() != 2 or init_obs.shape[1] != self.ns:
            raise ValueError("init_obs: expected [B, %d], got %s" % (self.ns, tuple(init_obs.shape)))
        B = init_obs.shape[0]
        actions = _f32(actions, dev)
        if actions.dim() != 3 or actions.shape[1] != B or actions.shape[2] != self.na:
            raise ValueError("actions: expected [T, %d, %d], got %s" % (B, self.na, tuple(actions.shape)))
        T = actions.shape[0]
        a = _lib.RolloutActionsArgs()
        a.B, a.T, a.sam_mode, a.uniform_model, a.force_step_loop = B, T, _lib.SAM_MODES[sam_mode], -1, int(bool(force_step_loop))
        d_model = None
        if model is not None:
            if isinstance(model, (int, np.integer)):
                a.uniform_model = int(model)
            else:
                d_model = _i32(model, dev, (B,))
        model_idx = _i32(model_idx, dev, (T, B)); noise = _f32(noise, dev, (T, B, self.ns))
        if out is None:
            out = (torch.empty(T + 1, B, self.ns, dtype=torch.float32, device=dev), torch.empty(T, B, dtype=torch.float32, device=dev),
                   torch.empty(T, B, dtype=torch.uint8, device=dev))
        obs, rew, done = out
        assert obs.dtype == torch.float32 and rew.dtype == torch.float32 and done.dtype == torch.uint8 and all(t.is_contiguous() for t in out)
        assert obs.numel() >= (T + 1) * B * self.ns and rew.numel() >= T * B and done.numel() >= T * B
        a.d_init_obs, a.d_actions = init_obs.data_ptr(), actions.data_ptr()
        for name, t in (('d_model', d_model), ('d_model_idx', model_idx), ('d_sel_noise', noise)):
            setattr(a, name, t.data_ptr() if t is not None else None)
        a.d_obs, a.d_rew, a.d_done = obs.data_ptr(), rew.data_ptr(), done.data_ptr()
        self._chk(lib.metrpo_rollout_actions(self._ctx, C.byref(a), self._stream()))
        self._ra_keep = (init_obs, actions, d_model, model_idx, noise)             # alive until the stream has consumed them
        return obs, rew, done

    def last_rollout_actions_kernel(self):
        """Path the last rollout_actions() (or model_error(known_actions=True)) of this engine took: 'fused' (all steps in one launch,
        rollout_actions.hip), 'step-loop' (step()'s kernel once per step); None before the first."""
        return {0: 'step-loop', 1: 'fused'}.get(int(lib.metrpo_last_rollout_actions_kernel(self._ctx)))

    # ------------------------------------------------------------------ disagreement of the heads at supplied rows
    DISAGREEMENT_OUTPUTS = ('score', 'maxdev', 'std', 'mean', 'next_all', 'rew_std', 'sums')

    def ensemble_disagreement(self, obs, actions, valid=None, rows_per_group=0, want=('score',), force_generic=False, out=None):
        """metrpo_ensemble_disagreement: how far the K heads' next states lie apart at every supplied (s, a) row -- obs [N, ns] and actions [N, na]
        (unclipped, clipped inside, never written), or time-major [T, B, .] (flattened; rows_per_group then defaults to B: one group per step).
        valid [N] (nonzero = use the row; a skipped row reads 0 in every output and is left out of `sums`).  want: any of
        score [N] (||std over the heads||_2), maxdev [N] (max_k ||s'_k - mean||_2), std [N, ns], mean [N, ns], next_all [K, N, ns], rew_std [N],
        sums [G, 4] float64 (valid rows, sum score, sum score^2, max score per group of rows_per_group rows; 0: one group).
        -> dict of device tensors (time-major inputs: the leading N is [T, B]), nothing synchronised.  out: dict name -> tensor to write into instead
        (contiguous, at least that large)."""
        dev = self.device
        obs = _f32(obs, dev); actions = _f32(actions, dev)
        lead = tuple(obs.shape[:-1])
        if obs.dim() not in (2, 3) or obs.shape[-1] != self.ns:
            raise ValueError("obs: expected [N, %d] or [T, B, %d], got %s" % (self.ns, self.ns, tuple(obs.shape)))
        if tuple(actions.shape) != lead + (self.na,):
            raise ValueError("actions: expected %s, got %s" % (lead + (self.na,), tuple(actions.shape)))
        want = (want,) if isinstance(want, str) else tuple(want)
        for w in want:
            if w not in self.DISAGREEMENT_OUTPUTS:
                raise ValueError("want: %r is none of %s" % (w, self.DISAGREEMENT_OUTPUTS))
        rows_per_group = int(rows_per_group)
        if rows_per_group < 0:
            raise ValueError("rows_per_group must not be negative")
        if obs.dim() == 3 and rows_per_group == 0:
            rows_per_group = int(obs.shape[1])
        N = 1
        for n in lead:
            N *= int(n)
        if valid is not None:
            valid = torch.as_tensor(valid, device=dev)
            valid = (valid != 0).to(torch.uint8).contiguous()
            if tuple(valid.shape) != lead:
                raise ValueError("valid: expected %s, got %s" % (lead, tuple(valid.shape)))
        G = (N + rows_per_group - 1) // rows_per_group if rows_per_group > 0 else 1
        shapes = {'score': lead, 'maxdev': lead, 'std': lead + (self.ns,), 'mean': lead + (self.ns,), 'next_all': (self.K,) + lead + (self.ns,),
                  'rew_std': lead, 'sums': (G, 4)}
        res = {}
        for w in want:
            dt = torch.float64 if w == 'sums' else torch.float32
            if out is not None and w in out:
                t = out[w]
                assert t.dtype == dt and t.is_contiguous() and t.device == dev and t.numel() >= int(np.prod(shapes[w], dtype=np.int64))
            else:
                t = torch.empty(shapes[w], dtype=dt, device=dev)
            res[w] = t
        a = _lib.DisagreementArgs()
        a.N, a.rows_per_group, a.force_generic = N, rows_per_group, int(bool(force_generic))
        a.d_obs, a.d_actions, a.d_valid = obs.data_ptr(), actions.data_ptr(), (valid.data_ptr() if valid is not None else None)
        for w in self.DISAGREEMENT_OUTPUTS:
            setattr(a, 'd_' + w, res[w].data_ptr() if w in res else None)
        self._chk(lib.metrpo_ensemble_disagreement(self._ctx, C.byref(a), self._stream()))
        self._dis_keep = (obs, actions, valid)                                     # alive until the stream has consumed them
        return res

    def last_disagreement_kernel(self):
        """Path the last ensemble_disagreement() of this engine took: 'fused' (disagreement.hip: one launch over all rows), 'generic' (step()'s kernel
        with want_all, then a reduction kernel); None before the first."""
        return {0: 'generic', 1: 'fused'}.get(int(lib.metrpo_last_disagreement_kernel(self._ctx)))

    # ------------------------------------------------------------------ what the four scoring calls below share
    def _score_starts(self, init_obs):
        """init_obs [S, ns] or [ns] -> (the device tensor [S, ns], S)"""
        init_obs = _f32(init_obs, self.device)
        if init_obs.dim() == 1:
            init_obs = init_obs.unsqueeze(0)
        if init_obs.dim() != 2 or init_obs.shape[1] != self.ns or init_obs.shape[0] < 1:
            raise ValueError("init_obs: expected [S, %d] or [%d], got %s" % (self.ns, self.ns, tuple(init_obs.shape)))
        return init_obs, init_obs.shape[0]

    def _score_sequences(self, seq, name, S, T=None):
        """The candidates' [T, B, na] sequences (name: 'actions' or 'noise') -> (the device tensor, T, B); noise=None: (None, T=, S)."""
        if seq is None and name == 'noise':
            if T is None or int(T) < 0:
                raise ValueError("noise=None needs T= (the number of steps), got %r" % (T,))
            return None, int(T), S
        seq = _f32(seq, self.device)
        if seq.dim() != 3 or seq.shape[2] != self.na or seq.shape[1] % S != 0:
            raise ValueError("%s: expected [T, B, %d] with B a multiple of %d, got %s" % (name, self.na, S, tuple(seq.shape)))
        if T is not None and int(T) != int(seq.shape[0]):
            raise ValueError("T = %r does not match %s %s" % (T, name, tuple(seq.shape)))
        return seq, int(seq.shape[0]), int(seq.shape[1])

    def _score_call(self, fn, a, names, want, out, init_obs, S, T, B, gamma, stop_at_done, force_generic, chunk=None):
        """Checks want / gamma / chunk, allocates the outputs (names[0] is always computed), fills the args struct `a` -- the caller has set what only its
        call has -- and enqueues fn.  -> dict name -> device tensor"""
        dev = self.device
        want = (want,) if isinstance(want, str) else tuple(want)
        for w in want:
            if w not in names:
                raise ValueError("want: %r is none of %s" % (w, names))
        if not np.isfinite(float(gamma)):
            raise ValueError("gamma must be finite")
        if chunk is not None:
            if int(chunk) < 0:
                raise ValueError("chunk must not be negative")
            a.chunk = int(chunk)
        K, ns, na = self.K, self.ns, self.na
        shapes = {'ret': (K, B), 'len': (K, B), 'ret_mean': (B,), 'ret_std': (B,), 'act_out': (K, T, B, na), 'grad': (K, T, B, na), 'grad_mean': (T, B, na),
                  'lam0': (K, B, ns)}
        res = {}
        for w in names[:1] + tuple(x for x in want if x != names[0]):
            dt = torch.int32 if w == 'len' else torch.float32
            if out is not None and w in out:
                t = out[w]
                assert t.dtype == dt and t.is_contiguous() and t.device == dev and t.numel() >= int(np.prod(shapes[w], dtype=np.int64))
            else:
                t = torch.empty(shapes[w], dtype=dt, device=dev)
            res[w] = t
        a.B, a.T, a.S, a.stop_at_done, a.force_generic, a.gamma = B, T, S, int(bool(stop_at_done)), int(bool(force_generic)), float(gamma)
        a.d_init_obs = init_obs.data_ptr()
        for w in names:
            setattr(a, 'd_' + w, res[w].data_ptr() if w in res else None)
        self._chk(fn(self._ctx, C.byref(a), self._stream()))
        return res

    # ------------------------------------------------------------------ every head's return of candidate action sequences
    SCORE_ACTIONS_OUTPUTS = ('ret', 'len', 'ret_mean', 'ret_std')

    def score_actions(self, init_obs, actions, gamma=1.0, stop_at_done=True, want=('ret',), force_generic=False, out=None):
        """metrpo_score_actions: the discounted return each of the K heads predicts for each of B candidate action sequences -- init_obs [S, ns] or
        [ns] (S start states, B % S == 0: candidate b starts from init_obs[b // (B // S)]), actions [T, B, na] unclipped (clipped inside, never written).
        Head k rolls its own trajectory (rollout_actions(sam_mode='eps_rand', model=k)); stop_at_done: a candidate stops counting behind its first done
        (the step that ends it still counts), False: every step counts.  want: any of ret [K, B], len [K, B] int32 (steps counted), ret_mean [B],
        ret_std [B] (population std over the heads); ret is always computed.  -> dict of device tensors, nothing synchronised.  out: dict name ->
        tensor to write into instead (contiguous, at least that large)."""
        init_obs, S = self._score_starts(init_obs)
        actions, T, B = self._score_sequences(actions, 'actions', S)
        a = _lib.ScoreActionsArgs()
        a.d_actions = actions.data_ptr()
        res = self._score_call(lib.metrpo_score_actions, a, self.SCORE_ACTIONS_OUTPUTS, want, out, init_obs, S, T, B, gamma, stop_at_done, force_generic)
        self._sa_keep = (init_obs, actions)                                        # alive until the stream has consumed them
        return res

    def last_score_actions_kernel(self):
        """Path the last score_actions() of this engine took: 'fused' (score_actions.hip: one launch, a wave per (tile, head)), 'generic' (per head
        the step loop of rollout_actions, then a reduction kernel); None before the first."""
        return {0: 'generic', 1: 'fused'}.get(int(lib.metrpo_last_score_actions_kernel(self._ctx)))

    # ------------------------------------------------------------------ every head's return of candidate noise sequences around the policy
    SCORE_POLICY_ACTIONS_OUTPUTS = ('ret', 'len', 'ret_mean', 'ret_std', 'act_out')

    def score_policy_actions(self, init_obs, noise=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False, want=('ret',), force_generic=False,
                             out=None):
        """metrpo_score_policy_actions: the discounted return each of the K heads predicts for each of B candidate NOISE sequences around the policy --
        score_actions with a_t = clip(policy mean(s_t) + noise_t) formed from the head's own state at every step (noise_in_std: noise_t in units of
        the policy's std, get_actions' arithmetic).  init_obs [S, ns] or [ns], noise [T, B, na] with B % S == 0 (candidate b starts from
        init_obs[b // (B // S)]; never written), or None: the deterministic policy for T= steps, B = S.  want: any of ret [K, B], len [K, B] int32,
        ret_mean [B], ret_std [B], act_out [K, T, B, na] (the UNCLIPPED action head k's trajectory took); ret is always computed.  -> dict of device
        tensors, nothing synchronised.  out: dict name -> tensor to write into instead (contiguous, at least that large)."""
        init_obs, S = self._score_starts(init_obs)
        noise, T, B = self._score_sequences(noise, 'noise', S, T)
        a = _lib.ScorePolicyActionsArgs()
        a.noise_in_std, a.d_noise = int(bool(noise_in_std)), (noise.data_ptr() if noise is not None else None)
        res = self._score_call(lib.metrpo_score_policy_actions, a, self.SCORE_POLICY_ACTIONS_OUTPUTS, want, out, init_obs, S, T, B, gamma, stop_at_done,
                               force_generic)
        self._spa_keep = (init_obs, noise)                                         # alive until the stream has consumed them
        return res

    def last_score_policy_actions_kernel(self):
        """Path the last score_policy_actions() of this engine took: 'fused' (score_policy_actions.hip: one launch, a wave per (tile, head)), 'generic'
        (per head and step the policy_actions and step launches, then a reduction kernel); None before the first."""
        return {0: 'generic', 1: 'fused'}.get(int(lib.metrpo_last_score_policy_actions_kernel(self._ctx)))

    # ------------------------------------------------------------------ gradient of every head's return with respect to the candidate actions
    SCORE_ACTIONS_GRAD_OUTPUTS = ('grad', 'ret', 'len', 'grad_mean', 'lam0')

    def score_actions_grad(self, init_obs, actions, gamma=1.0, stop_at_done=True, want=('grad', 'ret'), force_generic=False, chunk=0, out=None):
        """metrpo_score_actions_grad: the gradient of each head's predicted return (score_actions' ret) with respect to the UNCLIPPED candidate actions
        -- the ascent direction -- for init_obs [S, ns] or [ns] and actions [T, B, na] as in score_actions.  want: any of grad [K, T, B, na] (always
        computed; 0 where the action is clipped and behind a candidate's last counted step), ret [K, B], len [K, B] int32, grad_mean [T, B, na] (the
        heads' mean, summed in head order), lam0 [K, B, ns] (the gradient with respect to the start state).  chunk: candidates per pass of the
        workspace (0: the library's rule); it changes no bit of any output.  -> dict of device tensors, nothing synchronised.  out: dict name ->
        tensor to write into instead (contiguous, at least that large)."""
        init_obs, S = self._score_starts(init_obs)
        actions, T, B = self._score_sequences(actions, 'actions', S)
        a = _lib.ScoreActionsGradArgs()
        a.d_actions = actions.data_ptr()
        res = self._score_call(lib.metrpo_score_actions_grad, a, self.SCORE_ACTIONS_GRAD_OUTPUTS, want, out, init_obs, S, T, B, gamma, stop_at_done,
                               force_generic, chunk)
        self._sag_keep = (init_obs, actions)                                       # alive until the stream has consumed them
        return res

    def last_score_actions_grad_kernel(self):
        """Path the last score_actions_grad() of this engine took: 'fused' (score_actions_grad.hip: a forward and a reverse launch per chunk on the
        matrix instructions), 'generic' (one thread per (candidate, head)); None before the first."""
        return {0: 'generic', 1: 'fused'}.get(int(lib.metrpo_last_score_actions_grad_kernel(self._ctx)))

    # ------------------------------------------------------------------ gradient of every head's closed-loop return with respect to the noise
    SCORE_POLICY_ACTIONS_GRAD_OUTPUTS = ('grad', 'ret', 'len', 'grad_mean', 'lam0', 'act_out')

    def score_policy_actions_grad(self, init_obs, noise=None, T=None, gamma=1.0, stop_at_done=True, noise_in_std=False, want=('grad', 'ret'),
                                  force_generic=False, chunk=0, out=None):
        """metrpo_score_policy_actions_grad: the gradient of each head's closed-loop return (score_policy_actions' ret) with respect to the candidate
        NOISE sequences -- the ascent direction, TOTAL: the policy of every later step sees the states a noise moved -- for init_obs [S, ns] or [ns]
        and noise [T, B, na] as in score_policy_actions (None: the gradient at noise = 0 for T= steps, B = S).  want: any of grad [K, T, B, na]
        (always computed; 0 where the head's action is clipped and behind a candidate's last counted step), ret [K, B], len [K, B] int32, grad_mean
        [T, B, na] (the heads' mean, summed in head order), lam0 [K, B, ns] (the gradient with respect to the start state, policy path included),
        act_out [K, T, B, na].  ret, len and act_out carry score_policy_actions' bits on the same path.  chunk: candidates per pass of the workspace
        (0: the library's rule); it changes no bit of any output.  -> dict of device tensors, nothing synchronised.  out: dict name -> tensor to
        write into instead (contiguous, at least that large)."""
        init_obs, S = self._score_starts(init_obs)
        noise, T, B = self._score_sequences(noise, 'noise', S, T)
        a = _lib.ScorePolicyActionsGradArgs()
        a.noise_in_std, a.d_noise = int(bool(noise_in_std)), (noise.data_ptr() if noise is not None else None)
        res = self._score_call(lib.metrpo_score_policy_actions_grad, a, self.SCORE_POLICY_ACTIONS_GRAD_OUTPUTS, want, out, init_obs, S, T, B, gamma,
                               stop_at_done, force_generic, chunk)
        self._spag_keep = (init_obs, noise)                                        # alive until the stream has consumed them
        return res

    def last_score_policy_actions_grad_kernel(self):
        """Path the last score_policy_actions_grad() of this engine took: 'fused' (score_policy_actions_grad.hip: a forward and a reverse launch per
        chunk on the matrix instructions), 'generic' (one thread per (candidate, head)); None before the first."""
        return {0: 'generic', 1: 'fused'}.get(int(lib.metrpo_last_score_policy_actions_grad_kernel(self._ctx)))

    # ------------------------------------------------------------------ terminal value of the four scoring calls
    def set_terminal_value(self, w1, w2, bias):
        """Terminal value of score_actions / score_actions_grad / score_policy_actions / score_policy_actions_grad (include/metrpo.h):
        V(s) = bias + sum_d (w1[d] o_d + w2[d] o_d^2), o = clip(s, -10, 10); ret gains gamma^T alive_T V(s_T), the gradients start from the
        matching seed.  w1, w2 [ns]; bias a scalar, or [S]: one per start state of the scoring call (candidate b uses bias[b // (B // S)]).
        Tensors or arrays.  planning.baseline_terminal_value forms the three from a LinearFeatureBaseline fit.  Stays set until
        clear_terminal_value(); every other call ignores it.  Stream-ordered like the scoring calls: nothing is synchronised."""
        dev = self.device
        a = _f32(w1, dev, (self.ns,)); b = _f32(w2, dev, (self.ns,))
        c = _f32(bias, dev).reshape(-1)
        self._chk(lib.metrpo_set_terminal_value(self._ctx, _ptr(a), _ptr(b), _ptr(c), int(c.numel()), self._stream()))
        self._tv_keep = (a, b, c)                                                  # alive until the stream has consumed them

    def set_terminal_value_mlp(self, params, hidden, bias=0.0):
        """The terminal value's second form (include/metrpo.h: metrpo_set_terminal_value_mlp), a two-layer tanh net on o = clip(s, -10, 10):
        V(s) = bias + b2 + W2 . tanh(W1^T tanh(W0^T o + b0) + b1).  params: the packed vector W0 [ns][h1] | b0 | W1 [h1][h2] | b1 | W2 [h2] | b2
        (planning.ValueMLP.packed() forms it, input normaliser folded in); hidden = (h1, h2), each in 1 .. 32; bias a scalar, or [S] as in
        set_terminal_value.  Replaces a quadratic value that is set, and is replaced by one; clear_terminal_value() clears either."""
        dev = self.device
        h1, h2 = (int(h) for h in hidden)
        n = self.ns * h1 + h1 + h1 * h2 + h2 + h2 + 1
        p = _f32(params, dev, (n,))
        c = _f32(bias, dev).reshape(-1)
        self._chk(lib.metrpo_set_terminal_value_mlp(self._ctx, _ptr(p), h1, h2, _ptr(c), int(c.numel()), self._stream()))
        self._tv_keep = (p, c)                                                     # alive until the stream has consumed them

    def clear_terminal_value(self):
        self._chk(lib.metrpo_clear_terminal_value(self._ctx))

    @property
    def terminal_value_kind(self):
        """0 while no terminal value is set, 1: the quadratic form (set_terminal_value), 2: the MLP (set_terminal_value_mlp)."""
        return int(lib.metrpo_terminal_value_kind(self._ctx))

    @property
    def terminal_value(self):
        """0 while no terminal value is set, else the number of biases it holds (1, or S)."""
        return int(lib.metrpo_has_terminal_value(self._ctx))

    # ------------------------------------------------------------------ fused rollout
    def rollout(self, B, T, H, sam_mode, pool, determ=False, eval_all_heads=True, seed=0, stream_offset=0,
                eps=None, model_idx=None, sel_noise=None, reset_idx=None, reset_model=None, out=None,
                force_generic=False, t0=0, resume=None, last_state=None, stop=None, stop_batch=0, stop_cum=None):
        """`resume` = (obs [B,ns] f32, ts [B] i32, model [B] i32) continues a chunked rollout at global step `t0` (the supplied
        draw tensors are then indexed from this chunk's first step); `last_state` = (ts, model) int32 output tensors;
        `stop` = int32 device flag that turns the call into a no-op when set (metrpo_sampler_progress); `stop_batch` > 0 with `stop_cum` (float64 device
        scalar: samples completed in front of this call) lets a one-launch kernel family apply the sampler's stop rule inside the call (rows behind the stop
        step are then undefined)."""
        dev = self.device
        # launch fast path (the bench / training loop): same buffers, same modes, production draws -> only the seed changes in the cached struct
        no_draws = eps is None and model_idx is None and sel_noise is None and reset_idx is None and reset_model is None
        chunked = resume is not None or last_state is not None or stop is not None or t0 != 0 or stop_batch
        if no_draws and not chunked and out is not None and not force_generic and isinstance(pool, torch.Tensor):
            key = (id(out), pool.data_ptr(), B, T, H, sam_mode, bool(determ), bool(eval_all_heads), int(stream_offset))
            cached = getattr(self, '_ra_cache', None)
            if cached is not None and cached[0] == key:
                a = cached[1]
                a.seed = int(seed)
                self._chk(lib.metrpo_rollout(self._ctx, C.byref(a), self._stream()))
                return out
        pool = _f32(pool, dev); assert pool.dim() == 2 and pool.shape[1] == self.ns
        eps = _f32(eps, dev, (T, B, self.na)); sel_noise = _f32(sel_noise, dev, (T, B, self.ns))
        model_idx = _i32(model_idx, dev, (T, B))
        reset_idx = _i32(reset_idx, dev, (T + 1, B)); reset_model = _i32(reset_model, dev, (T + 1, B))
        if out is None:
            out = self.alloc_trajectory(B, T, H)
        a = _lib.RolloutArgs()
        a.B, a.T, a.H, a.sam_mode = B, T, H, _lib.SAM_MODES[sam_mode]
        a.determ, a.eval_all_heads = int(bool(determ)), int(bool(eval_all_heads))
        a.d_pool, a.n_pool, a.seed, a.stream_offset = pool.data_ptr(), pool.shape[0], int(seed), int(stream_offset)
        for name, t in (('d_eps', eps), ('d_model_idx', model_idx), ('d_sel_noise', sel_noise),
                        ('d_reset_idx', reset_idx), ('d_reset_model', reset_model)):
            setattr(a, name, t.data_ptr() if t is not None else None)
        a.d_obs, a.d_act, a.d_rew, a.d_mean = out.obs.data_ptr(), out.act.data_ptr(), out.rew.data_ptr(), out.mean.data_ptr()
        a.d_done, a.d_tpath, a.d_last_obs = out.done.data_ptr(), out.tpath.data_ptr(), out.last_obs.data_ptr()
        a.t0 = int(t0)
        if resume is not None:
            r_obs, r_ts, r_model = resume
            assert r_obs.dtype == torch.float32 and r_ts.dtype == torch.int32 and r_model.dtype == torch.int32
            assert tuple(r_obs.shape) == (B, self.ns) and r_ts.numel() == B and r_model.numel() == B
            a.d_init_obs, a.d_init_ts, a.d_init_model = r_obs.data_ptr(), r_ts.data_ptr(), r_model.data_ptr()
        if last_state is not None:
            assert all(t.dtype == torch.int32 and t.numel() == B for t in last_state)
            a.d_last_ts, a.d_last_model = last_state[0].data_ptr(), last_state[1].data_ptr()
        if stop is not None:
            assert stop.dtype == torch.int32
            a.d_stop = stop.data_ptr()
        if stop_batch:
            assert stop_cum is not None and stop_cum.dtype == torch.float64 and stop_cum.is_cuda
            a.stop_batch, a.d_stop_cum = int(stop_batch), stop_cum.data_ptr()
        fn = lib.metrpo_rollout_generic if force_generic else lib.metrpo_rollout
        self._chk(fn(self._ctx, C.byref(a), self._stream()))
        self._keep = (pool, eps, model_idx, sel_noise, reset_idx, reset_model, resume, last_state, stop, stop_cum)   # alive until the stream has consumed them
        if no_draws and not chunked and not force_generic:
            self._ra_cache = ((id(out), pool.data_ptr(), B, T, H, sam_mode, bool(determ), bool(eval_all_heads), int(stream_offset)), a, out, pool)
        return out

    def sampler_progress(self, done, tpath, t0, batch_size, counts, state, stop):
        """Loop condition of obtain_samples for the chunk (done, tpath [T,B]) that starts at global step t0; see metrpo.h."""
        T, B = done.shape
        assert counts.dtype == torch.float64 and counts.numel() >= T and state.dtype == torch.float64 and stop.dtype == torch.int32
        self._chk(lib.metrpo_sampler_progress(self._ctx, _ptr(done), _ptr(tpath), int(T), int(B), int(t0), int(batch_size),
                                              _ptr(counts), _ptr(state), _ptr(stop), self._stream()))

    def rollout_path(self):
        """7 step-wise GEMM with bf16 operands (set_dyn_precision('bf16')), 3 step-wise GEMM (large nets), 2 cooperative-heads MFMA, 1 head-per-wave MFMA,
        0 generic (current selection)."""
        if self.dyn_precision == 'bf16':
            return 7
        return int(lib.metrpo_set_rollout_variant(self._ctx, int(getattr(self, '_variant', 0))))

    def last_rollout_kernel(self):
        """Kernel family the last rollout() of this engine ran on: 'generic', 'mfma-head-per-wave', 'mfma-cooperative', 'gemm-stepwise',
        'resident' (whole time loop in one launch, rollout_resident.hip), 'gemm-streamk' (step-wise, the whole ensemble of a step in one
        evenly split launch, mlp_streamk.h), 'streamk-persistent' (all steps of a chunk in one launch, rollout_persist.hip), 'gemm-bf16' (step-wise tile GEMMs
        on bf16 operands, rollout_bf16.hip: set_dyn_precision('bf16')); None before the first rollout."""
        k = int(lib.metrpo_last_rollout_kernel(self._ctx))
        return {0: 'generic', 1: 'mfma-head-per-wave', 2: 'mfma-cooperative', 3: 'gemm-stepwise', 4: 'resident', 5: 'gemm-streamk', 6: 'streamk-persistent', 7: 'gemm-bf16'}.get(k)

    ROLLOUT_LAUNCH_FIELDS = ('family', 'pre', 'post_width', 'sk_mode', 'late', 'l0', 'fuse_tile', 'out_splits', 'persist_wide', 'nclose', 'rounds',
                             'res_ws', 'res_threads', 'res_pw', 'res_rg', 'res_rot')

    def last_rollout_launch(self):
        """Diagnostics: the sub-form of the last rollout() on a GEMM-class or resident family, as the host noted it while it enqueued it: dict(family (as
        last_rollout_kernel), pre 'mfma' | 'mfma-merged' | 'mfma3' | 'mfma3-split' | 'gemm-chain' | 'valu' | 'mfma3-merged' (None: no pre-step launch),
        post_width (k_big_post's lanes per env, 0 where a persistent or resident launch closes the steps), sk_mode 0 ... 3, late, l0 'producer' | 'rows' |
        'gemm', fuse_tile 0 ... 2, out_splits (partials of the output layer added by the closing kernel), persist_wide, nclose, rounds 'single' |
        'parallel' | 'merged', res_ws / res_threads / res_pw / res_rg / res_rot (resident: slice width, threads, post waves per workgroup, rounds per
        launch group, rotating deal))."""
        out = (C.c_int32 * 16)()
        self._chk(lib.metrpo_debug_last_rollout_launch(self._ctx, out))
        d = dict(zip(self.ROLLOUT_LAUNCH_FIELDS, (int(x) for x in out)))
        d['family'] = self.last_rollout_kernel()
        d['pre'] = {0: 'mfma', 1: 'mfma-merged', 2: 'mfma3', 3: 'mfma3-split', 4: 'gemm-chain', 5: 'valu', 6: 'mfma3-merged'}.get(d['pre'])
        d['l0'] = {0: 'producer', 1: 'rows', 2: 'gemm'}.get(d['l0'])
        d['rounds'] = {0: 'single', 1: 'parallel', 2: 'merged'}.get(d['rounds'])
        return d

    def set_coop_split(self, split):
        """False keeps the 4-wave form of the cooperative rollout kernel where the head-split 8-wave form would run (same results bit for bit: A/B
        tests, fallback); True (default) restores the rule.  Read at the next rollout()."""
        self._chk(lib.metrpo_set_coop_split(self._ctx, int(bool(split))))

    def last_coop_waves(self):
        """Waves per workgroup of the last cooperative-kernel launch: 8 = head-split form (two waves per SIMD on one tile), 4 = the 4-wave form
        (set_coop_split(False), two workgroups per CU, K = 1, K > 5, half-cheetah, Ant); 0 before the first."""
        return int(lib.metrpo_debug_coop_waves(self._ctx))

    GEMM_FORM_FIELDS = ('tm', 'tn', 'al', 'pd', 'splits', 'kchunk', 'gx', 'gy', 'gz', 'reduced', 'stride_part')

    def debug_gemm(self, op, epi=0, **fields):
        """Diagnostics: ONE call of the shared MFMA GEMM's host entries (csrc/gemm_mfma.h) on caller-owned float32 device tensors, for
        tests/test_gpu_gemm.py.  op 'auto' (gemm_auto<epi, ta, tb>, or the tile forced with tm, tn = 1 | 2), 'skinny' (gemm_skinny_bias) or
        'fused_out' (gemm_relu_fused_out); epi a name of _lib.GEMM_EPIS.  The other fields are those of _lib.DebugGemmArgs; a pointer field
        takes a tensor or (tensor, offset in floats).  The caller sizes every tensor for the extents and strides it passes; no context state
        is read or written.  -> the launched form, a dict over GEMM_FORM_FIELDS."""
        a = _lib.DebugGemmArgs()
        a.op, a.epi = _lib.GEMM_DEBUG_OPS[op], _lib.GEMM_EPIS[epi] if isinstance(epi, str) else int(epi)
        kinds = dict((n, t) for n, t in _lib.DebugGemmArgs._fields_)
        for name, val in fields.items():
            if kinds[name] is C.c_void_p:
                t, off = val if isinstance(val, tuple) else (val, 0)
                if t is not None:
                    assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device and 0 <= off < t.numel()
                val = None if t is None else t.data_ptr() + 4 * int(off)
            setattr(a, name, val)
        self._chk(lib.metrpo_debug_gemm(self._ctx, C.byref(a), self._stream()))
        return dict((n, int(getattr(a, 'o_' + n))) for n in self.GEMM_FORM_FIELDS)

    BF16_GEMM_FORM_FIELDS = ('bn', 'gx', 'gy', 'gz', 'n_cu')

    def debug_gemm_bf16(self, op, **fields):
        """Diagnostics: ONE launch of the bf16 dynamics forward's own kernels (csrc/rollout_bf16.hip) on caller-owned device tensors, for
        tests/test_gpu_bf16_gemm.py.  op 'image' (k_bf16_wimage: W float32 [heads][Kd][N] -> C int16 [heads][N][Kp]) or 'gemm' (gemm_bf16_pick:
        a_bf16 / c_bf16 choose the element types, float32 or int16 tensors holding bf16 bits; bn = 0 leaves the tile to the rule, 64 / 128 force
        it).  The other fields are those of _lib.DebugGemmBf16Args; a pointer field takes a tensor.  The caller sizes every tensor for the
        extents and strides it passes; no context state is read or written.  -> the launched form, a dict over BF16_GEMM_FORM_FIELDS."""
        a = _lib.DebugGemmBf16Args()
        a.op = _lib.GEMM_BF16_DEBUG_OPS[op] if isinstance(op, str) else int(op)
        kinds = dict((n, t) for n, t in _lib.DebugGemmBf16Args._fields_)
        for name, val in fields.items():
            if kinds[name] is C.c_void_p and val is not None:
                assert val.dtype in (torch.float32, torch.int16) and val.is_contiguous() and val.device == self.device
                val = val.data_ptr()
            setattr(a, name, val)
        self._chk(lib.metrpo_debug_gemm_bf16(self._ctx, C.byref(a), self._stream()))
        return dict((n, int(getattr(a, 'o_' + n))) for n in self.BF16_GEMM_FORM_FIELDS)

    def debug_env_model(self, env, x_next, u, w, compile_time=False):
        """Diagnostics: ONE launch that evaluates the reward model (csrc/env_model.h) of environment `env` (a name of _lib.ENV_IDS, any engine) on
        float32 device tensors x_next [N][ns], u [N][na], w [N], for tests/test_gpu_env_model.py.  compile_time picks the kernel instantiated on
        the environment (the five 2 x 64 environments) instead of the one that takes it at run time.  -> dict(cost [N], done [N] int32,
        gx [N][ns] = d(w cost)/dx_next dimension by dimension, gx_row = the same in the row form added into zeros, gu [N][na] = d(w cost)/du)."""
        for t in (x_next, u, w):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device
        N, ns = x_next.shape
        na = u.shape[1]
        assert u.shape[0] == N and tuple(w.shape) == (N,)
        out = dict(cost=torch.empty(N, dtype=torch.float32, device=self.device), done=torch.empty(N, dtype=torch.int32, device=self.device),
                   gx=torch.empty_like(x_next), gx_row=torch.empty_like(x_next), gu=torch.empty_like(u))
        a = _lib.DebugEnvModelArgs()
        a.env, a.ns, a.na, a.N, a.compile_time = _lib.ENV_IDS[env], ns, na, N, int(bool(compile_time))
        a.x, a.u, a.w = x_next.data_ptr(), u.data_ptr(), w.data_ptr()
        for name, t in out.items():
            setattr(a, name, t.data_ptr())
        self._chk(lib.metrpo_debug_env_model(self._ctx, C.byref(a), self._stream()))
        return out

    def last_bf16_layers(self):
        """Diagnostics: the column tile (64 or 128) of every dynamics-layer GEMM of the last bf16 rollout's steps, as the host noted it when it
        enqueued them; [] before the first bf16 rollout."""
        out = (C.c_int32 * 8)()
        self._chk(lib.metrpo_debug_last_bf16_layers(self._ctx, out))
        return [int(out[1 + l]) for l in range(int(out[0]))]

    def rollout_note(self):
        """Why the last rollout() ran outside the fast dispatch table (K != 5 at 2x64, hidden widths 65..127, ...); '' when it did not."""
        return lib.metrpo_rollout_note(self._ctx).decode()

    def alloc_trajectory(self, B, T, H):
        dev, f = self.device, torch.float32
        return Trajectory(torch.empty(T, B, self.ns, dtype=f, device=dev), torch.empty(T, B, self.na, dtype=f, device=dev),
                          torch.empty(T, B, dtype=f, device=dev), torch.empty(T, B, self.na, dtype=f, device=dev),
                          torch.empty(T, B, dtype=torch.uint8, device=dev), torch.empty(T, B, dtype=torch.int32, device=dev),
                          torch.empty(B, self.ns, dtype=f, device=dev), B, T, H)

    def validation_cost(self, s0, T, gamma):
        s0 = _f32(s0, self.device); assert s0.shape[1] == self.ns
        costs = torch.empty(self.K, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_validation_cost(self._ctx, _ptr(s0), s0.shape[0], int(T), float(gamma), _ptr(costs), self._stream()))
        return costs

    # ------------------------------------------------------------------ process_samples pieces
    def gae(self, traj, coeffs, gamma, lam, stats=None):
        """-> adv (uncentred), ret, valid, stats[3] = (sum adv, sum adv^2, count) over valid samples."""
        dev = self.device
        T, B = traj.T, traj.B
        adv = torch.empty(T, B, dtype=torch.float32, device=dev); ret = torch.empty_like(adv)
        valid = torch.empty(T, B, dtype=torch.uint8, device=dev)
        if stats is None:
            stats = torch.zeros(3, dtype=torch.float64, device=dev)       # else: caller-provided, already zero
        if coeffs is not None:
            if isinstance(coeffs, torch.Tensor) and coeffs.is_cuda:
                coeffs = coeffs.to(torch.float64).contiguous()
            else:
                # host coefficients: pinned staging + async copy, so that this call does not block the host behind the rollout that is
                # still running on the stream (a pageable H2D copy would) and the GAE kernels are queued while it runs
                F = 2 * self.ns + 4
                if getattr(self, '_coef_pin', None) is None:
                    self._coef_pin = [torch.empty(F, dtype=torch.float64).pin_memory() for _ in range(2)]
                    self._coef_dev = [torch.empty(F, dtype=torch.float64, device=dev) for _ in range(2)]
                    self._coef_i = 0
                self._coef_i ^= 1
                pin, cd = self._coef_pin[self._coef_i], self._coef_dev[self._coef_i]
                pin.copy_(torch.as_tensor(np.asarray(coeffs, dtype=np.float64)))
                cd.copy_(pin, non_blocking=True)
                coeffs = cd
            assert coeffs.numel() == 2 * self.ns + 4
        self._chk(lib.metrpo_gae(self._ctx, _ptr(traj.obs), _ptr(traj.rew), _ptr(traj.done), _ptr(traj.tpath), T, B,
                                 _ptr(coeffs), float(gamma), float(lam), _ptr(adv), _ptr(ret), _ptr(valid), _ptr(stats),
                                 self._stream()))
        return adv, ret, valid, stats

    def process_begin(self, n_acc):
        """-> (old_log_std [na] float32, acc [n_acc] float64 zeros): metrpo_process_begin, one launch for what policy.log_std() + torch.zeros are as three.
        Closes an update that is only enqueued first (as get_policy does): the snapshot must see the policy the rollout ran with."""
        self._close_open_update()
        ls = torch.empty(self.na, dtype=torch.float32, device=self.device)
        acc = torch.empty(int(n_acc), dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_process_begin(self._ctx, _ptr(ls), _ptr(acc), int(n_acc), self._stream()))
        return ls, acc

    def center_advantages(self, adv, valid, stats):
        self._chk(lib.metrpo_center_advantages(self._ctx, _ptr(adv), _ptr(valid), adv.numel(), _ptr(stats), self._stream()))
        return adv

    def baseline_gram(self, obs, ret, tpath, valid, out=None):
        """out: optional zeroed float64 buffer of F*F + F elements (AtA row-major, then Aty) that receives the sums."""
        F = 2 * self.ns + 4
        if out is None:
            out = torch.zeros(F * F + F, dtype=torch.float64, device=self.device)
        AtA, Aty = out[:F * F].view(F, F), out[F * F:]
        self._chk(lib.metrpo_baseline_gram(self._ctx, _ptr(obs), _ptr(ret), _ptr(tpath), _ptr(valid), ret.numel(),
                                           _ptr(AtA), _ptr(Aty), self._stream()))
        return AtA, Aty

    # ------------------------------------------------------------------ TRPO update pieces
    def baseline_solve(self, gram, reg_coeff=1e-5, out=None):
        """LinearFeatureBaseline.fit's solve on the device: gram = [AtA (F*F, row-major) | Aty (F)] float64 device tensor (summed over the
        ranks) -> coefficients [F] float64 on the device, stream-ordered (no host round trip)."""
        F = 2 * self.ns + 4
        assert gram.is_cuda and gram.dtype == torch.float64 and gram.numel() == F * F + F and gram.is_contiguous()
        if out is None:
            out = torch.empty(F, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_baseline_solve(self._ctx, _ptr(gram), C.c_void_p(gram.data_ptr() + 8 * F * F), float(reg_coeff), _ptr(out), self._stream()))
        return out

    def make_batch(self, obs, act, adv, old_mean, old_log_std, valid=None, n_global=None):
        dev = self.device
        obs = _f32(obs, dev).reshape(-1, self.ns); N = obs.shape[0]
        act = _f32(act, dev).reshape(N, self.na); adv = _f32(adv, dev).reshape(N)
        stride = 0
        if old_mean is not None:             # (None: a batch for the VPG update only, which reads no old distribution)
            old_mean = _f32(old_mean, dev).reshape(N, self.na)
        if old_log_std is not None:
            old_log_std = _f32(old_log_std, dev)
            stride = 0 if old_log_std.numel() == self.na else self.na
            if stride:
                old_log_std = old_log_std.reshape(N, self.na)
        if valid is not None:
            valid = torch.as_tensor(valid, device=dev).to(torch.uint8).contiguous().reshape(N)
        if n_global is None:
            n_global = int(valid.sum().item()) if valid is not None else N
        b = _lib.Batch()
        b.d_obs, b.d_act, b.d_adv = obs.data_ptr(), act.data_ptr(), adv.data_ptr()
        b.d_old_mean = old_mean.data_ptr() if old_mean is not None else None
        b.d_old_log_std, b.old_log_std_stride = (old_log_std.data_ptr() if old_log_std is not None else None), stride
        b.d_valid = valid.data_ptr() if valid is not None else None
        b.N, b.inv_n_global = N, 1.0 / float(n_global)
        b._keep = (obs, act, adv, old_mean, old_log_std, valid)
        return b

    def subsample_batch(self, batch, idx, n_global_sub=None):
        """[rllab] ConjugateGradientOptimizer.optimize, subsample_factor < 1: subsample_inputs = tuple(x[inds] for x in inputs), gathered on the
        device (metrpo_subsample_batch).  idx: int32 row indices into `batch` (any order, duplicates allowed).  -> a Batch of len(idx) rows for fvp()
        and trpo_update(fvp_batch=...): observations, old distribution and valid flags live in an engine-owned workspace that stays valid until the
        next subsample_batch of this engine; actions and advantages are not gathered.  n_global_sub = the sub-batch's valid samples over all ranks
        (the denominator of its means); None: this rank's count -- len(idx) without a valid mask, else the gathered flags' sum, read once.
        .valid_count (1-element float64 device tensor) holds this rank's count either way (a sharded caller all-reduces it and sets .inv_n_global)."""
        idx = _i32(idx, self.device).reshape(-1)
        m = int(idx.numel())
        if m == 0:
            raise ValueError("subsample_batch: empty index vector")
        count = torch.zeros(1, dtype=torch.float64, device=self.device)
        sub = _lib.Batch()
        inv = 1.0 / float(n_global_sub) if n_global_sub is not None else 1.0 / m
        self._chk(lib.metrpo_subsample_batch(self._ctx, C.byref(batch), _ptr(idx), m, inv, C.byref(sub), _ptr(count), self._stream()))
        sub.valid_count = count
        sub._keep = (idx, batch)             # (a broadcast old_log_std is still the source batch's tensor)
        if n_global_sub is None and batch.d_valid:
            n = int(count.item())
            if n == 0:
                raise ValueError("subsample_batch: none of the %d gathered rows is valid" % m)
            sub.inv_n_global = 1.0 / n
        return sub

    def batch_tensors(self, batch):
        """Copies of the device arrays a Batch points to (diagnostics / tests): dict(obs, old_mean, old_log_std, valid); None where the pointer is."""
        N, dev = int(batch.N), self.device

        def view(ptr, count, typestr, shape):
            return torch.as_tensor(_DevView(ptr, count, typestr), device=dev).clone().reshape(shape) if ptr else None
        n_ls = N * self.na if batch.old_log_std_stride else self.na
        return dict(obs=view(batch.d_obs, N * self.ns, '<f4', (N, self.ns)), old_mean=view(batch.d_old_mean, N * self.na, '<f4', (N, self.na)),
                    old_log_std=view(batch.d_old_log_std, n_ls, '<f4', (-1, self.na)), valid=view(batch.d_valid, N, '|u1', (N,)))

    def loss_grad(self, batch):
        out = torch.empty(self.P + 1, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_loss_grad(self._ctx, C.byref(batch), _ptr(out), self._stream()))
        return out

    def vpg_loss_grad(self, batch):
        """VPG surrogate (algos/vpg.py:88) -mean(logli * adv) and its gradient: tensor [1 + P] float64, loss_grad's layout (this rank's share)."""
        out = torch.empty(self.P + 1, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_vpg_loss_grad(self._ctx, C.byref(batch), _ptr(out), self._stream()))
        return out

    def vpg_update(self, batch, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, want_loss=True):
        """One VPG optimize_policy (vpg.py:100-118): one TF-Adam step on the whole batch's gradient, the state of get_policy_adam /
        set_policy_adam, summed over the ranks by the communicator attached to this engine (if any).  Stream-ordered, no synchronisation;
        returns the loss at the entry theta as a 1-element float64 device tensor (None with want_loss=False)."""
        self._close_open_update()
        p = _lib.VpgParams()
        p.lr, p.beta1, p.beta2, p.eps = float(lr), float(beta1), float(beta2), float(eps)
        loss = torch.empty(1, dtype=torch.float64, device=self.device) if want_loss else None
        self._chk(lib.metrpo_vpg_update(self._ctx, C.byref(batch), C.byref(p), _ptr(loss), self._stream()))
        return loss

    @staticmethod
    def _ppo_params(clip_lr, entropy_bonus_coeff, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        p = _lib.PpoParams()
        p.clip_lr, p.entropy_bonus_coeff = float(clip_lr), float(entropy_bonus_coeff)
        p.lr, p.beta1, p.beta2, p.eps = float(lr), float(beta1), float(beta2), float(eps)
        return p

    def ppo_loss_grad(self, batch, clip_lr=0.3, entropy_bonus_coeff=0.0):
        """PPO's clipped surrogate with the entropy bonus (algos/ppo.py:107-119) and its gradient at the ctx policy: tensor [1 + P] float64,
        loss_grad's layout.  The surrogate part is this rank's share; the entropy term is added whole (a host-driven all-reduce over W ranks
        passes entropy_bonus_coeff / W)."""
        out = torch.empty(self.P + 1, dtype=torch.float64, device=self.device)
        p = self._ppo_params(clip_lr, entropy_bonus_coeff)
        self._chk(lib.metrpo_ppo_loss_grad(self._ctx, C.byref(batch), C.byref(p), _ptr(out), self._stream()))
        return out

    def ppo_update(self, batch, n_epochs=10, clip_lr=0.3, entropy_bonus_coeff=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, want_losses=True):
        """One PPO optimize_policy (ppo.py:157-177): n_epochs full-batch TF-Adam steps on ppo_loss_grad's loss, the batch's old distribution fixed
        while theta moves; the state of get_policy_adam / set_policy_adam, not reset; summed over the ranks by the communicator attached to this
        engine (if any).  Stream-ordered, no synchronisation and no host read between the epochs; returns the n_epochs losses at the thetas
        entering each epoch as a float64 device tensor (None with want_losses=False)."""
        self._close_open_update()
        p = self._ppo_params(clip_lr, entropy_bonus_coeff, lr, beta1, beta2, eps)
        losses = torch.empty(int(n_epochs), dtype=torch.float64, device=self.device) if want_losses else None
        self._chk(lib.metrpo_ppo_update(self._ctx, C.byref(batch), C.byref(p), int(n_epochs), _ptr(losses), self._stream()))
        return losses

    @staticmethod
    def _ppo_kl_params(kl_penalty, step_size):
        p = _lib.PpoKlParams()
        p.kl_penalty, p.step_size = float(kl_penalty), float(step_size)
        return p

    def ppo_kl_loss_grad(self, batch, clip_lr=0.3, entropy_bonus_coeff=0.0, kl_penalty=1.0, step_size=0.01, mean_kl=None):
        """ppo_loss_grad with the KL penalty kl_penalty * max(0, mean_kl - step_size) (algos/ppo.py:120-121): tensor [1 + P] float64.  mean_kl:
        a float64 device tensor holding the GLOBAL mean KL at the ctx policy (loss_kl(batch)[1:2], summed over the ranks); None: computed by the
        call.  The kernels read it on the device and take the gate (mean_kl - step_size > 0, strictly) themselves.  The surrogate and KL parts
        are this rank's share; the entropy term follows ppo_loss_grad's convention."""
        out = torch.empty(self.P + 1, dtype=torch.float64, device=self.device)
        p, kp = self._ppo_params(clip_lr, entropy_bonus_coeff), self._ppo_kl_params(kl_penalty, step_size)
        if mean_kl is not None:
            mean_kl = torch.as_tensor(mean_kl, device=self.device).to(torch.float64).reshape(-1)[:1].contiguous()
        self._chk(lib.metrpo_ppo_kl_loss_grad(self._ctx, C.byref(batch), C.byref(p), C.byref(kp), _ptr(mean_kl), _ptr(out), self._stream()))
        return out

    def ppo_kl_update(self, batch, n_epochs=10, clip_lr=0.3, entropy_bonus_coeff=0.0, kl_penalty=1.0, step_size=0.01, lr=1e-3, beta1=0.9, beta2=0.999,
                      eps=1e-8, want_losses=True, want_mean_kls=False):
        """ppo_update with the KL penalty: each epoch first leaves the global mean KL of the theta entering it on the device (loss_kl's launches,
        summed over the ranks by the communicator attached to this engine), then runs the gradient launch that reads it and the reduction with
        the Adam step.  Stream-ordered, no synchronisation and no host read between the epochs.  -> the n_epochs losses (None with
        want_losses=False); with want_mean_kls=True the pair (losses, mean_kls), mean_kls[e] = the mean KL entering epoch e."""
        self._close_open_update()
        p, kp = self._ppo_params(clip_lr, entropy_bonus_coeff, lr, beta1, beta2, eps), self._ppo_kl_params(kl_penalty, step_size)
        losses = torch.empty(int(n_epochs), dtype=torch.float64, device=self.device) if want_losses else None
        kls = torch.empty(int(n_epochs), dtype=torch.float64, device=self.device) if want_mean_kls else None
        self._chk(lib.metrpo_ppo_kl_update(self._ctx, C.byref(batch), C.byref(p), C.byref(kp), int(n_epochs), _ptr(losses), _ptr(kls), self._stream()))
        return (losses, kls) if want_mean_kls else losses

    def fvp(self, batch, v):
        v = torch.as_tensor(v, device=self.device).to(torch.float64).contiguous()
        hv = torch.empty(self.P, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_fvp(self._ctx, C.byref(batch), _ptr(v), _ptr(hv), self._stream()))
        return hv

    def loss_kl(self, batch, theta=None):
        theta = _f32(theta, self.device, (self.P,)) if theta is not None else None
        out = torch.empty(2, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_loss_kl(self._ctx, C.byref(batch), _ptr(theta), _ptr(out), self._stream()))
        return out

    def trpo_update(self, batch, max_kl=0.01, cg_iters=10, reg_coeff=1e-5, backtrack_ratio=0.8, max_backtracks=15,
                    accept_violation=False, residual_tol=1e-10, allreduce=None, want_vectors=False, explicit_final_hvp=False, spec_trials=0,
                    fvp_batch=None):
        """One ConjugateGradientOptimizer.optimize; `allreduce(tensor_f64)` reduces in place across ranks.  spec_trials = S > 0: only
        enqueue it, with the first S line-search trials decided on the device (no synchronisation; see trpo_update_end).
        fvp_batch (subsample_batch's result, or any Batch): the Fisher-vector products of the CG solve and of the step scale run on it, gradient and
        line search on `batch` (metrpo_trpo_update_fvp / _fvp_begin); None: metrpo_trpo_update / _begin, as before."""
        p = _lib.TrpoParams()
        p.max_kl, p.cg_iters, p.reg_coeff, p.backtrack_ratio = max_kl, cg_iters, reg_coeff, backtrack_ratio
        p.max_backtracks, p.accept_violation, p.residual_tol = max_backtracks, int(accept_violation), residual_tol
        p.explicit_final_hvp = int(bool(explicit_final_hvp))
        if allreduce is not None:
            dev = self.device

            def _cb(user, d_buf, count, stream):
                try:
                    view = torch.as_tensor(_DevView(d_buf, count), device=dev)
                    allreduce(view)
                    return 0
                except Exception:      # never let an exception cross the C ABI
                    import traceback
                    traceback.print_exc()
                    return -1
            cb = _lib.ALLREDUCE_FN(_cb)
            p.allreduce = cb
            self._cb_keepalive = cb
        diag = _lib.TrpoDiag()
        g = d = None
        if want_vectors:
            g = torch.empty(self.P, dtype=torch.float64, device=self.device); d = torch.empty_like(g)
        if spec_trials:
            # first half only (metrpo_trpo_update_begin): no synchronisation; trpo_update_end() returns the diagnostics
            if fvp_batch is not None:
                self._chk(lib.metrpo_trpo_update_fvp_begin(self._ctx, C.byref(batch), C.byref(fvp_batch), C.byref(p), int(spec_trials), _ptr(g), _ptr(d),
                                                           self._stream()))
            else:
                self._chk(lib.metrpo_trpo_update_begin(self._ctx, C.byref(batch), C.byref(p), int(spec_trials), _ptr(g), _ptr(d), self._stream()))
            self._upd_open = (batch, p, g, d, int(spec_trials))              # keeps the batch struct and the output tensors alive until _end
            self._upd_fvp_batch = fvp_batch
            return None
        if fvp_batch is not None:
            self._chk(lib.metrpo_trpo_update_fvp(self._ctx, C.byref(batch), C.byref(fvp_batch), C.byref(p), C.byref(diag), _ptr(g), _ptr(d), self._stream()))
        else:
            self._chk(lib.metrpo_trpo_update(self._ctx, C.byref(batch), C.byref(p), C.byref(diag), _ptr(g), _ptr(d), self._stream()))
        out = dict(loss_before=diag.loss_before, loss=diag.loss, kl=diag.kl, beta=diag.beta,
                   n_backtrack=diag.n_backtrack, accepted=bool(diag.accepted), cg_iters_run=diag.cg_iters_run)
        if want_vectors:
            out['g'], out['d'] = g, d
        return out

    def trpo_update_end(self):
        """Second half of trpo_update(..., spec_trials=S): waits for the update (not for launches enqueued after it) and returns its
        diagnostics; 'late' is True when the policy changed inside this call (accepted at a trial >= S): work enqueued since the first
        half saw the previous policy and must be redone."""
        if getattr(self, '_upd_open', None) is None:
            # already closed -- by get_policy() / set_policy(), which must not see or overwrite a policy whose search is still open
            closed = getattr(self, '_upd_closed', None)
            if closed is None:
                raise RuntimeError('trpo_update_end: no update is open')
            self._upd_closed = None
            return closed
        batch, p, g, d, spec = self._upd_open
        diag = _lib.TrpoDiag()
        late = C.c_int32(0)
        try:
            self._chk(lib.metrpo_trpo_update_end(self._ctx, C.byref(diag), C.byref(late), self._stream()))
        finally:
            self._upd_open = None
            self._upd_fvp_batch = None
        out = dict(loss_before=diag.loss_before, loss=diag.loss, kl=diag.kl, beta=diag.beta,
                   n_backtrack=diag.n_backtrack, accepted=bool(diag.accepted), cg_iters_run=diag.cg_iters_run)
        out['late'] = bool(late.value)
        if g is not None:
            out['g'], out['d'] = g, d
        return out

    def _close_open_update(self):
        """Reading or replacing the policy while an update is only enqueued: close it first (its diagnostics wait for the optimizer's finish())."""
        if getattr(self, '_upd_open', None) is not None:
            self._upd_closed = self.trpo_update_end()


    # ------------------------------------------------------------------ ensemble dynamics training
    def get_dynamics(self):
        out = torch.empty(self.K, self.dyn_param_count, dtype=torch.float32, device=self.device)
        self._chk(lib.metrpo_get_dynamics(self._ctx, _ptr(out), self._stream()))
        return out

    def set_dynamics_model(self, k, params_k):
        p = _f32(params_k, self.device, (self.dyn_param_count,))
        self._chk(lib.metrpo_set_dynamics_model(self._ctx, int(k), _ptr(p), self._stream()))
        self._keep_model = p

    def set_normalizers(self, in_mean, in_std, diff_mean, diff_std):
        dev = self.device
        a = _f32(in_mean, dev, (self.ns + self.na,)); b = _f32(in_std, dev, (self.ns + self.na,))
        c = _f32(diff_mean, dev, (self.ns,)); e = _f32(diff_std, dev, (self.ns,))
        self._chk(lib.metrpo_set_normalizers(self._ctx, _ptr(a), _ptr(b), _ptr(c), _ptr(e), self._stream()))
        torch.cuda.current_stream(dev).synchronize()

    def train_reset(self):
        self._chk(lib.metrpo_dyn_train_reset(self._ctx, self._stream()))

    def get_train_adam(self):
        """-> (m, v [K, dyn_param_count] float32 device tensors, t): the dynamics optimizer's moments in get_dynamics' layout and
        its step count (zeros and 0 before the first train_step)."""
        m = torch.empty(self.K, self.dyn_param_count, dtype=torch.float32, device=self.device)
        v = torch.empty_like(m)
        t = C.c_int64()
        self._chk(lib.metrpo_get_dyn_adam(self._ctx, _ptr(m), _ptr(v), C.byref(t), self._stream()))
        return m, v, int(t.value)

    def set_train_adam(self, m, v, t):
        """Restore get_train_adam's state: the next train_step continues as if never interrupted."""
        shape = (self.K, self.dyn_param_count)
        m = _f32(m, self.device, shape); v = _f32(v, self.device, shape)
        self._chk(lib.metrpo_set_dyn_adam(self._ctx, _ptr(m), _ptr(v), int(t), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()     # inputs may be temporaries

    def train_step(self, x, y, batch_size, lr, reg_constant=0.0, beta1=0.9, beta2=0.999, eps=1e-8, want_loss=True):
        """x [batch_size*K, ns+na], y [batch_size*K, ns] device tensors; returns per-model losses (before the update)."""
        dev = self.device
        x = _f32(x, dev, (batch_size * self.K, self.ns + self.na)); y = _f32(y, dev, (batch_size * self.K, self.ns))
        tp = _lib.TrainParams(lr, beta1, beta2, eps, reg_constant, batch_size)
        loss = torch.empty(self.K, dtype=torch.float64, device=dev) if want_loss else None
        self._chk(lib.metrpo_dyn_train_step(self._ctx, _ptr(x), _ptr(y), C.byref(tp), _ptr(loss), self._stream()))
        self._keep_train = (x, y)
        return loss

    def eval_losses(self, x, y, reg_constant=0.0):
        dev = self.device
        x = _f32(x, dev); y = _f32(y, dev, (x.shape[0], self.ns))
        out = torch.empty(self.K, dtype=torch.float64, device=dev)
        self._chk(lib.metrpo_dyn_eval_losses(self._ctx, _ptr(x), _ptr(y), x.shape[0], float(reg_constant), _ptr(out), self._stream()))
        self._keep_eval = (x, y)
        return out

    def rms_accumulate(self, x, rsum, rsumsq):
        x = _f32(x, self.device)
        self._chk(lib.metrpo_rms_accumulate(self._ctx, _ptr(x), x.shape[0], x.shape[1], _ptr(rsum), _ptr(rsumsq), self._stream()))
        self._keep_rms = x

    def set_det_path(self, use_mfma):
        """test hook: per-model deterministic rollouts (validation cost, BPTT sweeps) on the MFMA kernels (True) or the generic ones."""
        return int(lib.metrpo_set_det_path(self._ctx, 1 if use_mfma else 0))

    # ---- BPTT policy update ('bptt' branch of optimize_policy, model_based_rl.py:1181-1187) ----
    def bptt_grad(self, init_states, T, gamma=1.0):
        """-> (costs [K] float64 device tensor = policy_costs per model, grad [P] float64 device tensor of mean_k cost)."""
        x0 = _f32(init_states, self.device)
        costs = torch.empty(self.K, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.P, dtype=torch.float64, device=self.device)
        self._chk(lib.metrpo_bptt_grad(self._ctx, _ptr(x0), x0.shape[0], int(T), float(gamma), _ptr(costs), _ptr(grad), self._stream()))
        self._keep_bptt = x0
        return costs, grad

    def bptt_grad_stochastic(self, init_states, T, gamma=1.0, noise=None, seed=None, n_saturates=False):
        """'bptt-stochastic' gradient (model_based_rl.py:1188-1196): bptt_grad with u = clip(mean + eps * exp(log_std)), log_std slots
        included.  `noise` [K, T, B, na]: the draws (parity mode); None: Philox draws keyed by `seed` (an int; required then).
        -> (costs, grad), plus n_saturates [B, na] int32 device tensor (model_based_rl.py:129) when asked for."""
        x0 = _f32(init_states, self.device)
        B = x0.shape[0]
        if noise is None:
            if seed is None:
                raise ValueError("bptt_grad_stochastic: give the draws (noise) or a Philox seed")
            eps = None
        else:
            eps = _f32(noise, self.device, (self.K, int(T), B, self.na))
        costs = torch.empty(self.K, dtype=torch.float64, device=self.device)
        grad = torch.empty(self.P, dtype=torch.float64, device=self.device)
        nsat = torch.empty((B, self.na), dtype=torch.int32, device=self.device) if n_saturates else None
        self._chk(lib.metrpo_bptt_grad_stochastic(self._ctx, _ptr(x0), B, int(T), float(gamma), _ptr(eps), int(seed or 0) & 0xFFFFFFFFFFFFFFFF,
                                                  _ptr(costs), _ptr(grad), _ptr(nsat), self._stream()))
        self._keep_bptt = (x0, eps)
        return (costs, grad, nsat) if n_saturates else (costs, grad)

    # ------------------------------------------------------------------ 'l-bfgs' policy update (csrc/lbfgs.hip)
    @staticmethod
    def lbfgs_opts(m=10, maxls=20, maxiter=15000, maxfun=15000, ftol=2.220446049250313e-09, gtol=1e-5, lookahead=2, round_f32=True):
        """metrpo_lbfgs_opts; the defaults are scipy's L-BFGS-B defaults (minimize(method='L-BFGS-B') with no options)."""
        o = _lib.LbfgsOpts()
        o.m, o.maxls, o.maxiter, o.maxfun = int(m), int(maxls), int(maxiter), int(maxfun)
        o.ftol, o.gtol, o.lookahead, o.round_f32 = float(ftol), float(gtol), int(lookahead), int(bool(round_f32))
        return o

    def lbfgs_begin(self, x0, opts=None):
        """Open a reverse-communication L-BFGS-B minimisation at x0 ([n] float64): -> the first point to evaluate ([n] float64 device tensor)."""
        x0 = torch.as_tensor(x0, device=self.device).to(torch.float64).contiguous()
        self._lb_x = torch.empty_like(x0)
        self._lb_task = torch.empty(2, dtype=torch.int32, device=self.device)
        o = opts if opts is not None else self.lbfgs_opts()
        self._chk(lib.metrpo_lbfgs_begin(self._ctx, x0.numel(), _ptr(x0), C.byref(o), _ptr(self._lb_x), self._stream()))
        self._lb_keep = x0
        return self._lb_x

    def lbfgs_iterate(self, f, g):
        """One step on f (1-element float64 device tensor) and g ([n] float64) at the point asked for last: -> (x_next [n], task [2] int32),
        both device tensors (stream-ordered, no synchronisation); task is scipy's (task[0], task[1]), (3, 0) = evaluate x_next."""
        f = torch.as_tensor(f, device=self.device).to(torch.float64).reshape(1).contiguous()
        g = torch.as_tensor(g, device=self.device).to(torch.float64).contiguous()
        self._chk(lib.metrpo_lbfgs_iterate(self._ctx, _ptr(f), _ptr(g), _ptr(self._lb_x), _ptr(self._lb_task), self._stream()))
        self._lb_keep = (f, g)
        return self._lb_x, self._lb_task

    def lbfgs_result(self):
        """The open minimisation's state (metrpo_lbfgs_get_result; synchronises): dict(fun, nit, nfev, status, task)."""
        r = _lib.LbfgsResult()
        self._chk(lib.metrpo_lbfgs_get_result(self._ctx, C.byref(r), self._stream()))
        return dict(fun=r.fun, nit=r.nit, nfev=r.nfev, status=r.status, task=(r.task, r.task_code))

    def lbfgs_policy(self, init_states, T, gamma=1.0, opts=None):
        """The 'l-bfgs' branch's minimize on the BPTT cost of init_states (metrpo_lbfgs_policy): the policy ends at float32 of the last
        accepted iterate.  Synchronises.  -> dict(fun, nit, nfev, status, task=(task[0], task[1]))."""
        self._close_open_update()
        x0 = _f32(init_states, self.device)
        o = opts if opts is not None else self.lbfgs_opts()
        r = _lib.LbfgsResult()
        self._chk(lib.metrpo_lbfgs_policy(self._ctx, _ptr(x0), x0.shape[0], int(T), float(gamma), C.byref(o), C.byref(r), self._stream()))
        return dict(fun=r.fun, nit=r.nit, nfev=r.nfev, status=r.status, task=(r.task, r.task_code))

    def policy_adam_reset(self):
        self._chk(lib.metrpo_policy_adam_reset(self._ctx, self._stream()))

    def get_policy_adam(self):
        """-> (m, v [P] float32 device tensors, t): the BPTT policy optimizer's moments in get_policy's layout and its step count."""
        m = torch.empty(self.P, dtype=torch.float32, device=self.device)
        v = torch.empty_like(m)
        t = C.c_int64()
        self._chk(lib.metrpo_get_policy_adam(self._ctx, _ptr(m), _ptr(v), C.byref(t), self._stream()))
        return m, v, int(t.value)

    def set_policy_adam(self, m, v, t):
        m = _f32(m, self.device, (self.P,)); v = _f32(v, self.device, (self.P,))
        self._chk(lib.metrpo_set_policy_adam(self._ctx, _ptr(m), _ptr(v), int(t), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def policy_adam_step(self, grad, lr, clip_val=None, beta1=0.9, beta2=0.999, eps=1e-8):
        g = grad if isinstance(grad, torch.Tensor) else torch.as_tensor(grad)
        g = g.to(self.device, torch.float64).contiguous()
        self._chk(lib.metrpo_policy_adam_step(self._ctx, _ptr(g), float(lr), float(beta1), float(beta2), float(eps),
                                              float(clip_val) if clip_val else 0.0, self._stream()))
        self._keep_adam = g

    # ------------------------------------------------------------------ 'svg' policy update (csrc/svg.hip; svg_utils.py:12-66)
    def _svg_call(self, obs, act, lengths, model, gamma, path, chunk, jacobians, lr):
        dev = self.device
        obs = _f32(obs, dev); act = _f32(act, dev)
        if obs.dim() != 3 or obs.shape[2] != self.ns:
            raise ValueError("obs: expected [n, T, %d], got %s" % (self.ns, tuple(obs.shape)))
        n, T = int(obs.shape[0]), int(obs.shape[1])
        if tuple(act.shape) != (n, T, self.na):
            raise ValueError("act: expected [%d, %d, %d], got %s" % (n, T, self.na, tuple(act.shape)))
        lengths = _i32(lengths, dev, (n,))
        a = _lib.SvgArgs()
        a.d_obs, a.d_act, a.d_len = obs.data_ptr(), act.data_ptr(), (lengths.data_ptr() if lengths is not None else None)
        a.n, a.T, a.model, a.chunk, a.gamma = n, T, int(model), int(chunk), float(gamma)
        a.path = _lib.SVG_PATHS[path] if isinstance(path, str) else int(path)
        out = dict(theta=torch.empty(self.P, dtype=torch.float64, device=dev), state=torch.empty(self.ns, dtype=torch.float64, device=dev))
        a.d_grad, a.d_state_grad = out['theta'].data_ptr(), out['state'].data_ptr()
        if jacobians:
            out['mean_adj'] = torch.empty(n, T, self.na, dtype=torch.float32, device=dev)
            out['dyn_jac'] = torch.empty(n, T, self.ns, self.ns + self.na, dtype=torch.float32, device=dev)
            out['pol_jac'] = torch.empty(n, T, self.na, self.ns, dtype=torch.float32, device=dev)
            a.d_mean_adj, a.d_dyn_jac, a.d_pol_jac = out['mean_adj'].data_ptr(), out['dyn_jac'].data_ptr(), out['pol_jac'].data_ptr()
        if lr is None:
            self._chk(lib.metrpo_svg_grad(self._ctx, C.byref(a), self._stream()))
        else:
            self._close_open_update()
            self._chk(lib.metrpo_svg_update(self._ctx, C.byref(a), float(lr), self._stream()))
        self._keep_svg = (obs, act, lengths)                                        # alive until the stream has consumed them
        return out

    def svg_grad(self, obs, act, lengths=None, model=0, gamma=1.0, path=0, chunk=0, jacobians=False):
        """metrpo_svg_grad: svg_gradient (svg_utils.py:12-53) on recorded rollouts -- obs [n, T, ns] = s_t, act [n, T, na] = a_t as recorded,
        trajectory-major and padded to T; lengths [n] int (None: all T; rows at or behind a length are never read into a result).  model: the
        dynamics head (the reference: 0).  path: 0 / 'auto', 1 / 'generic', 2 / 'gemm'; chunk: samples per Jacobian chunk (0: the library's choice).
        -> dict(theta [P] float64 = avg_grads['theta'] in get_policy's layout with the log_std slots 0, state [ns] float64 = avg_grads['state']);
        with jacobians also mean_adj [n, T, na] = gamma^t q_t, dyn_jac [n, T, ns, ns+na] = F_t, pol_jac [n, T, na, ns] = Pi_t (float32).
        Device tensors, nothing synchronised."""
        return self._svg_call(obs, act, lengths, model, gamma, path, chunk, jacobians, None)

    def svg_update(self, obs, act, lr, lengths=None, model=0, gamma=1.0, path=0, chunk=0, jacobians=False):
        """metrpo_svg_update: svg_grad, then svg_update's step (svg_utils.py:56-66) theta += float32(-lr) * float32(grad) on the W / b of the ctx
        policy's mean network (log_std untouched).  -> svg_grad's dict (the gradient the step used)."""
        return self._svg_call(obs, act, lengths, model, gamma, path, chunk, jacobians, lr)

    def last_svg_path(self):
        """Jacobian path of the last svg_grad() / svg_update() of this engine: 'generic', 'gemm'; None before the first."""
        return {1: 'generic', 2: 'gemm'}.get(int(lib.metrpo_last_svg_path(self._ctx)))


class _DevView(object):
    """Zero-copy view (float64 unless told otherwise) of library-owned device memory for torch (CUDA array interface)."""

    def __init__(self, ptr, count, typestr='<f8'):
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


def xavier_policy_theta(ns, hidden, na, init_std=1.0, seed=0):
    """[rllab] GaussianMLPPolicy initial parameters: Xavier-uniform W, zero b, log_std = log(init_std)."""
    rng = np.random.RandomState(seed)
    dims = [ns] + list(hidden) + [na]
    parts = []
    for i in range(len(dims) - 1):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        parts += [rng.uniform(-lim, lim, size=dims[i] * dims[i + 1]), np.zeros(dims[i + 1])]
    parts.append(np.full(na, np.log(init_std)))
    return np.concatenate(parts).astype(np.float32)
