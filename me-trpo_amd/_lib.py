"""ctypes binding of libmetrpo.so (include/metrpo.h).  There is NO CPU fallback: if the HIP library
is missing or fails to load, importing this module raises."""
import ctypes as C
import os

import torch  # noqa: F401  -- must be imported first so that libmetrpo.so binds to torch's libamdhip64.so.7

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmetrpo.so")
MAX_LAYERS = 6

ENV_IDS = {'swimmer': 0, 'half_cheetah': 1, 'half-cheetah': 1, 'ant': 2, 'humanoid': 3, 'hopper': 4, 'snake': 5}
SAM_MODES = {'step_rand': 0, 'eps_rand': 1, 'model_mean_std': 2, 'model_mean': 3, 'model_med': 4, 'one_model': 5}
DYN_PRECISIONS = {'f32': 0, 'bf16': 1}          # metrpo_dyn_precision
ACTS = {'identity': 0, 'tf.identity': 0, 'relu': 1, 'tf.nn.relu': 1, 'tanh': 2, 'tf.nn.tanh': 2, 'tf.tanh': 2}


class Dims(C.Structure):
    _fields_ = [('env', C.c_int32), ('ns', C.c_int32), ('na', C.c_int32), ('n_models', C.c_int32),
                ('dyn_n_hidden', C.c_int32), ('dyn_hidden', C.c_int32 * MAX_LAYERS), ('dyn_act', C.c_int32 * MAX_LAYERS),
                ('n_drop', C.c_int32), ('pol_n_hidden', C.c_int32), ('pol_hidden', C.c_int32 * MAX_LAYERS)]


class RolloutArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('sam_mode', C.c_int32), ('determ', C.c_int32),
                ('eval_all_heads', C.c_int32), ('d_pool', C.c_void_p), ('n_pool', C.c_int32), ('seed', C.c_uint64),
                ('stream_offset', C.c_uint64), ('d_eps', C.c_void_p), ('d_model_idx', C.c_void_p),
                ('d_sel_noise', C.c_void_p), ('d_reset_idx', C.c_void_p), ('d_reset_model', C.c_void_p),
                ('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_rew', C.c_void_p), ('d_mean', C.c_void_p),
                ('d_done', C.c_void_p), ('d_tpath', C.c_void_p), ('d_last_obs', C.c_void_p),
                # continuation (ABI 2)
                ('t0', C.c_int32), ('d_init_obs', C.c_void_p), ('d_init_ts', C.c_void_p), ('d_init_model', C.c_void_p),
                ('d_last_ts', C.c_void_p), ('d_last_model', C.c_void_p), ('d_stop', C.c_void_p),
                # in-launch stop rule (ABI 4)
                ('stop_batch', C.c_int64), ('d_stop_cum', C.c_void_p)]


class Batch(C.Structure):
    _fields_ = [('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_adv', C.c_void_p), ('d_old_mean', C.c_void_p),
                ('d_old_log_std', C.c_void_p), ('old_log_std_stride', C.c_int32), ('d_valid', C.c_void_p),
                ('N', C.c_int64), ('inv_n_global', C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class TrpoParams(C.Structure):
    _fields_ = [('max_kl', C.c_double), ('cg_iters', C.c_int32), ('reg_coeff', C.c_double),
                ('backtrack_ratio', C.c_double), ('max_backtracks', C.c_int32), ('accept_violation', C.c_int32),
                ('residual_tol', C.c_double), ('allreduce', ALLREDUCE_FN), ('allreduce_user', C.c_void_p),
                ('explicit_final_hvp', C.c_int32)]


class TrainParams(C.Structure):
    _fields_ = [('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double),
                ('reg_constant', C.c_double), ('batch_size', C.c_int32)]


class TrpoDiag(C.Structure):
    _fields_ = [('loss_before', C.c_double), ('loss', C.c_double), ('kl', C.c_double), ('beta', C.c_double),
                ('n_backtrack', C.c_int32), ('accepted', C.c_int32), ('cg_iters_run', C.c_int32)]


class VpgParams(C.Structure):
    _fields_ = [('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double)]


class PpoParams(C.Structure):
    _fields_ = [('clip_lr', C.c_double), ('entropy_bonus_coeff', C.c_double), ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double),
                ('eps', C.c_double)]


class PpoKlParams(C.Structure):
    _fields_ = [('kl_penalty', C.c_double), ('step_size', C.c_double)]


class LbfgsOpts(C.Structure):
    _fields_ = [('m', C.c_int32), ('maxls', C.c_int32), ('maxiter', C.c_int32), ('maxfun', C.c_int32), ('ftol', C.c_double),
                ('gtol', C.c_double), ('lookahead', C.c_int32), ('round_f32', C.c_int32)]


class LbfgsResult(C.Structure):
    _fields_ = [('fun', C.c_double), ('nit', C.c_int32), ('nfev', C.c_int32), ('status', C.c_int32), ('task', C.c_int32),
                ('task_code', C.c_int32), ('pad_', C.c_int32)]


class ModelErrorArgs(C.Structure):
    _fields_ = [('d_Os', C.c_void_p), ('d_As', C.c_void_p), ('d_Rs', C.c_void_p), ('n', C.c_int32), ('T', C.c_int32),
                ('hs', C.POINTER(C.c_int32)), ('n_h', C.c_int32), ('model', C.c_int32), ('known_actions', C.c_int32), ('t0_only', C.c_int32),
                ('signed_diff', C.c_int32), ('d_state_diff', C.c_void_p), ('d_cost_diff', C.c_void_p), ('d_valid', C.c_void_p), ('d_sums', C.c_void_p),
                ('d_dbg_obs', C.c_void_p), ('d_dbg_rew', C.c_void_p), ('d_dbg_done', C.c_void_p), ('d_dbg_last_obs', C.c_void_p)]


class RolloutActionsArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('sam_mode', C.c_int32), ('uniform_model', C.c_int32), ('force_step_loop', C.c_int32),
                ('d_init_obs', C.c_void_p), ('d_actions', C.c_void_p), ('d_model', C.c_void_p), ('d_model_idx', C.c_void_p), ('d_sel_noise', C.c_void_p),
                ('d_obs', C.c_void_p), ('d_rew', C.c_void_p), ('d_done', C.c_void_p)]


class SvgArgs(C.Structure):
    _fields_ = [('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_len', C.c_void_p), ('n', C.c_int32), ('T', C.c_int32), ('model', C.c_int32),
                ('path', C.c_int32), ('chunk', C.c_int32), ('gamma', C.c_double), ('d_grad', C.c_void_p), ('d_state_grad', C.c_void_p),
                ('d_mean_adj', C.c_void_p), ('d_dyn_jac', C.c_void_p), ('d_pol_jac', C.c_void_p)]


class DisagreementArgs(C.Structure):
    _fields_ = [('N', C.c_int64), ('rows_per_group', C.c_int32), ('force_generic', C.c_int32), ('d_obs', C.c_void_p), ('d_actions', C.c_void_p),
                ('d_valid', C.c_void_p), ('d_score', C.c_void_p), ('d_maxdev', C.c_void_p), ('d_std', C.c_void_p), ('d_mean', C.c_void_p),
                ('d_next_all', C.c_void_p), ('d_rew_std', C.c_void_p), ('d_sums', C.c_void_p)]


class ScoreActionsArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('S', C.c_int32), ('stop_at_done', C.c_int32), ('force_generic', C.c_int32), ('gamma', C.c_double),
                ('d_init_obs', C.c_void_p), ('d_actions', C.c_void_p), ('d_ret', C.c_void_p), ('d_len', C.c_void_p), ('d_ret_mean', C.c_void_p),
                ('d_ret_std', C.c_void_p)]


class ScoreActionsGradArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('S', C.c_int32), ('stop_at_done', C.c_int32), ('force_generic', C.c_int32), ('chunk', C.c_int32),
                ('gamma', C.c_double), ('d_init_obs', C.c_void_p), ('d_actions', C.c_void_p), ('d_grad', C.c_void_p), ('d_ret', C.c_void_p),
                ('d_len', C.c_void_p), ('d_grad_mean', C.c_void_p), ('d_lam0', C.c_void_p)]


class ScorePolicyActionsArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('S', C.c_int32), ('stop_at_done', C.c_int32), ('noise_in_std', C.c_int32), ('force_generic', C.c_int32),
                ('gamma', C.c_double), ('d_init_obs', C.c_void_p), ('d_noise', C.c_void_p), ('d_ret', C.c_void_p), ('d_len', C.c_void_p),
                ('d_ret_mean', C.c_void_p), ('d_ret_std', C.c_void_p), ('d_act_out', C.c_void_p)]


class ScorePolicyActionsGradArgs(C.Structure):
    _fields_ = [('B', C.c_int32), ('T', C.c_int32), ('S', C.c_int32), ('stop_at_done', C.c_int32), ('noise_in_std', C.c_int32), ('force_generic', C.c_int32),
                ('chunk', C.c_int32), ('gamma', C.c_double), ('d_init_obs', C.c_void_p), ('d_noise', C.c_void_p), ('d_grad', C.c_void_p),
                ('d_ret', C.c_void_p), ('d_len', C.c_void_p), ('d_grad_mean', C.c_void_p), ('d_lam0', C.c_void_p), ('d_act_out', C.c_void_p)]


class DebugGemmArgs(C.Structure):          # csrc/gemm_debug.h (a diagnostics hook, not part of include/metrpo.h)
    _fields_ = ([(n, C.c_int32) for n in ('op', 'epi', 'ta', 'tb', 'tm', 'tn', 'M', 'N', 'Kd', 'heads', 'lda', 'ldw', 'ldc', 'ldm')] +
                [(n, C.c_int64) for n in ('strideA', 'strideW', 'strideC', 'strideBias', 'strideMask', 'strideAdam', 'stridePart', 'strideW2')] +
                [(n, C.c_void_p) for n in ('A', 'W', 'C', 'bias', 'mask', 'am', 'av', 'bvec', 'bam', 'bav', 'part', 'w2')] +
                [(n, C.c_float) for n in ('lr_t', 'beta1', 'beta2', 'eps', 'decay')] +
                [(n, C.c_int32) for n in ('splits', 'kchunk', 'no', 'act', 'defer')] +
                [(n, C.c_int32) for n in ('o_tm', 'o_tn', 'o_al', 'o_pd', 'o_splits', 'o_kchunk', 'o_gx', 'o_gy', 'o_gz', 'o_reduced')] +
                [('o_stride_part', C.c_int64)])


class DebugGemmBf16Args(C.Structure):      # csrc/rollout_bf16.hip (a diagnostics hook, not part of include/metrpo.h)
    _fields_ = ([(n, C.c_int32) for n in ('op', 'a_bf16', 'c_bf16', 'bn', 'M', 'N', 'Kd', 'Kp', 'heads', 'lda', 'ldc', 'act')] +
                [(n, C.c_int64) for n in ('sA', 'sW', 'sB', 'sC')] +
                [(n, C.c_void_p) for n in ('A', 'W', 'bias', 'C')] +
                [(n, C.c_int32) for n in ('o_bn', 'o_gx', 'o_gy', 'o_gz', 'o_n_cu')])


class DebugEnvModelArgs(C.Structure):      # csrc/probe.hip (a diagnostics hook, not part of include/metrpo.h)
    _fields_ = ([(n, C.c_int32) for n in ('env', 'ns', 'na', 'N', 'compile_time')] +
                [(n, C.c_void_p) for n in ('x', 'u', 'w', 'cost', 'done', 'gx', 'gx_row', 'gu')])


GEMM_BF16_DEBUG_OPS = {'image': 0, 'gemm': 1}
GEMM_EPIS = {'BIAS_ID': 0, 'BIAS_RELU': 1, 'BIAS_TANH': 2, 'RELU_MASK': 3, 'ADAM': 4, 'PLAIN': 5, 'PARTIAL': 6, 'DTANH': 7}     # csrc/gemm_mfma.h
GEMM_DEBUG_OPS = {'auto': 0, 'skinny': 1, 'fused_out': 2}
SVG_PATHS = {'auto': 0, 'generic': 1, 'gemm': 2}          # metrpo_svg_args.path
MODEL_ERROR_MAX_HORIZONS = 32          # include/metrpo.h


# every symbol include/metrpo.h declares: name -> (restype, argtypes)
_P, _I, _L, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
SYMBOLS = {
    'metrpo_abi_version': (_I, []),
    'metrpo_status_string': (C.c_char_p, [_I]),
    'metrpo_create': (_I, [C.POINTER(_P), _I, C.POINTER(Dims)]),
    'metrpo_destroy': (_I, [_P]),
    'metrpo_last_error': (C.c_char_p, [_P]),
    'metrpo_dyn_param_count': (_I, [_P]),
    'metrpo_policy_param_count': (_I, [_P]),
    'metrpo_set_dynamics': (_I, [_P, _P, _P, _P, _P, _P, _P]),
    'metrpo_set_policy': (_I, [_P, _P, _P]),
    'metrpo_get_policy': (_I, [_P, _P, _P]),
    'metrpo_policy_actions': (_I, [_P, _P, _P, _I, _P, _P, _P]),
    'metrpo_step': (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    'metrpo_rollout': (_I, [_P, C.POINTER(RolloutArgs), _P]),
    'metrpo_comm_get_unique_id': (_I, [_P]),
    'metrpo_comm_init': (_I, [_P, _P, _I, _I]),
    'metrpo_comm_destroy': (_I, [_P]),
    'metrpo_allreduce_sum_f64': (_I, [_P, _P, _L, _P]),
    'metrpo_comm_ipc_export': (_I, [_P, _P]),
    'metrpo_comm_ipc_attach': (_I, [_P, _P, _I, _I]),
    'metrpo_comm_ipc_detach': (_I, [_P]),
    'metrpo_comm_set_timeout_ms': (_I, [_P, _L]),
    'metrpo_comm_transport': (_I, [_P]),
    'metrpo_comm_check': (_I, [_P, _P]),
    'metrpo_sampler_progress': (_I, [_P, _P, _P, _I, _I, _I, _L, _P, _P, _P, _P]),
    'metrpo_validation_cost': (_I, [_P, _P, _I, _I, _D, _P, _P]),
    'metrpo_gae': (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _D, _D, _P, _P, _P, _P, _P]),
    'metrpo_process_begin': (_I, [_P, _P, _P, _L, _P]),
    'metrpo_center_advantages': (_I, [_P, _P, _P, _L, _P, _P]),
    'metrpo_baseline_gram': (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _P]),
    'metrpo_baseline_solve': (_I, [_P, _P, _P, _D, _P, _P]),
    'metrpo_loss_grad': (_I, [_P, C.POINTER(Batch), _P, _P]),
    'metrpo_fvp': (_I, [_P, C.POINTER(Batch), _P, _P, _P]),
    'metrpo_loss_kl': (_I, [_P, C.POINTER(Batch), _P, _P, _P]),
    'metrpo_vpg_loss_grad': (_I, [_P, C.POINTER(Batch), _P, _P]),
    'metrpo_vpg_update': (_I, [_P, C.POINTER(Batch), C.POINTER(VpgParams), _P, _P]),
    'metrpo_ppo_loss_grad': (_I, [_P, C.POINTER(Batch), C.POINTER(PpoParams), _P, _P]),
    'metrpo_ppo_update': (_I, [_P, C.POINTER(Batch), C.POINTER(PpoParams), C.c_int32, _P, _P]),
    'metrpo_ppo_kl_loss_grad': (_I, [_P, C.POINTER(Batch), C.POINTER(PpoParams), C.POINTER(PpoKlParams), _P, _P, _P]),
    'metrpo_ppo_kl_update': (_I, [_P, C.POINTER(Batch), C.POINTER(PpoParams), C.POINTER(PpoKlParams), C.c_int32, _P, _P, _P]),
    'metrpo_trpo_update': (_I, [_P, C.POINTER(Batch), C.POINTER(TrpoParams), C.POINTER(TrpoDiag), _P, _P, _P]),
    'metrpo_trpo_update_begin': (_I, [_P, C.POINTER(Batch), C.POINTER(TrpoParams), _I, _P, _P, _P]),
    'metrpo_trpo_update_end': (_I, [_P, C.POINTER(TrpoDiag), C.POINTER(C.c_int32), _P]),
    'metrpo_subsample_batch': (_I, [_P, C.POINTER(Batch), _P, _L, _D, C.POINTER(Batch), _P, _P]),
    'metrpo_trpo_update_fvp': (_I, [_P, C.POINTER(Batch), C.POINTER(Batch), C.POINTER(TrpoParams), C.POINTER(TrpoDiag), _P, _P, _P]),
    'metrpo_trpo_update_fvp_begin': (_I, [_P, C.POINTER(Batch), C.POINTER(Batch), C.POINTER(TrpoParams), _I, _P, _P, _P]),
    'metrpo_model_error_windows': (_I, [_P, _P, _I, _I, _P, _P]),
    'metrpo_model_error': (_I, [_P, C.POINTER(ModelErrorArgs), _P]),
    'metrpo_rollout_actions': (_I, [_P, C.POINTER(RolloutActionsArgs), _P]),
    'metrpo_last_rollout_actions_kernel': (_I, [_P]),
    'metrpo_svg_grad': (_I, [_P, C.POINTER(SvgArgs), _P]),
    'metrpo_svg_update': (_I, [_P, C.POINTER(SvgArgs), _D, _P]),
    'metrpo_last_svg_path': (_I, [_P]),
    'metrpo_ensemble_disagreement': (_I, [_P, C.POINTER(DisagreementArgs), _P]),
    'metrpo_last_disagreement_kernel': (_I, [_P]),
    'metrpo_score_actions': (_I, [_P, C.POINTER(ScoreActionsArgs), _P]),
    'metrpo_last_score_actions_kernel': (_I, [_P]),
    'metrpo_score_actions_grad': (_I, [_P, C.POINTER(ScoreActionsGradArgs), _P]),
    'metrpo_last_score_actions_grad_kernel': (_I, [_P]),
    'metrpo_score_policy_actions': (_I, [_P, C.POINTER(ScorePolicyActionsArgs), _P]),
    'metrpo_last_score_policy_actions_kernel': (_I, [_P]),
    'metrpo_score_policy_actions_grad': (_I, [_P, C.POINTER(ScorePolicyActionsGradArgs), _P]),
    'metrpo_last_score_policy_actions_grad_kernel': (_I, [_P]),
    'metrpo_set_terminal_value': (_I, [_P, _P, _P, _P, _I, _P]),
    'metrpo_clear_terminal_value': (_I, [_P]),
    'metrpo_has_terminal_value': (_I, [_P]),
    'metrpo_set_terminal_value_mlp': (_I, [_P, _P, _I, _I, _P, _I, _P]),
    'metrpo_terminal_value_kind': (_I, [_P]),
    'metrpo_dyn_train_reset': (_I, [_P, _P]),
    'metrpo_dyn_train_step': (_I, [_P, _P, _P, C.POINTER(TrainParams), _P, _P]),
    'metrpo_dyn_eval_losses': (_I, [_P, _P, _P, _L, _D, _P, _P]),
    'metrpo_get_dynamics': (_I, [_P, _P, _P]),
    'metrpo_set_dynamics_model': (_I, [_P, _I, _P, _P]),
    'metrpo_set_normalizers': (_I, [_P, _P, _P, _P, _P, _P]),
    'metrpo_rms_accumulate': (_I, [_P, _P, _L, _I, _P, _P, _P]),
    'metrpo_bptt_grad': (_I, [_P, _P, _I, _I, _D, _P, _P, _P]),
    'metrpo_bptt_grad_stochastic': (_I, [_P, _P, _I, _I, _D, _P, C.c_uint64, _P, _P, _P, _P]),
    'metrpo_set_exclusive': (_I, [_P, _I]),
    'metrpo_set_option': (_I, [_P, C.c_char_p, C.c_char_p]),
    'metrpo_get_option': (_I, [_P, C.c_char_p, C.c_char_p, _I]),
    'metrpo_option_name': (C.c_char_p, [_I]),
    'metrpo_last_rollout_kernel': (_I, [_P]),
    'metrpo_rollout_note': (C.c_char_p, [_P]),
    'metrpo_debug_last_rollout_launch': (_I, [_P, _P]),
    'metrpo_set_dyn_precision': (_I, [_P, _I]),
    'metrpo_get_dyn_precision': (_I, [_P]),
    'metrpo_policy_adam_reset': (_I, [_P, _P]),
    'metrpo_policy_adam_step': (_I, [_P, _P, _D, _D, _D, _D, _D, _P]),
    'metrpo_lbfgs_begin': (_I, [_P, _I, _P, C.POINTER(LbfgsOpts), _P, _P]),
    'metrpo_lbfgs_iterate': (_I, [_P, _P, _P, _P, _P, _P]),
    'metrpo_lbfgs_get_result': (_I, [_P, C.POINTER(LbfgsResult), _P]),
    'metrpo_lbfgs_policy': (_I, [_P, _P, _I, _I, _D, C.POINTER(LbfgsOpts), C.POINTER(LbfgsResult), _P]),
    'metrpo_get_dyn_adam': (_I, [_P, _P, _P, C.POINTER(_L), _P]),
    'metrpo_set_dyn_adam': (_I, [_P, _P, _P, _L, _P]),
    'metrpo_get_policy_adam': (_I, [_P, _P, _P, C.POINTER(_L), _P]),
    'metrpo_set_policy_adam': (_I, [_P, _P, _P, _L, _P]),
}
# diagnostics hooks exported besides the header's ABI (used by tests to cross-check the two rollout kernels)
EXTRA_SYMBOLS = {
    'metrpo_rollout_generic': (_I, [_P, C.POINTER(RolloutArgs), _P]),
    'metrpo_has_mfma_path': (_I, [_P]),
    'metrpo_set_update_path': (_I, [_P, _I]),
    'metrpo_update_path': (_I, [_P, _L]),
    'metrpo_set_rollout_variant': (_I, [_P, _I]),
    'metrpo_set_det_path': (_I, [_P, _I]),
    'metrpo_probe_peaks': (_I, [_P, _P, _P]),
    'metrpo_schedulable_cus': (_I, [_P, _P]),
    'metrpo_debug_fvp_us': (_I, [_P, _P, _P]),
    'metrpo_debug_last_update': (_I, [_P, _P]),
    'metrpo_debug_last_solve': (_I, [_P, _P]),
    'metrpo_debug_persist_stats': (_I, [_P, _P, _I, _P]),
    'metrpo_debug_ws_retired': (_I, [_P, _P, _I]),
    'metrpo_debug_coop_waves': (_I, [_P]),
    'metrpo_set_coop_split': (_I, [_P, _I]),
    'metrpo_debug_score_policy_chunk': (_I, [_P, _I]),
    'metrpo_debug_gemm': (_I, [_P, C.POINTER(DebugGemmArgs), _P]),
    'metrpo_debug_gemm_bf16': (_I, [_P, C.POINTER(DebugGemmBf16Args), _P]),
    'metrpo_debug_last_bf16_layers': (_I, [_P, _P]),
    'metrpo_debug_env_model': (_I, [_P, C.POINTER(DebugEnvModelArgs), _P]),
}


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmetrpo.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for table in (SYMBOLS, EXTRA_SYMBOLS):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
    if lib.metrpo_abi_version() != 4:
        raise ImportError("libmetrpo.so ABI version mismatch")
    return lib


lib = load()


class MetrpoError(RuntimeError):
    pass


def check(rc, ctx=None):
    if rc != 0:
        msg = lib.metrpo_status_string(rc).decode()
        if ctx:
            msg += ": " + lib.metrpo_last_error(ctx).decode()
        raise MetrpoError(msg)
