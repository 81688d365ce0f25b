"""metrpo_amd -- MI355X-native ME-TRPO policy-optimisation inner loop.

The package directory is `me-trpo_amd/`; import it as `metrpo_amd` (repo-root alias module).
Host code mirrors the reference's operator interface for this one path
(NeuralNetEnv / vec_env_executor / VectorizedSampler / BatchPolopt / NPO / TRPO / VPG / PPO /
ConjugateGradientOptimizer / FirstOrderOptimizer / AdamOptimizer / LinearFeatureBaseline); all arithmetic runs in libmetrpo.so
(hand-written HIP for gfx950) through the C ABI of include/metrpo.h.  No CPU fallback exists.
"""
from . import _lib                      # raises ImportError if libmetrpo.so is missing
from .engine import Engine, Trajectory, xavier_policy_theta
from .parallel import Comm
from .imagined_env import NeuralNetEnv, VecSimpleEnv, InitStatePool, Box, EnvSpec
from .policy import GaussianMLPPolicy
from .baseline import LinearFeatureBaseline
from .sampler import VectorizedSampler, BaseSampler, DevicePaths
from .optimizer import ConjugateGradientOptimizer, AdamOptimizer
from .algos import BatchPolopt, NPO, TRPO, VPG, PPO, FirstOrderOptimizer
from . import early_stop
from . import dynamics_training
from .bptt import BPTT
from .lbfgs import LBFGS
from . import svg
from .svg import SVG, rollout_triplets, pack_rollouts
from . import formats
from . import tf_checkpoint
from .params import from_params, shapes_from_params
from . import model_error
from .model_error import evaluate_model_predictions, get_error_distribution, open_loop_predictions, ensemble_disagreement
from . import planning
from .planning import score_action_sequences, plan_random_shooting, plan_cem, ShootingController
from .planning import engine_grad_scorer, aggregate_heads_grad, refine_actions, plan_cem_gd
from .planning import engine_policy_scorer, score_noise_sequences, plan_cem_policy
from .planning import engine_policy_grad_scorer, refine_noise, plan_cem_policy_gd
from .planning import baseline_terminal_value, ValueMLP, value_targets

__all__ = ['Engine', 'Trajectory', 'xavier_policy_theta', 'Comm', 'NeuralNetEnv', 'VecSimpleEnv', 'InitStatePool',
           'Box', 'EnvSpec', 'GaussianMLPPolicy', 'LinearFeatureBaseline', 'VectorizedSampler', 'BaseSampler',
           'DevicePaths', 'ConjugateGradientOptimizer', 'BatchPolopt', 'NPO', 'TRPO', 'VPG', 'PPO', 'FirstOrderOptimizer', 'AdamOptimizer', 'LBFGS', 'svg', 'SVG', 'rollout_triplets', 'pack_rollouts', 'early_stop', 'dynamics_training', 'from_params', 'shapes_from_params', 'model_error', 'evaluate_model_predictions', 'get_error_distribution', 'open_loop_predictions', 'ensemble_disagreement',
           'planning', 'score_action_sequences', 'plan_random_shooting', 'plan_cem', 'ShootingController',
           'engine_grad_scorer', 'aggregate_heads_grad', 'refine_actions', 'plan_cem_gd',
           'engine_policy_scorer', 'score_noise_sequences', 'plan_cem_policy', 'engine_policy_grad_scorer', 'refine_noise', 'plan_cem_policy_gd',
           'baseline_terminal_value', 'ValueMLP', 'value_targets']
