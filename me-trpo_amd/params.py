"""The reference's run configuration (`params/params-*.json`, read by main.py:40-60 and unpacked in training.py:100-130 / :330-372) mapped onto
this package: `from_params(path_or_dict)` builds the Engine, policy, baseline, imagined env and TRPO (or VPG) object the way training.py:297-372 and
model_based_rl.py:373-380 wire them, and returns the keyword arguments of `early_stop.optimize_policy` (policy_opt_params.{T, gamma, mode, whole,
log_every, num_iters_threshold, max_iters, stop_critereon}) and of `dynamics_training` (dynamics_opt_params).  `shapes_from_params` is the GPU-free
half: it only reads the keys and says which shapes the run has -- what tests/test_params.py checks against DESIGN.md section 4 for the six env files.

Keys read (params-swimmer.json:5-86):
    env, algo, n_models
    dynamics_model.{hidden_layers, nonlinearity, ignore_xy_input | ignore_x_input, prediction_type, use_logit_weights, regularization.constant,
                    rollout_precision (EXTENSION, see below)}
    policy.hidden_layers
    policy_opt_params.{T, gamma, mode, whole, log_every, num_iters_threshold, max_iters, batch_size, sam_mode, learning_rate, grad_norm_clipping,
                       stop_critereon.{threshold, offset, percent_models_threshold}, trpo.{init_std, step_size, discount, batch_size, reset,
                                                                                             subsample_factor (EXTENSION, see below)},
                       vpg.{init_std, discount, batch_size, reset},
                       ppo.{init_std, discount, batch_size, reset, clip_lr, n_epochs, learning_rate, entropy_bonus_coeff,
                            use_kl_penalty, initial_kl_penalty, step_size}}
    dynamics_opt_params.{learning_rate.{scratch, refine}, batch_size, max_passes, log_every, num_passes_threshold, sample_mode, reinitialize,
                         stop_critereon.{threshold, offset}}
'algo' builds 'trpo', 'vpg' (training.py:337-352: VPG with the vpg block's batch size, discount and log_std reset), 'bptt' and 'bptt-stochastic';
svg and l-bfgs raise.  trpo.subsample_factor is an EXTENSION key (default 1.0: the reference's run; below 1 the Fisher-vector products of the update
see that fraction of the batch, [rllab] ConjugateGradientOptimizer(subsample_factor)); it is reported as shapes['trpo_ext'].  dynamics_model.rollout_precision is an EXTENSION key too ('f32' default: the reference's arithmetic; 'bf16': the
imagined rollouts that feed the TRPO / VPG / PPO update run their dynamics layers on bf16 operands, Engine.set_dyn_precision; training, validation and
early stopping stay f32); it is reported as shapes['dyn_ext'] and applied by from_params once the engine exists.  'ppo' (algos/ppo.py) is an EXTENSION: the reference's training.py has no such branch and its params files no ppo block; the
block's defaults are ppo.py's (clip_lr 0.3, entropy_bonus_coeff 0, use_kl_penalty false, initial_kl_penalty 1, step_size 0.01), AdamOptimizer's (n_epochs 10, learning_rate 1e-3) and the vpg block's.  Everything else in the files (rollout_params, sweep_iters, sample_size, *_path) steers the reference's real-simulator data collection and outer
sweeps, which are out of scope here; those keys are passed through untouched in `Setup.params`."""
import json

ENV_NAMES = {'swimmer': 'swimmer', 'half-cheetah': 'half_cheetah', 'half_cheetah': 'half_cheetah', 'ant': 'ant', 'humanoid': 'humanoid',
             'hopper': 'hopper', 'snake': 'snake'}
# (ns, na) of the six envs with an analytic reward (envs/com_*_env.py); the input columns dropped come from the params file
ENV_DIMS = {'swimmer': (10, 2), 'half_cheetah': (18, 6), 'ant': (29, 8), 'humanoid': (55, 21), 'hopper': (11, 3), 'snake': (14, 4)}
_ACTS = {'tf.nn.relu': 'relu', 'tf.nn.tanh': 'tanh', 'tf.tanh': 'tanh', 'tf.identity': 'identity'}


def _load(path_or_dict):
    if isinstance(path_or_dict, dict):
        return path_or_dict
    with open(path_or_dict) as f:
        return json.load(f)


def shapes_from_params(path_or_dict):
    """Shapes and scalar settings of a run, from the reference's keys alone (no GPU, no library call).  Raises ValueError with the key's name for
    a variant this path does not build -- the same settings Engine() rejects."""
    p = _load(path_or_dict)
    env_key = p['env']
    if env_key not in ENV_NAMES:
        raise ValueError("params 'env' = %r: this path has the analytic rewards of %s (env_helpers.py / envs/com_*_env.py); point-mass and point2D are "
                         "out of scope" % (env_key, sorted(set(ENV_NAMES.values()))))
    env = ENV_NAMES[env_key]
    ns, na = ENV_DIMS[env]
    dm, pol, po = p['dynamics_model'], p['policy'], p['policy_opt_params']
    if dm.get('use_logit_weights'):
        raise ValueError("dynamics_model.use_logit_weights (training.py:234-242) is not built")
    if dm.get('prediction_type', 'state_change') != 'state_change':
        raise ValueError("dynamics_model.prediction_type = %r: only 'state_change' (training.py:257) is built" % dm.get('prediction_type'))
    acts = [_ACTS.get(a) for a in dm.get('nonlinearity', ['tf.nn.relu'] * len(dm['hidden_layers']))]
    if None in acts or len(acts) != len(dm['hidden_layers']):                    # training.py:156 asserts the lengths agree
        raise ValueError("dynamics_model.nonlinearity = %r: one of %s per hidden layer" % (dm.get('nonlinearity'), sorted(_ACTS)))
    n_drop = 2 if dm.get('ignore_xy_input') else (1 if dm.get('ignore_x_input') else 0)      # training.py:146-154
    rollout_precision = dm.get('rollout_precision', 'f32')
    if rollout_precision not in ('f32', 'bf16'):
        raise ValueError("dynamics_model.rollout_precision = %r: 'f32' or 'bf16'" % (rollout_precision,))
    trpo, vpg, ppo = po.get('trpo', {}), po.get('vpg', {}), po.get('ppo', {})
    algo = p.get('algo', 'trpo')
    T = int(po['T'])
    # the sampler's batch comes from the block of the algorithm that runs (training.py:345 for vpg, :360 for trpo)
    batch_size = int((vpg if algo == 'vpg' else ppo if algo == 'ppo' else trpo).get('batch_size', 5000))
    n_envs = max(1, min(int(batch_size / T), 100))                                # vectorized_sampler.py:24-27
    sc = po.get('stop_critereon', {})
    dop = p.get('dynamics_opt_params', {})
    lr = dop.get('learning_rate', {'scratch': 1e-3, 'refine': 1e-3})
    lr = dict(lr) if isinstance(lr, dict) else {'scratch': float(lr), 'refine': float(lr)}
    return dict(
        env=env, algo=algo, K=int(p['n_models']), ns=ns, na=na, n_drop=n_drop, nin=ns + na - n_drop,
        dyn_hidden=tuple(int(h) for h in dm['hidden_layers']), dyn_act=acts, pol_hidden=tuple(int(h) for h in pol['hidden_layers']),
        dyn_reg_constant=float(dm.get('regularization', {}).get('constant', 0.0)),
        T=T, n_envs=n_envs, batch_size=batch_size, rounds=max(1, -(-batch_size // (n_envs * T))),
        sam_mode=po.get('sam_mode', 'step_rand'),
        trpo=dict(step_size=float(trpo.get('step_size', 0.01)), discount=float(trpo.get('discount', 1.0)), init_std=float(trpo.get('init_std', 1.0)),
                  reset=bool(trpo.get('reset', True))),
        vpg=dict(discount=float(vpg.get('discount', 1.0)), init_std=float(vpg.get('init_std', 1.0)), batch_size=int(vpg.get('batch_size', 5000)),
                 reset=bool(vpg.get('reset', True))),
        ppo=dict(discount=float(ppo.get('discount', 1.0)), init_std=float(ppo.get('init_std', 1.0)), batch_size=int(ppo.get('batch_size', 5000)),
                 reset=bool(ppo.get('reset', True)), clip_lr=float(ppo.get('clip_lr', 0.3)), n_epochs=int(ppo.get('n_epochs', 10)),
                 learning_rate=float(ppo.get('learning_rate', 1e-3)), entropy_bonus_coeff=float(ppo.get('entropy_bonus_coeff', 0.0))),
        # EXTENSION key of the trpo block (no reference params file has it): [rllab] ConjugateGradientOptimizer(subsample_factor), the fraction of the batch
        # the Fisher-vector products see; 1.0 = the reference's run (algos/trpo.py:18-20 passes no optimizer_args).  Kept apart from the reference's keys above.
        trpo_ext=dict(subsample_factor=float(trpo.get('subsample_factor', 1.0))),
        # EXTENSION key of the dynamics_model block (no reference params file has it): operand precision of the dynamics forward inside the imagined rollouts
        # (Engine.set_dyn_precision); 'f32' = the reference's arithmetic.  Kept apart from the reference's keys above.
        dyn_ext=dict(rollout_precision=rollout_precision),
        # the KL penalty's keys of the same params block (ppo.py:27-28, :34), kept apart from the dict above
        ppo_kl=dict(use_kl_penalty=bool(ppo.get('use_kl_penalty', False)), initial_kl_penalty=float(ppo.get('initial_kl_penalty', 1.0)),
                    step_size=float(ppo.get('step_size', 0.01))),
        optimize_policy=dict(T=T, gamma=float(po.get('gamma', 1.0)), mode=po.get('mode', 'estimated'), whole=bool(po.get('whole', True)),
                             log_every=int(po.get('log_every', 5)), num_iters_threshold=int(po.get('num_iters_threshold', 25)),
                             max_iters=int(po.get('max_iters', 400))),
        stop_critereon=dict(threshold=float(sc.get('threshold', 0.10)), offset=float(sc.get('offset', 1e-5)),
                            percent_models_threshold=float(sc.get('percent_models_threshold', 0.5))),
        bptt=dict(batch_size=int(po.get('batch_size', 500)), learning_rate=float(po.get('learning_rate', 1e-3)),
                  grad_norm_clipping=po.get('grad_norm_clipping')),
        dynamics_opt=dict(learning_rate=lr,
                          batch_size=int(dop.get('batch_size', 1000)), max_passes=int(dop.get('max_passes', 2000)), log_every=int(dop.get('log_every', 5)),
                          num_passes_threshold=int(dop.get('num_passes_threshold', 25)), sample_mode=dop.get('sample_mode', 'random'),
                          reg_constant=float(dm.get('regularization', {}).get('constant', 0.0))),
        dynamics_reinitialize_every=dop.get('reinitialize', 5),     # model_based_rl.py: re-initialise the ensemble every n-th sweep (outer loop: caller's)
    )


class Setup(object):
    """What `from_params` hands back: the objects of the inner loop plus the keyword sets of the two loop drivers.
        s = metrpo_amd.from_params('params/params-swimmer.json', init_states=real_env_reset_states)
        s.engine.set_dynamics_layers(...)                       # or train them: dynamics_training.optimize_models(s.engine, ..., **s.dynamics_opt)
        out = metrpo_amd.early_stop.optimize_policy(s.algo, validation_init, **s.optimize_policy_kwargs)
    'bptt' / 'bptt-stochastic' runs also carry `bptt` (a BPTT object; stochastic for the latter) and the keywords of the BPTT branch:
        out = metrpo_amd.early_stop.optimize_policy(s.bptt, validation_init, **s.bptt_optimize_policy_kwargs)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def from_params(path_or_dict, device=0, init_states=None, comm=None, seed=0, n_envs=None):
    """Engine + GaussianMLPPolicy + LinearFeatureBaseline + NeuralNetEnv + TRPO for one of the reference's params files (training.py:297-372,
    model_based_rl.py:373-380).  `init_states` [n, ns]: reset states of the imagined env (the reference resets it with the real simulator,
    env_helpers.py:552-555); default: the synthetic pool of `synthetic.make_pool`.  `n_envs` lifts the sampler's 100-env clamp."""
    from . import synthetic, early_stop
    from .engine import Engine
    from .policy import GaussianMLPPolicy
    from .baseline import LinearFeatureBaseline
    from .imagined_env import NeuralNetEnv, InitStatePool
    from .algos import TRPO, VPG, PPO
    from .optimizer import AdamOptimizer
    from .bptt import BPTT
    p = _load(path_or_dict)
    sh = shapes_from_params(p)
    if sh['algo'] not in ('trpo', 'vpg', 'ppo', 'bptt', 'bptt-stochastic'):
        raise ValueError("params 'algo' = %r: this path builds 'trpo', 'vpg', 'ppo' (and the 'bptt' / 'bptt-stochastic' updates of section 8f); svg / l-bfgs "
                         "are not built from a params file (the 'l-bfgs' update runs as metrpo_amd.LBFGS, the 'svg' update as metrpo_amd.SVG on recorded rollouts)"
                         % sh['algo'])
    blk = sh['vpg'] if sh['algo'] == 'vpg' else sh['ppo'] if sh['algo'] == 'ppo' else sh['trpo']     # init_std / reset of the rllab algorithm that runs (training.py:350-352, 368-370)
    eng = Engine(sh['env'], sh['K'], sh['dyn_hidden'], sh['pol_hidden'], n_drop=sh['n_drop'], dyn_act=sh['dyn_act'], device=device)
    if sh['dyn_ext']['rollout_precision'] != 'f32':
        eng.set_dyn_precision(sh['dyn_ext']['rollout_precision'])      # a shape outside the GEMM rollout families raises the library's message
    policy = GaussianMLPPolicy(eng, init_std=blk['init_std'], seed=seed)
    baseline = LinearFeatureBaseline()
    pool = InitStatePool(synthetic.make_pool(sh['env']) if init_states is None else init_states, sh['na'])
    env = NeuralNetEnv(env=pool, inner_env=None, cost_np=sh['env'], dynamics_in=None, dynamics_outs=eng, sam_mode=sh['sam_mode'])
    sargs = dict(n_envs=n_envs) if n_envs else None
    if sh['algo'] == 'vpg':
        algo = VPG(env=env, policy=policy, baseline=baseline, batch_size=sh['batch_size'], max_path_length=sh['T'], discount=sh['vpg']['discount'],
                   sampler_args=sargs, comm=comm, seed=seed)
    elif sh['algo'] == 'ppo':
        algo = PPO(env=env, policy=policy, baseline=baseline, batch_size=sh['batch_size'], max_path_length=sh['T'], discount=blk['discount'],
                   clip_lr=blk['clip_lr'], entropy_bonus_coeff=blk['entropy_bonus_coeff'], use_kl_penalty=sh['ppo_kl']['use_kl_penalty'],
                   initial_kl_penalty=sh['ppo_kl']['initial_kl_penalty'], step_size=sh['ppo_kl']['step_size'],
                   optimizer=AdamOptimizer(learning_rate=blk['learning_rate'], n_epochs=blk['n_epochs']), sampler_args=sargs, comm=comm, seed=seed)
    else:
        algo = TRPO(env=env, policy=policy, baseline=baseline, batch_size=sh['batch_size'], max_path_length=sh['T'], discount=sh['trpo']['discount'],
                    step_size=sh['trpo']['step_size'], sampler_args=sargs, comm=comm, seed=seed,
                    optimizer_args=dict(subsample_factor=sh['trpo_ext']['subsample_factor'], seed=seed))
    stop_fn = early_stop.stop_critereon(sh['stop_critereon']['threshold'], sh['stop_critereon']['offset'], sh['stop_critereon']['percent_models_threshold'])
    okw = dict(sh['optimize_policy'], stop_fn=stop_fn, reset_log_std=blk['reset'])
    bptt, bkw = None, None
    if sh['algo'] in ('bptt', 'bptt-stochastic'):
        bptt = BPTT(eng, sh['T'], gamma=sh['optimize_policy']['gamma'], learning_rate=sh['bptt']['learning_rate'],
                    grad_norm_clipping=sh['bptt']['grad_norm_clipping'], batch_size=sh['bptt']['batch_size'],
                    stochastic=(sh['algo'] == 'bptt-stochastic'), seed=seed)
        # no reset_opt for these branches: the reference builds it for trpo / vpg only (training.py:350-352, 368-370)
        bkw = dict(sh['optimize_policy'], stop_fn=stop_fn, init_pool=pool)
    return Setup(params=p, shapes=sh, engine=eng, policy=policy, baseline=baseline, env=env, algo=algo, bptt=bptt, optimize_policy_kwargs=okw,
                 bptt_optimize_policy_kwargs=bkw, dynamics_opt=sh['dynamics_opt'])
