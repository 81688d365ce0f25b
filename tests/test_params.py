"""metrpo_amd.shapes_from_params: the reference's own run configurations (params/params-*.json; key sets committed as tests/golden/params_<env>.json by
tests/golden/make_params_fixtures.py) mapped to the shapes of DESIGN.md section 4 -- no GPU, no library call."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def load_params_module():
    # the package __init__ needs libmetrpo.so (built by __graft_entry__.build()); params.py itself is plain Python
    import metrpo_amd
    return metrpo_amd


# DESIGN.md section 4, "Which kernels the reference's own params files reach": every six-env file is K = 5, B = 100 (the sampler's clamp), 50 000 samples
EXPECT = {
    'swimmer':      dict(env='swimmer', dyn_hidden=(512, 512), pol_hidden=(32, 32), n_drop=2, T=200, rounds=3, ns=10, na=2),
    'half_cheetah': dict(env='half_cheetah', dyn_hidden=(1024, 1024), pol_hidden=(32, 32), n_drop=1, T=100, rounds=5, ns=18, na=6),
    'hopper':       dict(env='hopper', dyn_hidden=(1024, 1024), pol_hidden=(32, 32), n_drop=0, T=100, rounds=5, ns=11, na=3),
    'snake':        dict(env='snake', dyn_hidden=(1024, 1024), pol_hidden=(32, 32), n_drop=2, T=200, rounds=3, ns=14, na=4),
    'ant':          dict(env='ant', dyn_hidden=(1024, 1024), pol_hidden=(32, 32), n_drop=2, T=100, rounds=5, ns=29, na=8),
    'humanoid':     dict(env='humanoid', dyn_hidden=(1024, 1024), pol_hidden=(100, 50, 25), n_drop=0, T=100, rounds=5, ns=55, na=21),
}


@pytest.mark.parametrize('name', sorted(EXPECT))
def test_shapes_of_the_six_env_params_files(name):
    m = load_params_module()
    sh = m.shapes_from_params(os.path.join(GOLD, 'params_%s.json' % name))
    for k, v in EXPECT[name].items():
        assert sh[k] == v, (k, sh[k], v)
    assert sh['K'] == 5 and sh['n_envs'] == 100 and sh['batch_size'] == 50000 and sh['sam_mode'] == 'step_rand' and sh['algo'] == 'trpo'
    assert sh['nin'] == sh['ns'] + sh['na'] - sh['n_drop'] and sh['dyn_act'] == ['relu', 'relu']
    assert sh['trpo'] == dict(step_size=0.01, discount=1.0, init_std=1.0, reset=True)
    op = sh['optimize_policy']
    assert (op['mode'], op['whole'], op['log_every'], op['num_iters_threshold'], op['gamma']) == ('estimated', True, 5, 25, 1.0) and op['T'] == sh['T']
    assert sh['stop_critereon']['threshold'] == 0.10 and sh['stop_critereon']['offset'] == 1e-5 and 0 < sh['stop_critereon']['percent_models_threshold'] <= 0.5
    assert sh['dynamics_opt']['batch_size'] == 1000 and sh['dynamics_opt']['sample_mode'] in ('random', 'next_batch')
    assert set(sh['dynamics_opt']['learning_rate']) == {'scratch', 'refine'}


def test_bench_configs_of_the_params_files_are_the_files_shapes():
    """bench.py --config C0p / C0hc / C0ho / C0sn / C0an / C0hu (synthetic.CONFIGS) must be what the reference's files say."""
    m = load_params_module()
    from metrpo_amd import synthetic
    for cfg, name in (('C0p', 'swimmer'), ('C0hc', 'half_cheetah'), ('C0ho', 'hopper'), ('C0sn', 'snake'), ('C0an', 'ant'), ('C0hu', 'humanoid')):
        sh = m.shapes_from_params(os.path.join(GOLD, 'params_%s.json' % name))
        c = synthetic.CONFIGS[cfg]
        assert (c['env'], c['K'], tuple(c['dyn_hidden']), tuple(c['pol_hidden']), c['B'], c['H'], c['batch_size']) == \
               (sh['env'], sh['K'], sh['dyn_hidden'], sh['pol_hidden'], sh['n_envs'], sh['T'], sh['batch_size']), cfg
        assert synthetic.ENV_SPECS[c['env']] == (sh['ns'], sh['na'], sh['n_drop'])
        assert synthetic.config_from_params(os.path.join(GOLD, 'params_%s.json' % name)) == dict(c, gpus=1)


def test_per_layer_nonlinearity_reaches_the_engine_arguments():
    """dynamics_model.nonlinearity is a list with one activation per hidden layer (training.py:156-208): tanh (both spellings) and identity are mapped
    onto Engine(dyn_act=[...]) in layer order; an unknown name is refused by name."""
    m = load_params_module()
    p = json.load(open(os.path.join(GOLD, 'params_swimmer.json')))
    p['dynamics_model']['nonlinearity'] = ['tf.nn.tanh', 'tf.identity']
    assert m.shapes_from_params(p)['dyn_act'] == ['tanh', 'identity']
    p['dynamics_model']['nonlinearity'] = ['tf.identity', 'tf.tanh']
    assert m.shapes_from_params(p)['dyn_act'] == ['identity', 'tanh']
    p['dynamics_model']['nonlinearity'] = ['tf.nn.relu', 'tf.nn.tanh']
    assert m.shapes_from_params(p)['dyn_act'] == ['relu', 'tanh']
    p['dynamics_model']['nonlinearity'] = ['tf.nn.tanh', 'tf.nn.elu']
    with pytest.raises(ValueError, match='nonlinearity'):
        m.shapes_from_params(p)


def test_from_params_hands_the_activations_to_the_engine(monkeypatch):
    """from_params builds Engine(..., dyn_act=[one name per hidden layer]): the constructor's arguments, caught in front of the device."""
    import importlib
    import sys
    m = load_params_module()
    pkg = sys.modules[m.from_params.__module__].__package__
    seen = {}

    class Caught(Exception):
        pass

    def fake_engine(*args, **kw):
        seen.update(args=args, kw=kw)
        raise Caught()
    monkeypatch.setattr(importlib.import_module(pkg + '.engine'), 'Engine', fake_engine)
    p = json.load(open(os.path.join(GOLD, 'params_swimmer.json')))
    p['dynamics_model']['nonlinearity'] = ['tf.nn.tanh', 'tf.identity']
    with pytest.raises(Caught):
        m.from_params(p)
    assert seen['kw']['dyn_act'] == ['tanh', 'identity'] and tuple(seen['args'][2]) == (512, 512)


def test_variants_without_a_kernel_are_named():
    m = load_params_module()
    for name in ('point_mass', 'point2D'):                      # envs without an analytic reward on this path
        with pytest.raises(ValueError, match='env'):
            m.shapes_from_params(os.path.join(GOLD, 'params_%s.json' % name))
    p = json.load(open(os.path.join(GOLD, 'params_swimmer.json')))
    p['dynamics_model']['use_logit_weights'] = True
    with pytest.raises(ValueError, match='use_logit_weights'):
        m.shapes_from_params(p)
    p['dynamics_model']['use_logit_weights'] = False
    p['dynamics_model']['prediction_type'] = 'second_derivative'
    with pytest.raises(ValueError, match='prediction_type'):
        m.shapes_from_params(p)
    p['dynamics_model']['prediction_type'] = 'state_change'
    p['dynamics_model']['nonlinearity'] = ['tf.nn.relu']
    with pytest.raises(ValueError, match='nonlinearity'):
        m.shapes_from_params(p)
