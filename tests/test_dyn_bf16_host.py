"""The EXTENSION key dynamics_model.rollout_precision of a params file (metrpo_amd.params; no reference file has it): parsed into shapes['dyn_ext'],
'f32' by default, a bad value named, and the reference's own six files (tests/golden/params_<env>.json) mapped exactly as before -- no GPU."""
import copy
import json
import os

import pytest

from test_params import EXPECT, GOLD


def _params(name='swimmer'):
    return json.load(open(os.path.join(GOLD, 'params_%s.json' % name)))


def test_rollout_precision_is_parsed_and_defaults_to_f32():
    import metrpo_amd
    p = _params()
    assert 'rollout_precision' not in p['dynamics_model']
    assert metrpo_amd.shapes_from_params(p)['dyn_ext'] == dict(rollout_precision='f32')
    for v in ('f32', 'bf16'):
        q = copy.deepcopy(p); q['dynamics_model']['rollout_precision'] = v
        assert metrpo_amd.shapes_from_params(q)['dyn_ext'] == dict(rollout_precision=v)


def test_a_bad_rollout_precision_raises_by_name():
    import metrpo_amd
    p = _params(); p['dynamics_model']['rollout_precision'] = 'fp16'
    with pytest.raises(ValueError, match='rollout_precision'):
        metrpo_amd.shapes_from_params(p)


@pytest.mark.parametrize('name', sorted(EXPECT))
def test_the_reference_files_keep_their_shapes(name):
    """Every key the shapes had before this extension is what it was (tests/test_params.py's table); the new key sits apart and the synthetic bench
    configuration of a file does not carry it."""
    import metrpo_amd
    from metrpo_amd import synthetic
    path = os.path.join(GOLD, 'params_%s.json' % name)
    sh = metrpo_amd.shapes_from_params(path)
    for k, v in EXPECT[name].items():
        assert sh[k] == v, (k, sh[k], v)
    assert sh['dyn_ext'] == dict(rollout_precision='f32') and sh['trpo_ext'] == dict(subsample_factor=1.0)
    q = _params(name); q['dynamics_model']['rollout_precision'] = 'bf16'
    sb = metrpo_amd.shapes_from_params(q)
    assert {k: v for k, v in sb.items() if k != 'dyn_ext'} == {k: v for k, v in sh.items() if k != 'dyn_ext'}
    assert 'rollout_precision' not in json.dumps(synthetic.config_from_params(q)) and synthetic.config_from_params(q) == synthetic.config_from_params(path)


def test_engine_binding_names_the_new_entry_points():
    from metrpo_amd import _lib, Engine
    assert _lib.SYMBOLS['metrpo_set_dyn_precision'][1] == [_lib._P, _lib._I] and _lib.SYMBOLS['metrpo_get_dyn_precision'][1] == [_lib._P]
    assert _lib.DYN_PRECISIONS == {'f32': 0, 'bf16': 1}
    assert callable(Engine.set_dyn_precision) and isinstance(Engine.dyn_precision, property)
