"""CPU checks of the 'l-bfgs' policy update: argument errors of the new C entry points come back as status codes before the device is
touched, LBFGS's defaults are scipy's L-BFGS-B defaults, and from_params still refuses 'l-bfgs' (its wiring is a separate change)."""
import ctypes as C
import inspect
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_codes_without_gpu():
    from metrpo_amd import _lib
    lib = _lib.lib
    o = _lib.LbfgsOpts()
    r = _lib.LbfgsResult()
    x = C.c_void_p(1)
    assert lib.metrpo_lbfgs_begin(None, 4, x, C.byref(o), x, None) == -2             # METRPO_ENULL
    assert lib.metrpo_lbfgs_iterate(None, x, x, x, x, None) == -2
    assert lib.metrpo_lbfgs_get_result(None, C.byref(r), None) == -2
    assert lib.metrpo_lbfgs_policy(None, x, 10, 5, 1.0, C.byref(o), C.byref(r), None) == -2


def test_struct_layouts():
    from metrpo_amd import _lib
    assert C.sizeof(_lib.LbfgsOpts) == 4 * 4 + 2 * 8 + 2 * 4
    assert C.sizeof(_lib.LbfgsResult) == 8 + 6 * 4
    hdr = open(os.path.join(REPO, 'include', 'metrpo.h')).read()
    for name in ('metrpo_lbfgs_begin', 'metrpo_lbfgs_iterate', 'metrpo_lbfgs_get_result', 'metrpo_lbfgs_policy'):
        assert name + '(' in hdr and name in _lib.SYMBOLS and hasattr(_lib.lib, name)


def test_defaults_are_scipy_defaults():
    import metrpo_amd
    so = pytest.importorskip('scipy.optimize')
    sig = inspect.signature(metrpo_amd.LBFGS.__init__).parameters
    import scipy.optimize._lbfgsb_py as lb
    ref = inspect.signature(lb._minimize_lbfgsb).parameters
    assert sig['maxcor'].default == ref['maxcor'].default == 10
    assert sig['ftol'].default == ref['ftol'].default
    assert sig['gtol'].default == ref['gtol'].default
    assert sig['maxiter'].default == ref['maxiter'].default
    assert sig['maxfun'].default == ref['maxfun'].default
    assert sig['maxls'].default == ref['maxls'].default
    eo = inspect.signature(metrpo_amd.Engine.lbfgs_opts).parameters
    for k, v in (('m', 10), ('maxls', 20), ('maxiter', 15000), ('maxfun', 15000), ('ftol', ref['ftol'].default), ('gtol', 1e-5)):
        assert eo[k].default == v


def test_messages_are_scipys():
    from metrpo_amd.lbfgs import task_message
    import lbfgs_ref as L
    assert task_message((4, 402)) == 'CONVERGENCE: RELATIVE REDUCTION OF F <= FACTR*EPSMCH'
    assert task_message((5, 504)) == 'STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT'
    for t in (L.CONV_PG, L.CONV_F, L.STOP_ITER, L.STOP_FUN, L.ABNORMAL):
        assert task_message(t) == L.message(t)


def test_from_params_still_refuses_lbfgs():
    from metrpo_amd import from_params
    p = json.load(open(os.path.join(REPO, 'tests', 'golden', 'params_swimmer.json')))
    p['algo'] = 'l-bfgs'
    with pytest.raises(ValueError, match='l-bfgs'):
        from_params(p)


def test_product_does_not_import_scipy():
    pkg = os.path.join(REPO, 'me-trpo_amd')
    for f in os.listdir(pkg):
        if f.endswith('.py'):
            assert 'import scipy' not in open(os.path.join(pkg, f)).read() and 'from scipy' not in open(os.path.join(pkg, f)).read(), f
