"""Host-side checks of metrpo_ensemble_disagreement (include/metrpo.h) that need no GPU: the symbols, the struct's layout, the NULL checks, and that the
addition leaves the ABI version and the option table alone."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound():
    from metrpo_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'metrpo.h')).read()
    for n in ('metrpo_ensemble_disagreement', 'metrpo_last_disagreement_kernel'):
        assert hasattr(_lib.lib, n) and n in _lib.SYMBOLS and n + '(' in hdr
    assert _lib.SYMBOLS['metrpo_ensemble_disagreement'][1] == [_lib._P, C.POINTER(_lib.DisagreementArgs), _lib._P]
    assert _lib.SYMBOLS['metrpo_last_disagreement_kernel'] == (_lib._I, [_lib._P])


def test_struct_layout_matches_the_header():
    from metrpo_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'metrpo.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} metrpo_disagreement_args;', hdr).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.search(r'(\w+)\s*$', d.strip()).group(1) for d in body.split(';') if d.strip()]
    assert names == [f[0] for f in _lib.DisagreementArgs._fields_]
    # int64 N, two int32, ten pointers (LP64)
    assert C.sizeof(_lib.DisagreementArgs) == 8 + 2 * 4 + 10 * 8
    assert _lib.DisagreementArgs.d_obs.offset == 16 and _lib.DisagreementArgs.d_sums.offset == 88


def test_null_checks_and_abi_version():
    from metrpo_amd import _lib
    lib = _lib.lib
    assert lib.metrpo_ensemble_disagreement(None, None, None) == -2                       # METRPO_ENULL
    assert lib.metrpo_ensemble_disagreement(None, C.byref(_lib.DisagreementArgs()), None) == -2
    assert lib.metrpo_last_disagreement_kernel(None) == -2
    assert lib.metrpo_abi_version() == 4


def test_option_table_still_has_25_keys():
    from metrpo_amd import _lib
    n = 0
    while _lib.lib.metrpo_option_name(n) is not None:
        n += 1
    assert n == 25


def test_exported_from_the_package():
    import metrpo_amd
    assert 'ensemble_disagreement' in metrpo_amd.__all__ and metrpo_amd.ensemble_disagreement is metrpo_amd.model_error.ensemble_disagreement
    assert hasattr(metrpo_amd.Engine, 'ensemble_disagreement') and hasattr(metrpo_amd.Engine, 'last_disagreement_kernel')
