"""CPU: the C-ABI library builds, loads, and exports every symbol include/mmla.h declares.
No compute calls (there is no GPU here); creating a context without a device must fail cleanly."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, 'include', 'mmla.h')
LIB = os.path.join(REPO, 'mmla_audio_amd', 'libmmla.so')


def declared_symbols():
    src = open(HEADER).read()
    return sorted(set(re.findall(r'^\s*(?:int|const char\*)\s+(mmla_\w+)\s*\(', src, re.M)))


def test_header_declares_expected_entry_points():
    syms = declared_symbols()
    for s in ('mmla_create', 'mmla_destroy', 'mmla_load_weights', 'mmla_od_features',
              'mmla_si_features', 'mmla_si_features_seq', 'mmla_od_forward', 'mmla_si_forward',
              'mmla_od_pipeline', 'mmla_si_pipeline', 'mmla_last_error'):
        assert s in syms


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        pytest.skip('libmmla.so not built (run __graft_entry__.build())')
    return ctypes.CDLL(LIB)


def test_library_exports_every_declared_symbol(lib):
    for s in declared_symbols():
        assert hasattr(lib, s), f'{s} declared in include/mmla.h but not exported'


def test_shim_signatures_cover_header():
    from mmla_audio_amd import _lib
    declared = set(declared_symbols()) - {'mmla_last_error'}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    # ... and with the header's parameter list: the same count, and per parameter the same class
    # (pointer, int64_t, int32_t / int, uint32_t, float, double)
    src = re.sub(r'/\*.*?\*/|//[^\n]*', '', open(HEADER).read(), flags=re.S)
    protos = dict(re.findall(r'^\s*int\s+(mmla_\w+)\s*\(([^)]*)\)\s*;', src, re.M))
    assert declared <= set(protos)
    scalars = {'int64_t': 'i64', 'int32_t': 'i32', 'int': 'i32', 'uint32_t': 'u32', 'float': 'f32',
               'double': 'f64'}

    def header_class(param):
        if '*' in param:
            return 'ptr'
        words = [w for w in param.split() if w != 'const']
        assert len(words) == 2 and words[0] in scalars, param      # type, name
        return scalars[words[0]]

    def shim_class(t):
        if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
            return 'ptr'
        return {ctypes.c_int64: 'i64', ctypes.c_int32: 'i32', ctypes.c_int: 'i32', ctypes.c_uint32: 'u32',
                ctypes.c_float: 'f32', ctypes.c_double: 'f64'}[t]

    for name in sorted(declared):
        params = [p.strip() for p in protos[name].split(',')]
        params = [] if params in ([''], ['void']) else params
        assert [header_class(p) for p in params] == [shim_class(t) for t in _lib.SIGNATURES[name]], name


def test_abi_version(lib):
    assert lib.mmla_abi_version() == 2


def test_null_args_rejected_without_device(lib):
    lib.mmla_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    assert lib.mmla_create(0, None) == -1          # MMLA_E_INVALID before touching HIP
    lib.mmla_destroy.argtypes = [ctypes.c_void_p]
    assert lib.mmla_destroy(None) == -1


def test_package_imports_without_gpu():
    import mmla_audio_amd
    from mmla_audio_amd import weights
    assert weights.n_params(weights.OD) > 1_000_000
    assert mmla_audio_amd.__doc__
