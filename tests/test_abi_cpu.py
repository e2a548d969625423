"""The C-ABI shared library loads without a GPU and exports every symbol include/mv2d_hip.h declares; argument
validation errors are reported through the return code + mv2d_last_error (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from mv2d_amd import _lib
    return _lib.load()


def declared_functions():
    src = open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mv2d_\w+)\s*\(', src)))


def test_header_symbols_are_exported(lib):
    names = declared_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/mv2d_hip.h but not exported'
    from mv2d_amd._lib import SIGNATURES
    assert set(SIGNATURES) == set(names), set(SIGNATURES) ^ set(names)


C_TYPES = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong, 'unsigned': ctypes.c_uint,
           'unsigned int': ctypes.c_uint}


def _ctype(decl):
    """ctypes type of a C return type or parameter type as include/mv2d_hip.h writes them: every pointer is a c_void_p, char* a c_char_p"""
    words = [t for t in decl.replace('*', ' * ').split() if t != 'const']
    if '*' in words:
        return ctypes.c_char_p if words[0] == 'char' else ctypes.c_void_p
    return C_TYPES[' '.join(words)]


def declared_signatures():
    """{name: (restype, [argtypes])} of every `ret mv2d_x(args);` of the header, comments stripped"""
    src = open(os.path.join(ROOT, 'include', 'mv2d_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    src = re.sub(r'//[^\n]*|^\s*#[^\n]*', ' ', src, flags=re.M)
    sigs = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w\s*]*?)\b(mv2d_\w+)\s*\(([^()]*)\)\s*;', src):
        args = [a.strip() for a in args.split(',')]
        args = [] if args == ['void'] else [re.sub(r'\w+\s*(\[\w*\])?$', lambda m: '*' if m.group(1) else '', a) for a in args]     # (drop the parameter's name)
        assert name not in sigs, f'{name} is declared twice'
        sigs[name] = (_ctype(ret), [_ctype(a) for a in args])
    return sigs


def test_signatures_agree_with_the_header_position_by_position():
    """Every call in ops.py rests on SIGNATURES: return type and every argument type against the header's declaration (a char* may be bound as
    c_void_p)."""
    from mv2d_amd._lib import SIGNATURES
    decl = declared_signatures()
    assert set(decl) == set(declared_functions()), set(decl) ^ set(declared_functions())           # every declaration parsed
    assert set(decl) == set(SIGNATURES)
    same = lambda want, got: got is want or (want is ctypes.c_char_p and got is ctypes.c_void_p)
    for name, (ret, args) in decl.items():
        got_ret, got_args = SIGNATURES[name]
        assert same(ret, got_ret), f'{name}: returns {ret.__name__} in the header, {got_ret.__name__} in SIGNATURES'
        assert len(args) == len(got_args), f'{name}: {len(args)} arguments in the header, {len(got_args)} in SIGNATURES'
        for i, (a, b) in enumerate(zip(args, got_args)):
            assert same(a, b), f'{name}: argument {i} is {a.__name__} in the header, {b.__name__} in SIGNATURES'


def test_error_reporting_without_gpu(lib):
    assert lib.mv2d_abi_version() == 6
    rc = lib.mv2d_gemm_f32(None, None, 0, None, None, 1, 1, 32, 32, 32, 1, 0, 1.0, 0.0, None, 0, 1, 0, 1, 0, 0, 0, 0, None)
    assert rc == -1
    assert b'mv2d_gemm_f32' in lib.mv2d_last_error()
    buf = ctypes.create_string_buffer(64)
    rc = lib.mv2d_row_ln(None, 0, 0, None, None, None, None, 0, None, None, None, None, None, None, 0, 1e-5, 0, None)
    assert rc == -1 and b'mv2d_row_ln' in lib.mv2d_last_error()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mv2d_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(_lib.Mv2dHipError):
        _lib.load(str(tmp_path / 'nope.so'))
