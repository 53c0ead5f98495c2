"""sdso_amd.abi is a view of include/sdso_abi.h; this file is what makes that true.  On the CPU, with the host compiler:

  layouts     a program written from the ctypes classes includes the header and prints sizeof of every structure and offsetof / size of
              every member; each line must equal what ctypes computes.  That the program compiles is the check of the member names.
  coverage    every `typedef struct { ... } sdso_*_t;` of the header has exactly one class, and every class names such a typedef.
  prototypes  every sdso_*(...) prototype of the header against abi.SIGNATURES: parameter count, kind of the return value, kind of
              every parameter.
  the rule    abi.ptr / abi.bind refuse what they cannot marshal, and a bound structure keeps its arrays alive.

Nothing runs on the GPU, and nothing is loaded into Python but the product library that tests/test_abi_cpu.py loads as well."""
import ctypes as C
import gc
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sdso_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdso_abi.h")
CXX = os.environ.get("CXX") or shutil.which("g++")
CALLBACK_TYPEDEFS = ("sdso_host_allreduce_fn", "sdso_host_allgather_fn")     # the parameters that are pointers without a `*`


def _header():
    """the header without comments and preprocessor lines"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)


def _typedefs():
    return re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(sdso_\w+)\s*;", _header())


def _c_member(name):
    return abi.C_MEMBER_NAMES.get(name, name)


@pytest.mark.skipif(CXX is None, reason="g++ not found")
def test_layouts_equal_the_compiled_header(tmp_path):
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "sdso_abi.h"', "int main() {"]
    expected = []
    for S in abi.STRUCTS:
        T = S._c_name_
        lines.append('  std::printf("%s %%zu\\n", sizeof(%s));' % (T, T))
        expected.append("%s %d" % (T, C.sizeof(S)))
        for name, _ in S._fields_:
            m, f = _c_member(name), getattr(S, name)
            lines.append('  std::printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (T, m, T, m, T, m))
            expected.append("%s.%s %d %d" % (T, m, f.offset, f.size))
    lines += ["  return 0;", "}"]
    src, exe = str(tmp_path / "abi_layout.cpp"), str(tmp_path / "abi_layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:]
    got = r.stdout.split("\n")[:-1]
    n_members = sum(len(S._fields_) for S in abi.STRUCTS)
    print("structures", len(abi.STRUCTS), "members", n_members)
    assert len(got) == len(expected) == len(abi.STRUCTS) + n_members
    wrong = [(g, e) for g, e in zip(got, expected) if g != e]
    assert not wrong, "header (left) against ctypes (right): %r" % (wrong[:10],)


def test_every_typedef_has_exactly_one_class():
    typedefs = _typedefs()
    assert len(typedefs) >= 34 and len(set(typedefs)) == len(typedefs)
    named = [S._c_name_ for S in abi.STRUCTS]
    assert sorted(named) == sorted(typedefs)        # equal as lists: no typedef without a class, no class twice, no class of another name
    for S in abi.STRUCTS:
        assert getattr(abi, S.__name__) is S
    # every ctypes structure the package defines is in STRUCTS, that is, names its C type
    for v in vars(abi).values():
        if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure:
            assert v in abi.STRUCTS, v


def _prototypes():
    """[(name, return type text, [parameter text])] of the header, in its order"""
    txt = re.sub(r"typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;", "", _header())
    txt = txt.replace('extern "C" {', "")
    out = []
    for stmt in txt.split(";"):
        m = re.match(r"\s*([\w\s\*]*?)\b(sdso_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, re.S)
        if not m or stmt.lstrip().startswith("typedef"):
            continue
        params = [p.strip() for p in m.group(3).split(",")]
        out.append((m.group(2), " ".join(m.group(1).split()), [] if params == ["void"] else params))
    return out


def _is_pointer_like(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C._CFuncPtr)))


SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long": C.c_long}


def test_signatures_equal_the_header_prototypes():
    protos = _prototypes()
    names = [p[0] for p in protos]
    assert len(names) == len(set(names)) >= 157
    assert sorted(names) == sorted(abi.SIGNATURES) and abi.EXPORTED_SYMBOLS == list(abi.SIGNATURES)
    wrong = []
    for name, ret, params in protos:
        sig = abi.SIGNATURES[name]
        argtypes, restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        if ret == "void":
            ok = restype is None
        elif "*" in ret:
            ok = _is_pointer_like(restype)
        else:
            ok = ret == "int" and restype is C.c_int
        if not ok:
            wrong.append((name, "returns", ret, restype))
        if len(params) != len(argtypes):
            wrong.append((name, "parameters", len(params), len(argtypes)))
            continue
        for i, (p, t) in enumerate(zip(params, argtypes)):
            words = [w for w in p.replace("*", " * ").split() if w != "const"]
            if "*" in words or "[" in p or words[0] in CALLBACK_TYPEDEFS:      # `const float K[4]` as a parameter is `const float*`
                ok = _is_pointer_like(t)
            else:
                ok = len(words) == 2 and t is SCALARS.get(words[0])       # a type word and the parameter's name
            if not ok:
                wrong.append((name, i, p, t))
    assert not wrong, wrong
    # what load() leaves on the library is the table
    L = abi.load()
    for name, sig in abi.SIGNATURES.items():
        argtypes, restype = sig if isinstance(sig, tuple) else (sig, C.c_int)
        assert list(getattr(L, name).argtypes) == list(argtypes) and getattr(L, name).restype is restype, name
    assert L.sdso_track_make_eval.restype is None


def test_ptr_refuses_what_it_cannot_marshal():
    for dt, pt in ((np.float32, abi.c_float_p), (np.float64, abi.c_double_p), (np.int32, abi.c_int_p), (np.uint8, abi.c_u8_p), (np.int8, abi.c_i8_p)):
        a = np.arange(6, dtype=dt).reshape(2, 3)
        p = abi.ptr(a)
        assert isinstance(p, pt) and C.addressof(p.contents) == a.ctypes.data and p[4] == a[1, 1]
    with pytest.raises(TypeError):
        abi.ptr(np.zeros(4, np.float16))
    with pytest.raises(TypeError):
        abi.ptr(np.zeros(4, np.int64))
    with pytest.raises(TypeError):
        abi.ptr(np.zeros((4, 3), np.float32)[:, 1])           # a column slice
    with pytest.raises(TypeError):
        abi.ptr([1.0, 2.0])
    assert abi.ptr(np.zeros((4, 3), np.float32)[1])           # a row is contiguous


def test_bind_refuses_a_wrong_dtype_and_keeps_the_arrays_alive():
    P = abi.TracePoints()
    with pytest.raises(TypeError):
        abi.bind(P, dict(color=np.zeros((3, 8), np.float64)))                # a double array for a float* member
    with pytest.raises(TypeError):
        abi.bind(P, dict(lastTraceStatus=np.zeros(3, np.float32)))
    with pytest.raises(AttributeError):
        abi.bind(P, dict(no_such_member=np.zeros(3, np.float32)))
    assert not P.color and not P.lastTraceStatus                            # a refused array sets nothing

    color = np.arange(24, dtype=np.float32).reshape(3, 8)
    status = np.array([5, 0, 2], np.uint8)
    assert abi.bind(P, dict(color=color, lastTraceStatus=status, gradH=None)) is P
    assert not P.gradH and C.addressof(P.color.contents) == color.ctypes.data
    want_c, want_s = color.ravel().tolist(), status.tolist()
    del color, status
    gc.collect()
    junk = [np.full(24, -1.0, np.float32) for _ in range(64)]               # would land in the freed blocks
    assert P.color[:24] == want_c and P.lastTraceStatus[:3] == want_s
    del junk

    # the builders go through the same two functions: what they return reads right after the caller's arrays are gone
    E, keep = abi.make_window_edit(drop_res=[4, 2, 9], drop_point=np.array([0, 1, 1, 0], np.uint8))
    del keep
    gc.collect()
    assert E.n_drop_res == 3 and E.drop_res[:3] == [4, 2, 9] and E.drop_point[:4] == [0, 1, 1, 0] and not E.remove_points and E.n_remove_points == 0
