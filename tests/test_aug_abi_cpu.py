"""CPU-side checks of the second C ABI: libmss_aug.so builds, loads, exports exactly what include/mss_aug_hip.h declares, is
bound with the declared types, and refuses bad arguments before any launch. No compute."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mss_aug_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib_aug
    return _lib_aug


def declarations():
    """(return type, name, [parameter declarations]) of every function the header declares: comments and preprocessor lines
    removed, a declaration is `<type words> mss_aug_name(<no parentheses>);`."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", ";", src, flags=re.M)
    return [(" ".join(ret.split()), name, [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in re.findall(r"(?:^|[;{}])\s*((?:\w+\s+)+?)\s*(mss_aug_\w+)\s*\(([^()]*)\)\s*(?=;)", src)]


def test_every_declared_symbol_is_exported_and_bound(lib):
    decls = declarations()
    names = sorted(d[1] for d in decls)
    assert len(names) == len(set(names)) == 12
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.AUG_LIB_PATH], text=True)
    exported = set(re.findall(r" T (mss_\w+)", out))
    assert exported == set(names) == set(lib.AUG_SIGNATURES)
    assert lib.load().mss_aug_abi_version() == lib.MSS_AUG_ABI_VERSION == int(re.search(r"#define MSS_AUG_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    # the two libraries share no symbol, and the first one's table is untouched
    from multishiftseg_amd import _lib
    main = set(re.findall(r" T (mss_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)))
    assert not main & exported and len(_lib.SIGNATURES) == 142
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", lib.AUG_LIB_PATH], text=True)
    assert "mss" not in undefined.lower(), "libmss_aug.so must not need any symbol of libmss_hip.so"


def test_ctypes_table_matches_header(lib):
    scalars = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}

    def ctype(param):
        if "*" in param:
            m = re.match(r"(?:const )?(Mss\w+) ?\*", param)
            return ctypes.POINTER(getattr(lib, m.group(1))) if m else ctypes.c_void_p
        base = re.sub(r" ?\w+$", "", param).replace("const ", "").strip()
        assert base in scalars, f"a parameter type this test does not know: {param!r}"
        return scalars[base]
    wrong = []
    for ret, name, params in declarations():
        want = [] if params in (["void"], [""]) else [ctype(p) for p in params]
        if name in lib.AUG_VALUE_RESTYPE:
            if lib.AUG_VALUE_RESTYPE[name] is not scalars[ret] or want != lib.AUG_SIGNATURES[name]:
                wrong.append((name, "value entry point"))
            continue
        if ret != "int" or params[-1] != "void* stream":
            wrong.append((name, "a status-returning entry point returns int and ends in the stream"))
        if want[:-1] != lib.AUG_SIGNATURES[name][:-1] or lib.AUG_SIGNATURES[name][-1] is not ctypes.c_void_p:
            wrong.append((name, "argtypes"))
    assert not wrong, wrong
    handle = lib.load()
    for name in lib.AUG_SIGNATURES:
        assert getattr(handle, name).restype is lib.AUG_VALUE_RESTYPE.get(name, ctypes.c_int), name


def test_point_ops_struct_layout(lib, tmp_path):
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "mss_aug_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(MssAugPointOps), '
            "offsetof(MssAugPointOps, kind), offsetof(MssAugPointOps, factor));return 0;}")
    exe = str(tmp_path / "aug_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=code.encode(), check=True)
    size, o_kind, o_factor = (int(v) for v in subprocess.check_output([exe], text=True).split())
    cls = lib.MssAugPointOps
    assert (ctypes.sizeof(cls), cls.kind.offset, cls.factor.offset) == (size, o_kind, o_factor)


def test_entry_points_validate_arguments_before_any_launch(lib):
    """Raw calls with a NULL stream and pointers nothing dereferences: every case returns before its launch, with the code the
    header documents; the order of the checks decides the code of a call with more than one fault."""
    OK_NEVER, BAD, UNS = 0, lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    h = lib.load()
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)
    Y = X + 16
    big = 1 << 15                       # big * big > MSS_AUG_MAX_PIXELS
    k9 = ctypes.cast((ctypes.c_float * 9)(*[1 / 9.0] * 9), ctypes.c_void_p)
    d3 = ctypes.cast((ctypes.c_double * 3)(1.0, 1.0, 1.0), ctypes.c_void_p)

    def ops(n, kind=1):
        po = lib.MssAugPointOps(n=n)
        for k in range(8):
            po.kind[k] = kind
        return ctypes.byref(po)

    def geom(*v):
        return ctypes.cast((ctypes.c_int * 6)(*v), ctypes.c_void_p)
    got = {
        "load null": h.mss_aug_load_f32(None, X, X, X, 4, 4, 0, 0.0, X, X, None),
        "load H=0": h.mss_aug_load_f32(X, X, X, X, 0, 4, 0, 0.0, X, X, None),
        "load huge": h.mss_aug_load_f32(X, X, X, X, big, big, 0, 0.0, X, X, None),
        "load p": h.mss_aug_load_f32(X, X, X, X, 4, 4, 1, 1.5, X, X, None),
        "load null+huge": h.mss_aug_load_f32(X, X, X, X, big, big, 0, 0.0, None, X, None),
        "stats null ws": h.mss_aug_stats_f32(X, 2, 4, 4, None, X, None),
        "stats N=0": h.mss_aug_stats_f32(X, 0, 4, 4, X, X, None),
        "stats N=65": h.mss_aug_stats_f32(X, 65, 4, 4, X, X, None),
        "point null ops": h.mss_aug_pointwise_f32(X, 2, 4, 4, None, None, None),
        "point n=0": h.mss_aug_pointwise_f32(X, 2, 4, 4, ops(0), None, None),
        "point n=9": h.mss_aug_pointwise_f32(X, 2, 4, 4, ops(9), None, None),
        "point kind=6": h.mss_aug_pointwise_f32(X, 2, 4, 4, ops(2, 6), X, None),
        "point contrast without stats": h.mss_aug_pointwise_f32(X, 2, 4, 4, ops(1, 2), None, None),
        "point huge before ops": h.mss_aug_pointwise_f32(X, 2, big, big, None, None, None),
        "blur 4x9": h.mss_aug_blur9_f32(X, Y, 2, 4, 9, k9, None),
        "blur 9x4": h.mss_aug_blur9_f32(X, Y, 2, 9, 4, k9, None),
        "blur in place": h.mss_aug_blur9_f32(X, X, 2, 9, 9, k9, None),
        "blur null k9": h.mss_aug_blur9_f32(X, Y, 2, 9, 9, None, None),
        "sharp in place": h.mss_aug_sharpness_f32(X, X, 2, 9, 9, 1.0, None),
        "sharp null": h.mss_aug_sharpness_f32(X, None, 2, 9, 9, 1.0, None),
        "equalize null ws": h.mss_aug_equalize_f32(X, 2, 9, 9, None, None),
        "equalize huge": h.mss_aug_equalize_f32(X, 2, big, big, X, None),
        "resize OH=0": h.mss_aug_resize_f32(X, X, 2, 9, 9, 0, 5, Y, Y, None),
        "resize huge out": h.mss_aug_resize_f32(X, X, 2, 9, 9, big, big, Y, Y, None),
        "rotate nan": h.mss_aug_rotate_f32(X, X, 2, 9, 9, float("nan"), 0.0, Y, Y, None),
        "rotate c=2": h.mss_aug_rotate_f32(X, X, 2, 9, 9, 2.0, 0.0, Y, Y, None),
        "window outside": h.mss_aug_window_f32(X, X, 2, 9, 9, 0, 0, 5, 0, 5, 9, Y, Y, None),
        "window negative": h.mss_aug_window_f32(X, X, 2, 9, 9, 0, 0, -1, 0, 5, 9, Y, Y, None),
        "window h=0": h.mss_aug_window_f32(X, X, 2, 9, 9, 0, 0, 0, 0, 0, 9, Y, Y, None),
        "finish null mean": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 0, 0, 9, 9, None, d3, None, None, 0, 0, None, 1, 0, Y, Y, None),
        "finish outside": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 1, 0, 9, 9, d3, d3, None, None, 0, 0, None, 1, 0, Y, Y, None),
        "finish b=B": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 0, 0, 9, 9, d3, d3, None, None, 0, 0, None, 2, 2, Y, Y, None),
        "finish geom without object": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 0, 0, 9, 9, d3, d3, None, None, 0, 0, geom(0, 0, 1, 1, 0, 0), 1, 0, Y, Y, None),
        "finish region outside object": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 0, 0, 9, 9, d3, d3, X, X, 4, 4, geom(2, 0, 3, 1, 0, 0), 1, 0, Y, Y, None),
        "finish negative geom": h.mss_aug_finish_f32(X, X, 9, 9, 0, 0, 0, 0, 9, 9, d3, d3, X, X, 4, 4, geom(0, 0, 1, 1, -1, 0), 1, 0, Y, Y, None),
    }
    want = {k: BAD for k in got}
    for k in ("load huge", "stats N=65", "point huge before ops", "blur 4x9", "blur 9x4", "equalize huge", "resize huge out"):
        want[k] = UNS
    assert got == want and OK_NEVER not in got.values()
    assert lib.value("mss_aug_stats_ws_doubles", 0, 5) == 0 and lib.value("mss_aug_stats_ws_doubles", 64, 64) == 8
    assert lib.value("mss_aug_stats_ws_doubles", 1024, 2048) == 256 * 8
