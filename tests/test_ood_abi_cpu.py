"""CPU-side checks of the third C ABI: libmss_ood.so builds, loads, exports exactly what include/mss_ood_hip.h declares, is bound
with the declared types, shares nothing with the other two libraries and refuses bad arguments before any launch. No compute."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mss_ood_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib_ood
    return _lib_ood


def declarations():
    """(return type, name, [parameter declarations]) of every function the header declares: comments and preprocessor lines
    removed, a declaration is `<type words> mss_ood_name(<no parentheses>);`."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", ";", src, flags=re.M)
    return [(" ".join(ret.split()), name, [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in re.findall(r"(?:^|[;{}])\s*((?:\w+\s+)+?)\s*(mss_ood_\w+)\s*\(([^()]*)\)\s*(?=;)", src)]


def _exported(path):
    return set(re.findall(r" T (mss\w+)", subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = sorted(d[1] for d in declarations())
    assert len(names) == len(set(names)) == 5
    exported = _exported(lib.OOD_LIB_PATH)
    assert exported == set(names) == set(lib.OOD_SIGNATURES)
    header = open(HEADER).read()
    assert lib.load().mss_ood_abi_version() == lib.MSS_OOD_ABI_VERSION == int(re.search(r"#define MSS_OOD_ABI_VERSION (\d+)", header).group(1))
    assert lib.MSS_OOD_MAX_CLASSES == int(re.search(r"#define MSS_OOD_MAX_CLASSES (\d+)", header).group(1))
    assert lib.MSS_OOD_MAX_PIXELS == int(re.search(r"#define MSS_OOD_MAX_PIXELS (0x[0-9a-f]+)ll", header).group(1), 16)
    assert lib.KINDS == {"margin": int(re.search(r"#define MSS_OOD_MARGIN (\d+)", header).group(1)),
                         "bce": int(re.search(r"#define MSS_OOD_BCE (\d+)", header).group(1))}


def test_the_three_libraries_share_no_symbol_and_the_other_tables_are_untouched(lib):
    from multishiftseg_amd import _lib, _lib_aug
    ood, main, aug = _exported(lib.OOD_LIB_PATH), _exported(_lib.LIB_PATH), _exported(_lib_aug.AUG_LIB_PATH)
    assert ood and not ood & main and not ood & aug
    assert len(_lib.SIGNATURES) == 142 and len(_lib_aug.AUG_SIGNATURES) == 12
    assert not set(lib.OOD_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_aug.AUG_SIGNATURES))
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", lib.OOD_LIB_PATH], text=True)
    assert "mss" not in undefined.lower(), "libmss_ood.so must not need any symbol of the other two libraries"
    needed = subprocess.check_output(["readelf", "-d", lib.OOD_LIB_PATH], text=True)
    assert "libmss" not in "".join(line for line in needed.splitlines() if "NEEDED" in line)


def test_ctypes_table_matches_header(lib):
    scalars = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}

    def ctype(param):
        if "*" in param:
            return ctypes.c_void_p
        base = re.sub(r" ?\w+$", "", param).replace("const ", "").strip()
        assert base in scalars, f"a parameter type this test does not know: {param!r}"
        return scalars[base]
    wrong = []
    for ret, name, params in declarations():
        want = [] if params in (["void"], [""]) else [ctype(p) for p in params]
        if name in lib.OOD_VALUE_RESTYPE:
            if lib.OOD_VALUE_RESTYPE[name] is not scalars[ret] or want != lib.OOD_SIGNATURES[name]:
                wrong.append((name, "value entry point"))
            continue
        if ret != "int" or params[-1] != "void* stream":
            wrong.append((name, "a status-returning entry point returns int and ends in the stream"))
        if want[:-1] != lib.OOD_SIGNATURES[name][:-1] or lib.OOD_SIGNATURES[name][-1] is not ctypes.c_void_p:
            wrong.append((name, "argtypes"))
    assert not wrong, wrong
    handle = lib.load()
    for name in lib.OOD_SIGNATURES:
        assert getattr(handle, name).restype is lib.OOD_VALUE_RESTYPE.get(name, ctypes.c_int), name
        assert list(getattr(handle, name).argtypes) == lib.OOD_SIGNATURES[name], name


def test_entry_points_validate_arguments_before_any_launch(lib):
    """Raw calls with a NULL stream and pointers nothing dereferences: every case returns before its launch, with the code the
    header documents; the order of the checks decides the code of a call with more than one fault."""
    OK_NEVER, BAD, UNS = 0, lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    h = lib.load()
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)
    big = 1 << 16                       # 2 * big * big > MSS_OOD_MAX_PIXELS
    nan, inf = float("nan"), float("inf")
    fwd, bwd = h.mss_ood_pixel_loss_f32, h.mss_ood_pixel_loss_backward_f32
    got = {
        "negmax null mix": h.mss_ood_negmax_f32(None, 2, 3, 4, 4, X, None),
        "negmax null t": h.mss_ood_negmax_f32(X, 2, 3, 4, 4, None, None),
        "negmax B=0": h.mss_ood_negmax_f32(X, 0, 3, 4, 4, X, None),
        "negmax C=0": h.mss_ood_negmax_f32(X, 2, 0, 4, 4, X, None),
        "negmax w=-1": h.mss_ood_negmax_f32(X, 2, 3, 4, -1, X, None),
        "negmax C=33": h.mss_ood_negmax_f32(X, 2, 33, 4, 4, X, None),
        "negmax huge": h.mss_ood_negmax_f32(X, 2, 3, big, big, X, None),
        "negmax null+huge": h.mss_ood_negmax_f32(None, 2, 3, big, big, X, None),
        "negmax C=0+huge": h.mss_ood_negmax_f32(X, 2, 0, big, big, X, None),
        "fwd null t": fwd(None, X, 2, 4, 4, 8, 8, 0, 1.0, X, X, X, None, None),
        "fwd null ood": fwd(X, None, 2, 4, 4, 8, 8, 0, 1.0, X, X, X, None, None),
        "fwd null partial": fwd(X, X, 2, 4, 4, 8, 8, 0, 1.0, None, X, X, None, None),
        "fwd null stats": fwd(X, X, 2, 4, 4, 8, 8, 0, 1.0, X, None, X, None, None),
        "fwd null loss": fwd(X, X, 2, 4, 4, 8, 8, 0, 1.0, X, X, None, X, None),
        "fwd H=0": fwd(X, X, 2, 4, 4, 0, 8, 0, 1.0, X, X, X, None, None),
        "fwd h=0": fwd(X, X, 2, 0, 4, 8, 8, 0, 1.0, X, X, X, None, None),
        "fwd kind=2": fwd(X, X, 2, 4, 4, 8, 8, 2, 1.0, X, X, X, None, None),
        "fwd kind=-1": fwd(X, X, 2, 4, 4, 8, 8, -1, 1.0, X, X, X, None, None),
        "fwd margin nan": fwd(X, X, 2, 4, 4, 8, 8, 0, nan, X, X, X, None, None),
        "fwd margin inf, bce": fwd(X, X, 2, 4, 4, 8, 8, 1, inf, X, X, X, None, None),
        "fwd huge out": fwd(X, X, 2, 4, 4, big, big, 0, 1.0, X, X, X, None, None),
        "fwd huge low": fwd(X, X, 2, big, big, 8, 8, 1, 0.0, X, X, X, None, None),
        "fwd kind=2+huge": fwd(X, X, 2, 4, 4, big, big, 2, 1.0, X, X, X, None, None),
        "bwd null mix": bwd(None, X, X, X, X, 2, 3, 4, 4, 8, 8, 0, 1.0, X, None),
        "bwd null stats": bwd(X, X, X, None, X, 2, 3, 4, 4, 8, 8, 0, 1.0, X, None),
        "bwd null gloss": bwd(X, X, X, X, None, 2, 3, 4, 4, 8, 8, 0, 1.0, X, None),
        "bwd null dmix": bwd(X, X, X, X, X, 2, 3, 4, 4, 8, 8, 0, 1.0, None, None),
        "bwd C=0": bwd(X, X, X, X, X, 2, 0, 4, 4, 8, 8, 0, 1.0, X, None),
        "bwd W=0": bwd(X, X, X, X, X, 2, 3, 4, 4, 8, 0, 0, 1.0, X, None),
        "bwd kind=7": bwd(X, X, X, X, X, 2, 3, 4, 4, 8, 8, 7, 1.0, X, None),
        "bwd margin -inf": bwd(X, X, X, X, X, 2, 3, 4, 4, 8, 8, 0, -inf, X, None),
        "bwd C=33": bwd(X, X, X, X, X, 2, 33, 4, 4, 8, 8, 0, 1.0, X, None),
        "bwd huge out": bwd(X, X, X, X, X, 2, 3, 4, 4, big, big, 1, 1.0, X, None),
        "bwd margin nan+C=33": bwd(X, X, X, X, X, 2, 33, 4, 4, 8, 8, 0, nan, X, None),
    }
    want = {k: BAD for k in got}
    for k in ("negmax C=33", "negmax huge", "fwd huge out", "fwd huge low", "bwd C=33", "bwd huge out"):
        want[k] = UNS
    assert got == want and OK_NEVER not in got.values()
    assert lib.value("mss_ood_loss_partials", 0) == 0 and lib.value("mss_ood_loss_partials", -5) == 0
    assert lib.value("mss_ood_loss_partials", lib.MSS_OOD_MAX_PIXELS + 1) == 0
    src = open(os.path.join(ROOT, "multishiftseg_amd", "csrc", "m2f_ood_loss.hip")).read()
    per = int(re.search(r"constexpr int OD_T = (\d+);", src).group(1)) * int(re.search(r"constexpr int OD_PX = (\d+);", src).group(1))
    for n in (1, per - 1, per, per + 1, 16 * 704 * 704, lib.MSS_OOD_MAX_PIXELS):
        assert lib.value("mss_ood_loss_partials", n) == -(-n // per), n
