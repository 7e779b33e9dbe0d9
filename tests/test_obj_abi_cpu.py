"""CPU-side checks of the fourth C ABI: libmss_obj.so builds, loads, exports exactly what include/mss_obj_hip.h declares, is bound
with the declared types, shares nothing with the other three libraries and refuses bad arguments before any launch. No compute."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mss_obj_hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib_obj
    return _lib_obj


def declarations():
    """(return type, name, [parameter declarations]) of every function the header declares: comments and preprocessor lines
    removed, a declaration is `<type words> mss_obj_name(<no parentheses>);`."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", ";", src, flags=re.M)
    return [(" ".join(ret.split()), name, [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in re.findall(r"(?:^|[;{}])\s*((?:\w+\s+)+?)\s*(mss_obj_\w+)\s*\(([^()]*)\)\s*(?=;)", src)]


def _exported(path):
    return set(re.findall(r" T (mss\w+)",subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = sorted(d[1] for d in declarations())
    assert len(names) == len(set(names)) == 3
    exported = _exported(lib.OBJ_LIB_PATH)
    assert exported == set(names) == set(lib.OBJ_SIGNATURES)
    assert all(n.startswith("mss_obj_") for n in exported)
    header = open(HEADER).read()
    assert lib.load().mss_obj_abi_version() == lib.MSS_OBJ_ABI_VERSION == int(re.search(r"#define MSS_OBJ_ABI_VERSION (\d+)", header).group(1)) == 1
    assert lib.MSS_OBJ_MAX_PIXELS == int(re.search(r"#define MSS_OBJ_MAX_PIXELS (0x[0-9a-f]+)ll", header).group(1), 16)
    for name in ("MSS_OBJ_MAX_BBOX_JOBS", "MSS_OBJ_MAX_BATCH", "MSS_OBJ_MAX_ROWS", "MSS_OBJ_BBOX_JOB_INTS", "MSS_OBJ_RESCALE_JOB_INTS"):
        assert getattr(lib, name) == int(re.search(rf"#define {name} (\w+)", header).group(1), 0), name
    # the launch grid behind MSS_OBJ_MAX_ROWS: 65535 tiles of OB_TH rows
    src = open(os.path.join(ROOT, "multishiftseg_amd", "csrc", "obj_bank.hip")).read()
    assert lib.MSS_OBJ_MAX_ROWS == 65535 * int(re.search(r"constexpr int OB_TH = (\d+);", src).group(1))


def test_the_four_libraries_share_no_symbol_and_the_other_tables_are_untouched(lib):
    from multishiftseg_amd import _lib, _lib_aug, _lib_ood
    obj = _exported(lib.OBJ_LIB_PATH)
    others = [_exported(_lib.LIB_PATH), _exported(_lib_aug.AUG_LIB_PATH), _exported(_lib_ood.OOD_LIB_PATH)]
    assert obj and all(o and not obj & o for o in others)
    assert not others[0] & others[1] and not others[0] & others[2] and not others[1] & others[2]
    assert len(_lib.SIGNATURES) == 142 and len(_lib_aug.AUG_SIGNATURES) == 12 and len(_lib_ood.OOD_SIGNATURES) == 5
    assert not set(lib.OBJ_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib_aug.AUG_SIGNATURES) | set(_lib_ood.OOD_SIGNATURES))
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", lib.OBJ_LIB_PATH], text=True)
    assert "mss" not in undefined.lower(), "libmss_obj.so must not need any symbol of the other three libraries"
    needed = subprocess.check_output(["readelf", "-d", lib.OBJ_LIB_PATH], text=True)
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
        if name in lib.OBJ_VALUE_RESTYPE:
            if lib.OBJ_VALUE_RESTYPE[name] is not scalars[ret] or want != lib.OBJ_SIGNATURES[name]:
                wrong.append((name, "value entry point"))
            continue
        if ret != "int" or params[-1] != "void* stream":
            wrong.append((name, "a status-returning entry point returns int and ends in the stream"))
        if want[:-1] != lib.OBJ_SIGNATURES[name][:-1] or lib.OBJ_SIGNATURES[name][-1] is not ctypes.c_void_p:
            wrong.append((name, "argtypes"))
    assert not wrong, wrong
    handle = lib.load()
    for name in lib.OBJ_SIGNATURES:
        assert getattr(handle, name).restype is lib.OBJ_VALUE_RESTYPE.get(name, ctypes.c_int), name
        assert list(getattr(handle, name).argtypes) == lib.OBJ_SIGNATURES[name], name


def test_entry_points_validate_arguments_before_any_launch(lib):
    """Raw calls with a NULL stream and pointers nothing dereferences: every case returns before its launch, with the code the
    header documents; the order of the checks decides the code of a call with more than one fault."""
    OK_NEVER, BAD, UNS = 0, lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    h = lib.load()
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)
    big = 1 << 16                       # 2 * big * big > MSS_OBJ_MAX_PIXELS
    huge = lib.MSS_OBJ_MAX_PIXELS + 1
    bbox, resc = h.mss_obj_bbox_u8, h.mss_obj_rescale_f32
    got = {
        "bbox null mask": bbox(None, 100, X, 2, X, None),
        "bbox null jobs": bbox(X, 100, None, 2, X, None),
        "bbox null boxes": bbox(X, 100, X, 2, None, None),
        "bbox pixels=0": bbox(X, 0, X, 2, X, None),
        "bbox pixels=-1": bbox(X, -1, X, 2, X, None),
        "bbox n=0": bbox(X, 100, X, 0, X, None),
        "bbox n=-3": bbox(X, 100, X, -3, X, None),
        "bbox huge bank": bbox(X, huge, X, 2, X, None),
        "bbox too many jobs": bbox(X, 100, X, lib.MSS_OBJ_MAX_BBOX_JOBS + 1, X, None),
        "bbox null+huge": bbox(None, huge, X, 2, X, None),
        "bbox n=0+huge": bbox(X, huge, X, 0, X, None),
        "rescale null img": resc(None, X, 100, X, 2, 8, 8, X, X, None),
        "rescale null mask": resc(X, None, 100, X, 2, 8, 8, X, X, None),
        "rescale null jobs": resc(X, X, 100, None, 2, 8, 8, X, X, None),
        "rescale null out_img": resc(X, X, 100, X, 2, 8, 8, None, X, None),
        "rescale null out_mask": resc(X, X, 100, X, 2, 8, 8, X, None, None),
        "rescale pixels=0": resc(X, X, 0, X, 2, 8, 8, X, X, None),
        "rescale B=0": resc(X, X, 100, X, 0, 8, 8, X, X, None),
        "rescale B=-1": resc(X, X, 100, X, -1, 8, 8, X, X, None),
        "rescale OHmax=0": resc(X, X, 100, X, 2, 0, 8, X, X, None),
        "rescale OWmax=-2": resc(X, X, 100, X, 2, 8, -2, X, X, None),
        "rescale huge bank": resc(X, X, huge, X, 2, 8, 8, X, X, None),
        "rescale B=65536": resc(X, X, 100, X, lib.MSS_OBJ_MAX_BATCH + 1, 8, 8, X, X, None),
        "rescale too many rows": resc(X, X, 100, X, 1, lib.MSS_OBJ_MAX_ROWS + 1, 1, X, X, None),
        "rescale huge out": resc(X, X, 100, X, 2, big, big, X, X, None),
        "rescale one past the pixels": resc(X, X, 100, X, 1, 1 << 15, 1 << 16, X, X, None),
        "rescale null+huge": resc(None, X, 100, X, 2, big, big, X, X, None),
        "rescale OWmax=0+huge": resc(X, X, huge, X, 2, big, 0, X, X, None),
    }
    want = {k: BAD for k in got}
    for k in ("bbox huge bank", "bbox too many jobs", "rescale huge bank", "rescale B=65536", "rescale too many rows", "rescale huge out",
              "rescale one past the pixels"):
        want[k] = UNS
    assert got == want and OK_NEVER not in got.values()
