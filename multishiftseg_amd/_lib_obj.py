"""ctypes binding of libmss_obj.so (include/mss_obj_hip.h): the resident COCO-object bank of the anomaly mix.

A fourth table beside _lib.SIGNATURES (closed at the 142 entry points of libmss_hip.so), _lib_aug.AUG_SIGNATURES (closed at 12) and
_lib_ood.OOD_SIGNATURES (closed at 5). Same rules: no CPU fallback, a missing library or a non-zero status raises.
"""
import ctypes
import os
from ctypes import c_int, c_longlong, c_void_p

import torch  # noqa: F401  (loads torch's HIP runtime first so that libmss_obj.so binds to the same one)

from ._lib import MSS_ERR_BAD_ARG, MSS_ERR_UNSUPPORTED, MssError, ptr, stream_ptr  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
OBJ_LIB_PATH = os.path.join(_HERE, "libmss_obj.so")

MSS_OBJ_ABI_VERSION = 1      # include/mss_obj_hip.h
MSS_OBJ_MAX_PIXELS = 0x7fffffff
MSS_OBJ_MAX_BBOX_JOBS = 0x1000000
MSS_OBJ_MAX_BATCH = 65535
MSS_OBJ_MAX_ROWS = 0xffff0
MSS_OBJ_BBOX_JOB_INTS = 5        # off, H, W, sh, sw
MSS_OBJ_RESCALE_JOB_INTS = 9     # off, H, W, sh, sw, y1, x1, bh, bw

P = c_void_p
I = c_int

# name -> argtypes, exactly the declarations of include/mss_obj_hip.h
OBJ_SIGNATURES = {
    "mss_obj_abi_version": [],
    "mss_obj_bbox_u8": [P, c_longlong, P, I, P, P],
    "mss_obj_rescale_f32": [P, P, c_longlong, P, I, I, I, P, P, P],
}
OBJ_VALUE_RESTYPE = {"mss_obj_abi_version": c_int}

_lib = None


def load():
    """dlopen libmss_obj.so (once) and check that it exports every function of the header."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(OBJ_LIB_PATH):
        raise MssError(
            f"{OBJ_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C multishiftseg_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(OBJ_LIB_PATH)
    for name, argtypes in OBJ_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = OBJ_VALUE_RESTYPE.get(name, c_int)
    got = lib.mss_obj_abi_version()
    if got != MSS_OBJ_ABI_VERSION:
        raise MssError(f"{OBJ_LIB_PATH} has ABI version {got}, this package expects {MSS_OBJ_ABI_VERSION}: rebuild it")
    _lib = lib
    return lib


_fns = {}


def call(name, *args):
    """Call a status-returning entry point on the current torch stream; raise on non-zero."""
    rc = status(name, *args)
    if rc != 0:
        kind = {MSS_ERR_BAD_ARG: "bad argument", MSS_ERR_UNSUPPORTED: "unsupported shape"}.get(rc, "hipError_t")
        raise MssError(f"{name} failed with code {rc} ({kind})")


def status(name, *args):
    """As call(), but hands the status code back instead of raising."""
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(load(), name)
    return fn(*args, stream_ptr())


def value(name, *args):
    assert name in OBJ_VALUE_RESTYPE
    return getattr(load(), name)(*args)
