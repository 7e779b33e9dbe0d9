"""ctypes binding of libmss_aug.so (include/mss_aug_hip.h): the Mask2Former input pipeline.

A second table beside _lib.SIGNATURES, which stays closed at the 142 entry points of libmss_hip.so. Same rules: no CPU
fallback, a missing library or a non-zero status raises.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_longlong, c_void_p

import torch  # noqa: F401  (loads torch's HIP runtime first so that libmss_aug.so binds to the same one)

from ._lib import MSS_ERR_BAD_ARG, MSS_ERR_UNSUPPORTED, MssError, ptr, stream_ptr  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
AUG_LIB_PATH = os.path.join(_HERE, "libmss_aug.so")

MSS_AUG_ABI_VERSION = 1      # include/mss_aug_hip.h
MSS_AUG_MAX_OPS = 8
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_AUTOCONTRAST = 1, 2, 3, 4, 5


class MssAugPointOps(Structure):
    """include/mss_aug_hip.h: a run of up to eight point-wise colour ops."""
    _fields_ = [("n", c_int), ("kind", c_int * MSS_AUG_MAX_OPS), ("factor", c_float * MSS_AUG_MAX_OPS)]


P = c_void_p
I = c_int

# name -> argtypes, exactly the declarations of include/mss_aug_hip.h
AUG_SIGNATURES = {
    "mss_aug_abi_version": [],
    "mss_aug_load_f32": [P, P, P, P, I, I, I, c_double, P, P, P],
    "mss_aug_stats_ws_doubles": [I, I],
    "mss_aug_stats_f32": [P, I, I, I, P, P, P],
    "mss_aug_pointwise_f32": [P, I, I, I, POINTER(MssAugPointOps), P, P],
    "mss_aug_blur9_f32": [P, P, I, I, I, P, P],
    "mss_aug_sharpness_f32": [P, P, I, I, I, c_float, P],
    "mss_aug_equalize_f32": [P, I, I, I, P, P],
    "mss_aug_resize_f32": [P, P, I, I, I, I, I, P, P, P],
    "mss_aug_rotate_f32": [P, P, I, I, I, c_float, c_float, P, P, P],
    "mss_aug_window_f32": [P, P, I, I, I, I, I, I, I, I, I, P, P, P],
    "mss_aug_finish_f32": [P, P, I, I, I, I, I, I, I, I, P, P, P, P, I, I, P, I, I, P, P, P],
}
AUG_VALUE_RESTYPE = {"mss_aug_abi_version": c_int, "mss_aug_stats_ws_doubles": c_longlong}

_lib = None


def load():
    """dlopen libmss_aug.so (once) and check that it exports every function of the header."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(AUG_LIB_PATH):
        raise MssError(
            f"{AUG_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C multishiftseg_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(AUG_LIB_PATH)
    for name, argtypes in AUG_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = AUG_VALUE_RESTYPE.get(name, c_int)
    got = lib.mss_aug_abi_version()
    if got != MSS_AUG_ABI_VERSION:
        raise MssError(f"{AUG_LIB_PATH} has ABI version {got}, this package expects {MSS_AUG_ABI_VERSION}: rebuild it")
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
    assert name in AUG_VALUE_RESTYPE
    return getattr(load(), name)(*args)
