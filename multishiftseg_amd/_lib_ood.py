"""ctypes binding of libmss_ood.so (include/mss_ood_hip.h): the margin / bce pixel losses of SetCriterion.loss_ood.

A third table beside _lib.SIGNATURES (closed at the 142 entry points of libmss_hip.so) and _lib_aug.AUG_SIGNATURES (closed at 12).
Same rules: no CPU fallback, a missing library or a non-zero status raises.
"""
import ctypes
import os
from ctypes import c_float, c_int, c_longlong, c_void_p

import torch  # noqa: F401  (loads torch's HIP runtime first so that libmss_ood.so binds to the same one)

from ._lib import MSS_ERR_BAD_ARG, MSS_ERR_UNSUPPORTED, MssError, ptr, stream_ptr  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
OOD_LIB_PATH = os.path.join(_HERE, "libmss_ood.so")

MSS_OOD_ABI_VERSION = 1      # include/mss_ood_hip.h
MSS_OOD_MAX_CLASSES = 32
MSS_OOD_MAX_PIXELS = 0x7fffffff
KINDS = {"margin": 0, "bce": 1}          # MSS_OOD_MARGIN, MSS_OOD_BCE

P = c_void_p
I = c_int

# name -> argtypes, exactly the declarations of include/mss_ood_hip.h
OOD_SIGNATURES = {
    "mss_ood_abi_version": [],
    "mss_ood_loss_partials": [c_longlong],
    "mss_ood_negmax_f32": [P, I, I, I, I, P, P],
    "mss_ood_pixel_loss_f32": [P, P, I, I, I, I, I, I, c_float, P, P, P, P, P],
    "mss_ood_pixel_loss_backward_f32": [P, P, P, P, P, I, I, I, I, I, I, I, c_float, P, P],
}
OOD_VALUE_RESTYPE = {"mss_ood_abi_version": c_int, "mss_ood_loss_partials": c_int}

_lib = None


def load():
    """dlopen libmss_ood.so (once) and check that it exports every function of the header."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(OOD_LIB_PATH):
        raise MssError(
            f"{OOD_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C multishiftseg_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(OOD_LIB_PATH)
    for name, argtypes in OOD_SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = OOD_VALUE_RESTYPE.get(name, c_int)
    got = lib.mss_ood_abi_version()
    if got != MSS_OOD_ABI_VERSION:
        raise MssError(f"{OOD_LIB_PATH} has ABI version {got}, this package expects {MSS_OOD_ABI_VERSION}: rebuild it")
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
    assert name in OOD_VALUE_RESTYPE
    return getattr(load(), name)(*args)
