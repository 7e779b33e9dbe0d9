"""Test helper: hand every kernel wrapper dirty memory.

The package allocates its outputs and scratch with torch.empty / empty_like / new_empty and relies on one contract that is
written down only in comments: every element that is later read has been written first. Inputs built with randn / zeros
and a caching allocator full of finite garbage hide a broken contract (finite garbage times a zero weight is 0), so

    with poisoned(float("nan")):      # or poisoned(BIG)
        y = wrapper(...)

fills every CUDA floating-point tensor those three functions return with the poison value, and the uint8 buffers of the
split-bf16 weight-plane producers with 0xFF (a bf16 NaN in every plane). NaN catches a read that is multiplied by zero;
the large finite value catches a read that NaN slips through (fmaxf(NaN, 0) == 0: ReLU, max-pool, running maxima).

Integer and other byte buffers are never poisoned: their readers turn them into addresses, loop bounds and counts, where
a poison would fault the GPU instead of failing an assertion. Every such allocation site of the package is listed in
UNPOISONED; tests/test_poison_sites.py keeps that table complete, and poisoned() itself records any unlisted site that
hands out an unpoisoned CUDA buffer at run time (`ctx.unlisted`, asserted empty on exit).

Plain module, imported by the tests that want it; nothing loads it automatically. Build models, parameters and inputs
outside the context: only the call under test belongs inside it.
"""
import contextlib
import math
import sys

import torch

BIG = 1e30
POISONS = (float("nan"), BIG)

# functions whose uint8 allocations are split-bf16 weight planes (kernels.py): poisoned with 0xFF
PLANE_PRODUCERS = frozenset({"split_planes", "w_split_of", "fused_planes"})

# (module, function, variable, reason): the package's allocation sites that are NOT poisoned (integer / byte buffers)
UNPOISONED = (
    ("MultiScaleDeformableAttention", "ms_deform_attn_backward", "ws", "binned-backward byte workspace: counts and record offsets"),
    ("MultiScaleDeformableAttention", "ms_deform_attn_backward_proj", "ws", "binned-backward byte workspace: counts and record offsets"),
    ("datapath", "make_pair_batch", "out_tgt", "int64 targets: class ids the loss turns into indices"),
    ("loss", "_run_global", "kind", "uint8 pixel classes: select which index list a pixel joins"),
    ("loss", "_run_global", "hist", "int32 radix-select histogram"),
    ("loss", "_run_global", "eqs", "int32 tie counts gathered from every rank"),
    ("loss", "_run_global", "idx", "int32 pixel indices of the three compacted sets"),
    ("loss", "_run_global", "block_counts", "int32 per-block counts of the compaction"),
    ("loss", "_run_global", "all_n", "int32 set sizes gathered from every rank"),
    ("loss", "_run_local", "ws", "byte workspace of the one-call loss: counters, histograms, indices"),
    ("loss", "_run_local", "kind", "uint8 pixel classes: select which index list a pixel joins"),
    ("loss", "_run_local", "hist", "int32 radix-select histogram"),
    ("loss", "_run_local", "idx", "int32 pixel indices of the three compacted sets"),
    ("loss", "_run_local", "block_counts", "int32 per-block counts of the compaction"),
    ("loss", "_run_local", "n_out", "int32 set sizes: loop bounds of the pair kernels"),
    ("metric", "update", "keys", "int32 sort keys of the streamed maps"),
    ("metric", "_flush", "keys", "int32 sort keys of a group of maps"),
    ("metric", "_sorted", "out", "int32 sorted keys"),
    ("metric", "_sorted", "temp", "radix-sort byte temp space"),
    ("metric", "compute", "neg_in", "int32 per-bin counts"),
    ("metric", "compute", "pos_in", "int32 per-bin counts"),
    ("metric", "compute", "u2", "int64 rank sums"),
    ("kernels", "ood_score", "label", "uint8 argmax label map (written whole, an output not scratch)"),
)

_UNPOISONED_FUNCS = frozenset((m, f) for m, f, _, _ in UNPOISONED)
_PKG = "multishiftseg_amd."


def _site(frame):
    mod = frame.f_globals.get("__name__", "")
    return (mod[len(_PKG):] if mod.startswith(_PKG) else None), frame.f_code.co_name


class _Ctx:
    def __init__(self, value):
        self.value = value
        self.filled = 0
        self.unlisted = []          # (module, function, dtype) of unpoisoned package allocations missing from UNPOISONED


def _fill(ctx, t, frame):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.numel() == 0:
        return t
    mod, fn = _site(frame)
    if t.is_floating_point():
        t.fill_(ctx.value)
        ctx.filled += 1
    elif t.dtype == torch.uint8 and mod == "kernels" and fn in PLANE_PRODUCERS:
        t.fill_(0xFF)
        ctx.filled += 1
    elif mod is not None and (mod, fn) not in _UNPOISONED_FUNCS:
        ctx.unlisted.append((mod, fn, str(t.dtype)))
    return t


@contextlib.contextmanager
def poisoned(value):
    """Patch torch.empty, torch.empty_like and torch.Tensor.new_empty for the duration of the block (see the module
    docstring). Yields a context whose `filled` counts the poisoned buffers."""
    assert math.isnan(value) or abs(value) >= 1e20, "a poison must be NaN or large enough to show in any output"
    ctx = _Ctx(value)
    orig_empty, orig_like, orig_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*a, **k):
        return _fill(ctx, orig_empty(*a, **k), sys._getframe(1))

    def empty_like(*a, **k):
        return _fill(ctx, orig_like(*a, **k), sys._getframe(1))

    def new_empty(self, *a, **k):
        return _fill(ctx, orig_new(self, *a, **k), sys._getframe(1))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield ctx
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = orig_empty, orig_like, orig_new
    assert not ctx.unlisted, f"unpoisoned package allocations missing from tests/poison.py UNPOISONED: {sorted(set(ctx.unlisted))}"


def _flat(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    if out is None:
        return []
    raise TypeError(f"poison_runs: cannot compare a {type(out).__name__}")


def _host(out):
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in _flat(out)]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def poison_runs(fn, setup=None, bitwise=None, allow_nonfinite=False):
    """Run fn() twice clean, then once under each poison (setup() runs before every call, outside any poison). fn returns a
    tensor or a (nested) list / tuple / dict of tensors. Asserts that every poisoned output is finite (unless its clean run
    was not, where allow_nonfinite) and equal bit for bit to the clean run -- wherever the two clean runs agree bit for bit
    (bitwise=None), or always (bitwise=True). Returns {"clean": [...], "clean2": [...], nan: [...], BIG: [...]} of host
    tensors, so that the caller can hold every run to the family's float64 bound; the entry "reproducible" tells which
    outputs were compared bitwise."""
    runs = {}
    for tag in ("clean", "clean2"):
        if setup is not None:
            setup()
        runs[tag] = _host(fn())
    repro = [_same(a, b) for a, b in zip(runs["clean"], runs["clean2"])]
    if bitwise:
        assert all(repro), f"two clean runs differ in outputs {[i for i, r in enumerate(repro) if not r]}"
    for v in POISONS:
        if setup is not None:
            setup()
        with poisoned(v) as ctx:
            out = fn()
        runs[v] = got = _host(out)
        assert len(got) == len(runs["clean"])
        for i, (g, c) in enumerate(zip(got, runs["clean"])):
            if g.is_floating_point():
                fin_c = torch.isfinite(c)
                bad = ~torch.isfinite(g) & fin_c if allow_nonfinite else ~torch.isfinite(g)
                assert not bad.any(), f"output {i} under poison {v}: {int(bad.sum())} of {g.numel()} non-finite elements " \
                                      f"(first at {tuple(bad.nonzero()[0].tolist())})"
                big = (g.abs() > 1e25) & (c.abs() <= 1e25)
                assert not big.any(), f"output {i} under poison {v}: {int(big.sum())} elements carry the poison"
            if repro[i]:
                assert _same(g, c), f"output {i} under poison {v} differs from the clean run " \
                                    f"(max |diff| {float((g.double() - c.double()).abs().nan_to_num(0).max()) if g.is_floating_point() else 'n/a'})"
    runs["reproducible"] = repro
    return runs
