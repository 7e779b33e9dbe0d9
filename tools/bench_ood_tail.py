#!/usr/bin/env python3
"""The OOD-score tail (csrc/glue.hip, mss_ood_score_f32 / mss_ood_score_bwd_f32) on its two routes, in one process on one device:

    specialised   the <19> kernels (the default at 19 classes)
    generic       the class-generic kernels (every other class count; 19 too under MSS_OOD_TAIL_GENERIC=1)

at the bench shape: the fused-heads buffer of a 2 x 512 x 1024 half-resolution map (deepv3.heads_layout) to 2 x 1024 x 2048 outputs,
forward (score + NCHW logits, the training form) and backward (both gradients into the fused buffer). C = 19 on both routes,
C = 12 and 33 on the generic one. The rows of one class count are timed in alternation, WINDOWS windows of ITERS calls each between
two device events (the window ends in a synchronise), after a warm-up of every row; each row gives the median window and the spread.
TB/s is algorithmic bytes over that time:

    forward    read  2 heads x C x 4 B per source pixel         write (1 + C) x 4 B per output pixel
    backward   read  (1 + C) x 4 B per output pixel + C x 4 B per source pixel (dec2)      write Kh x 4 B per source pixel

At 19 the two routes' outputs are compared at this size before anything is timed. One JSON line per row.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multishiftseg_amd import _lib  # noqa: E402
from multishiftseg_amd.deepv3 import heads_layout  # noqa: E402
from multishiftseg_amd.kernels import Act  # noqa: E402

N, IH, IW, OH, OW = 2, 512, 1024, 1024, 2048
WINDOWS, ITERS, WARMUP = 7, 20, 5
SWITCH = "MSS_OOD_TAIL_GENERIC"


def set_route(generic):
    if generic:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    _lib.reset_env_cache()


def window(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_ood_tail: needs the GPU (a CPU run measures nothing)")
    for C, routes in ((19, ("specialised", "generic")), (12, ("generic",)), (33, ("generic",))):
        q, Kh = heads_layout(C)
        g = torch.Generator(device="cuda").manual_seed(C)
        dec = Act(torch.randn((N, IH, IW, Kh), generator=g, device="cuda") * 3)
        dec2, dec1 = dec.slice(q, C), dec.slice(0, C)
        score = torch.empty((N, OH, OW), device="cuda")
        logit = torch.empty((N, C, OH, OW), device="cuda")
        dscore = torch.randn((N, OH, OW), generator=g, device="cuda")
        dlogit = torch.randn((N, C, OH, OW), generator=g, device="cuda")
        dd = Act(torch.empty((N, IH, IW, Kh), device="cuda"))
        dd2, dd1 = dd.slice(q, C), dd.slice(0, C)

        def fwd():
            _lib.call("mss_ood_score_f32", dec2.ptr, dec2.ld, dec1.ptr, dec1.ld, N, IH, IW, C, OH, OW, _lib.ptr(score), _lib.ptr(logit), None)

        def bwd():
            _lib.call("mss_ood_score_bwd_f32", dec2.ptr, dec2.ld, _lib.ptr(dscore), _lib.ptr(dlogit), N, IH, IW, C, OH, OW, dd2.ptr, dd2.ld,
                      dd1.ptr, dd1.ld)
        outs = {}
        for r in routes:                               # every row once before any window; at 19 the two routes must agree
            set_route(r == "generic" and C == 19)
            for _ in range(WARMUP):
                fwd()
                bwd()
            torch.cuda.synchronize()
            outs[r] = (score.clone(), logit.clone(), dd.buf.clone())
        if len(routes) == 2:
            for a, b in zip(outs[routes[0]], outs[routes[1]]):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
        del outs
        src, out = N * IH * IW, N * OH * OW
        nbytes = {"forward": src * 2 * C * 4 + out * (1 + C) * 4, "backward": out * (1 + C) * 4 + src * C * 4 + src * Kh * 4}
        times = {(r, d): [] for r in routes for d in ("forward", "backward")}
        for _ in range(WINDOWS):
            for r in routes:
                set_route(r == "generic" and C == 19)
                times[(r, "forward")].append(window(fwd))
                times[(r, "backward")].append(window(bwd))
        set_route(False)
        for d in ("forward", "backward"):
            base = statistics.median(times[(routes[0], d)])
            for r in routes:
                ms = statistics.median(times[(r, d)])
                row = dict(kernel=d, route=r, C=C, Kh=Kh, shape=[N, IH, IW, OH, OW], ms=round(ms, 4), ms_min=round(min(times[(r, d)]), 4),
                           ms_max=round(max(times[(r, d)]), 4), alg_bytes=nbytes[d], TBs=round(nbytes[d] / ms / 1e9, 3))
                if len(routes) == 2:
                    row["ratio_vs_specialised"] = round(ms / base, 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
