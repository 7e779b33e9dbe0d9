"""Winograd-domain weight-gradient products of the 2x1024x2048 step in isolation (TFLOP/s of executed MFMA work).
--per-image: the three dilated ASPP branches' per-image products beside the dense product on the same operands, with
three Dropout2d masks -- (a) every image keeps exactly 1024 channels (L = 24 live c tiles, whole workgroups), (b) 1040 (L = 25: a
c tile with one 16-column step in it), (c) random, p = 0.5 -- and four job plans: the unpacked one (MSS_WGRAD_PERIMG_PACK=0), the
packed one without scratch (whole tiles), with scratch (the last round cut by rows). Launches alternate; one device-event pair each."""
import sys, os, json, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from multishiftseg_amd import kernels as K
from multishiftseg_amd._lib import MssConvArgs, call, ptr
from tools.microbench import timeit
# (P, T, C, K): ASPP dilation 12 / 24 through F(6x6), dilation 36 through F(4x4), the two decoder convolutions through F(6x6)
CASES = [(64, 2304, 4096, 256), (36, 5184, 4096, 256), (64, 29412, 256, 256), (64, 29412, 304, 256), (1, 162624, 256, 256), (1, 162624, 1024, 256), (1, 162624, 256, 1024),
         (1, 65536, 4096, 256)]


def per_image(launches=24):
    from multishiftseg_amd import _lib
    n, C0, C1, Ko = 2, 2048, 2048, 256
    C = C0 + C1
    g = torch.Generator(device="cuda").manual_seed(5)
    nb = _lib.MSS_WGRAD_PERIMG_TAIL_BYTES
    ws = torch.empty(nb // 4, device="cuda")
    for (P, Ti) in [(64, 1152), (36, 2592)]:                  # d = 12 / 24 through F(6x6), d = 36 through F(4x4)
        T = n * Ti
        dyt = torch.randn(P, T, Ko, device="cuda", generator=g)
        for name, kept in (("a: 1024 kept", 1024), ("b: 1040 kept", 1040), ("c: random p=0.5", None)):
            if kept is None:
                keep = torch.rand((n, C1), device="cuda", generator=g) >= 0.5
            else:
                keep = torch.zeros((n, C1), dtype=torch.bool, device="cuda")
                for i in range(n):
                    keep[i, torch.randperm(C1, device="cuda", generator=g)[:kept]] = True
            mask = keep.float() * 2.0
            _idx, count, k_steps, place, _col = K.chan_compact_index(mask, want_col=True)
            ks, pl = k_steps.cpu().tolist(), place.cpu()
            xt = torch.randn(P, T, C, device="cuda", generator=g)
            xc = torch.zeros(P, T, C, device="cuda")
            for i in range(n):
                rows = slice(i * Ti, (i + 1) * Ti)
                xt[:, rows, C0:] *= keep[i].float()[None, None, :]
                ext = 16 * ks[i]
                p_i = pl[i, :ext].cuda().long()
                for p0 in range(0, P, 8):                     # in pieces: the gather's temporaries
                    xc[p0:p0 + 8, rows, :C0] = xt[p0:p0 + 8, rows, :C0]
                    xc[p0:p0 + 8, rows, C0:C0 + ext] = xt[p0:p0 + 8, rows, C0:][:, :, p_i.clamp_min(0)] * (p_i >= 0).float()[None, None, :]

            def args(x, batch, rows):
                a = MssConvArgs()
                a.x = ptr(x)
                a.N, a.H, a.W, a.C, a.ldx = 1, 1, rows, C, C
                a.OH, a.OW, a.K, a.Kpad = 1, rows, Ko, Ko
                a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
                a.batch, a.x_bs, a.y_bs = batch, rows * C, rows * Ko
                return a
            a0 = args(xt, P, T)
            ws0, wsb0 = K._wgrad_workspace(a0, C, "cuda")
            a1 = args(xc, P * n, Ti)
            a1.k_steps, a1.k_base, a1.k_imgs = ptr(k_steps), C0 // 16, n
            du0 = torch.empty(P, Ko, C, device="cuda")
            du1 = torch.empty(P * n, Ko, C, device="cuda")

            def variant(env, w, wb):
                def run():
                    for k, v in env.items():
                        os.environ[k] = v
                    _lib.reset_env_cache()
                    call("mss_conv2d_wgrad_f32", ctypes.byref(a1), ptr(dyt), Ko, ptr(du1), C, w, wb)
                return run
            variants = {
                "dense": lambda: call("mss_conv2d_wgrad_f32", ctypes.byref(a0), ptr(dyt), Ko, ptr(du0), C, ptr(ws0), wsb0),
                "unpacked": variant({"MSS_WGRAD_PERIMG_PACK": "0"}, None, 0),
                "packed": variant({"MSS_WGRAD_PERIMG_PACK": "1"}, None, 0),
                "packed+tail": variant({"MSS_WGRAD_PERIMG_PACK": "1"}, ptr(ws), nb),
            }
            times = {k: [] for k in variants}
            for it in range(launches + 3):
                for k, fn in variants.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if it >= 3:
                        times[k].append(s.elapsed_time(e))
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            L = [min(C // 128, -(-(C0 + 16 * k) // 128)) for k in ks]
            print(json.dumps(dict(P=P, rows_per_image=Ti, mask=name, kept=count.cpu().tolist(), L=L, live_jobs=P * 2 * sum(L), launches=launches,
                                  median_ms={k: round(v, 3) for k, v in med.items()}, min_ms={k: round(min(v), 3) for k, v in times.items()},
                                  vs_dense={k: round(v / med["dense"], 3) for k, v in med.items()},
                                  tflops_executed={k: round(2.0 * P * Ti * Ko * (n * C if k == "dense" else sum(C0 + 16 * q for q in ks)) / v / 1e9, 1)
                                                   for k, v in med.items()})), flush=True)
            del xt, xc


if "--per-image" in sys.argv:
    per_image()
    sys.exit(0)

for (P, T, C, Ko) in CASES:
    xt = torch.randn(P, T, C, device="cuda")
    dyt = torch.randn(P, T, Ko, device="cuda")
    du = torch.empty(P, Ko, C, device="cuda")
    a = MssConvArgs()
    a.x = ptr(xt)
    a.N, a.H, a.W, a.C, a.ldx = 1, 1, T, C, C
    a.OH, a.OW, a.K, a.Kpad = 1, T, Ko, Ko
    a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
    if P > 1:
        a.batch, a.x_bs, a.y_bs = P, T * C, T * Ko
    ws, wsb = K._wgrad_workspace(a, C, "cuda")
    ms = timeit(lambda: call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), Ko, ptr(du), C, ptr(ws), wsb), iters=5, warm=2)
    print(json.dumps(dict(P=P, T=T, C=C, K=Ko, ms=round(ms, 3), tflops=round(2.0 * P * T * C * Ko / ms / 1e9, 1), ws_MB=round(wsb / 1e6, 1),
                          tn=os.environ.get("MSS_WGRAD_TN", "1"))), flush=True)
