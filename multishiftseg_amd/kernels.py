"""Thin tensor-level wrappers over the C ABI (include/mss_hip.h).

torch is used for device memory and streams only; every computation below is a HIP kernel in
libmss_hip.so. An activation is an `Act`: a channel slice [c0, c0+C) of a contiguous NHWC buffer,
so concats are written in place and never copied.
"""
import ctypes
import os

import torch

from . import _lib, aspp_plan
from ._lib import MssConvArgs, call, ptr
from .aspp_plan import WINOGRAD_MIN_CHANNELS, use_winograd, wino_tile     # noqa: F401  (the Winograd tile policy, host-only)


class Act:
    """Channel slice of an NHWC fp32 buffer [N,H,W,ld]. `stats`: per-channel partial sums [parts,2,C] left by the
    kernel that produced this slice (conv epilogue / Winograd output transform), consumed by bn_fold(train=True)."""
    __slots__ = ("buf", "N", "H", "W", "C", "ld", "c0", "stats")

    def __init__(self, buf, C=None, c0=0):
        assert buf.dim() == 4 and buf.is_contiguous() and buf.dtype == torch.float32
        self.buf = buf
        self.stats = None
        self.N, self.H, self.W, self.ld = buf.shape
        self.C = self.ld - c0 if C is None else C
        self.c0 = c0
        assert self.c0 % 4 == 0 and self.ld % 4 == 0 and self.c0 + self.C <= self.ld

    @staticmethod
    def empty(N, H, W, C, device, ld=None):
        return Act(torch.empty((N, H, W, ld or C), device=device, dtype=torch.float32), C)

    @staticmethod
    def zeros(N, H, W, C, device, ld=None):
        return Act(torch.zeros((N, H, W, ld or C), device=device, dtype=torch.float32), C)

    def slice(self, c0, C):
        return Act(self.buf, C, self.c0 + c0)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.c0)

    @property
    def M(self):
        return self.N * self.H * self.W

    def nchw(self):
        """Materialise as an NCHW torch tensor (tests / debugging only)."""
        return self.buf[..., self.c0:self.c0 + self.C].permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def from_nchw(t, ld=None):
        n, c, h, w = t.shape
        a = Act.zeros(n, h, w, c, t.device, ld)
        a.buf[..., :c] = t.permute(0, 2, 3, 1)
        return a


class PackedWeight:
    """[R*S][Kpad][Cp] layout consumed by the MFMA kernels. When the output-channel count leaves a
    narrow last 128-wide tile (e.g. 304 = 2*128 + 48, the data gradient of final.0), `tail` holds
    those channels as a separate pack that runs on the 64-wide tile instead of wasting 2/3 of a tile."""
    __slots__ = ("t", "K", "C", "R", "S", "Kpad", "Cp", "tail", "planes")

    def __init__(self, t, K, C, R, S, Kpad, Cp, tail=None):
        self.t, self.K, self.C, self.R, self.S, self.Kpad, self.Cp, self.tail = t, K, C, R, S, Kpad, Cp, tail
        self.planes = None         # split-bf16 form, made on first use under that route (w_split_of)


def _round_up(v, m):
    return (v + m - 1) // m * m


# ---- the split-bf16 GEMM route (csrc/gemm_bf16x3.hip) ---------------------------------------------------------------------------
# MSS_GEMM_SPLIT=1 (or set_gemm_route("bf16x3")): every product the persistent GEMM kernel takes runs as six bf16 MFMAs on operands
# split into three bf16 terms (fp32 accumulate, fp32 accuracy); the weights' planes are made once per packed weight.
_route_override = None


def set_gemm_route(route):
    """"native" (fp32 MFMA), "bf16x3" (split-bf16) or None (back to the MSS_GEMM_SPLIT environment switch)."""
    global _route_override
    assert route in (None, "native", "bf16x3")
    _route_override = route


def gemm_route():
    if _route_override is not None:
        return _route_override
    return "bf16x3" if os.environ.get("MSS_GEMM_SPLIT", "0") == "1" else "native"


def split_planes(t, Kpad, C):
    """The three-bf16-plane form (MssConvArgs.w_split) of packed fp32 weights t [batch][Kpad][C]; None where the route does not
    apply (Kpad not a multiple of 128: the <= 64-channel packs run on the native narrow tile)."""
    batch = t.numel() // (Kpad * C)
    nbytes = _lib.value("mss_gemm_split_weights_bytes", batch, Kpad, C)
    if nbytes <= 0:
        return None
    planes = torch.empty(nbytes, device=t.device, dtype=torch.uint8)
    call("mss_gemm_split_weights_bf16x3", ptr(t), ptr(planes), batch, Kpad, C, Kpad * C)
    return planes


def w_split_of(pw):
    """Pointer for MssConvArgs.w_split of a PackedWeight / WinoWeight under the current route (None: native). The planes are cached
    on the pack object, which is itself re-made whenever the parameter changes (_cached_pack)."""
    if gemm_route() != "bf16x3":
        return None
    if pw.planes is None:
        taps = getattr(pw, "R", 1) * getattr(pw, "S", 1)
        if taps != 1 and isinstance(pw, PackedWeight):
            # an implicit-GEMM layer: the taps folded into one long reduction (mss_conv_split_weights_bf16x3)
            nbytes = _lib.value("mss_gemm_split_weights_bytes", taps, pw.Kpad, pw.Cp)
            if nbytes > 0:
                pw.planes = torch.empty(nbytes, device=pw.t.device, dtype=torch.uint8)
                call("mss_conv_split_weights_bf16x3", ptr(pw.t), ptr(pw.planes), taps, pw.Kpad, pw.Cp)
        elif isinstance(pw, WinoWeight) and pw._t is None:
            pw.planes = pw.fused_planes()
            if pw.planes is None:
                pw.planes = split_planes(pw.t, pw.Kpad, pw.Cp)
        else:
            pw.planes = split_planes(pw.t, pw.Kpad, pw.Cp)
        if pw.planes is None:
            pw.planes = False
    return ptr(pw.planes) if pw.planes is not False else None


def pack_weight(w, flip=False, min_c=16):
    """nn.Conv2d.weight [K,C,R,S] -> PackedWeight. flip=True packs the data-gradient filter."""
    K, C, R, S = w.shape
    if w.dtype != torch.float32 or not w.is_cuda:
        raise TypeError(f"pack_weight needs a float32 CUDA tensor, got {w.dtype} on {w.device}")
    w = w.detach().contiguous()
    if not flip:
        k_out, c_in = K, C
    else:
        k_out, c_in = C, K
    rem = k_out % 128
    if k_out > 128 and 0 < rem <= 64:
        split = k_out - rem
        if not flip:
            main, tail = pack_weight(w[:split], flip, min_c), pack_weight(w[split:], flip, min_c)
        else:
            main, tail = pack_weight(w[:, :split], flip, min_c), pack_weight(w[:, split:], flip, min_c)
        main.tail = tail
        return main
    Kpad = _lib.value("mss_conv2d_kpad", k_out)
    Cp = _round_up(max(c_in, min_c), 16)
    t = torch.empty((R * S, Kpad, Cp), device=w.device, dtype=torch.float32)
    call("mss_conv2d_pack_weights_f32", ptr(w), ptr(t), K, C, R, S, Kpad, Cp, 1 if flip else 0, None, 0, 0)
    return PackedWeight(t, k_out, c_in, R, S, Kpad, Cp)


def _cached_pack(param, key, make):
    """Packed forms live on the parameter object itself and die with it. (A module-level dict keyed by
    id(param) can hand a new parameter the packed weights of a dead one when Python recycles the id and the
    allocator recycles the storage address -- same-shaped layers of two successive models.) Re-packed when the
    parameter is modified in place (optimizer step, load_state_dict: tensor._version) or moved (data_ptr)."""
    cache = param.__dict__.setdefault("_mss_packed", {})
    ent = cache.get(key)
    if ent is not None and ent[0] == param._version and ent[1] == param.data_ptr():
        return ent[2]
    val = make()
    cache[key] = (param._version, param.data_ptr(), val)
    return val


_ONES = {}


def ones(n, device):
    """A shared all-ones fp32 vector (the unit scale of a bias-only epilogue): one tensor per (length, device) for the life of the
    process instead of a fill kernel per Linear call."""
    key = (int(n), str(device))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(int(n), device=device, dtype=torch.float32)
    return t


_ZEROS = {}


def zeros(n, device):
    """The shared all-zeros counterpart of ones() (the zero shift of a scale-only prologue): a constant, never written."""
    key = (int(n), str(device))
    t = _ZEROS.get(key)
    if t is None:
        t = _ZEROS[key] = torch.zeros(int(n), device=device, dtype=torch.float32)
    return t


def packed(param, flip=False):
    """Cached pack_weight of an nn.Parameter."""
    return _cached_pack(param, ("direct", flip), lambda: pack_weight(param, flip))


class ConvProfile:
    """Optional live timing of every MFMA conv launch (bench.py's roofline leg): a pair of HIP events
    on the launch stream around each launch plus the launch's algorithmic FLOPs (dense 2*MAC)."""

    def __init__(self):
        self.records = []   # (kind, flops, start_event, stop_event)
        self.tags = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, flops, s, e in self.records:
            ms = s.elapsed_time(e)
            d = out.setdefault(kind, dict(launches=0, flops=0.0, ms=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += ms
        return out

    def per_launch(self):
        """[(kind, tag, ms, TFLOP/s)] in launch order (debugging aid: tools/layer_table.py)."""
        torch.cuda.synchronize()
        rows = []
        for (kind, flops, s, e), tag in zip(self.records, self.tags):
            ms = s.elapsed_time(e)
            rows.append((kind, tag, ms, flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0))
        return rows


_profile = None


def set_conv_profile(prof):
    global _profile
    _profile = prof


class _Timed:
    def __init__(self, kind, flops, tag=None):
        self.kind, self.flops, self.tag = kind, flops, tag

    def __enter__(self):
        if _profile is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if _profile is not None:
            self.e.record()
            _profile.records.append((self.kind, self.flops, self.s, self.e))
            _profile.tags.append(self.tag)
        return False


def _fwd_kind(a):
    """Profiling label of a forward launch: which of the two MFMA kernels the C side picks."""
    if _profile is None:
        return "conv_igemm"
    return ("conv_igemm", "gemm_nt", "gemm_few_rows", "gemm_nt_bf16x3", "conv_igemm_bf16x3", "conv_stem7", "conv_dgrad_s2")[_lib.value("mss_conv2d_forward_route", ctypes.byref(a))]


def _wgrad_kind(a, lddy):
    """Profiling label of a weight-gradient launch: the split-bf16 TN kernel or one of the native fp32 MFMA kernels."""
    if _profile is None or not a.route:
        return "conv_wgrad"
    return "conv_wgrad_bf16x3" if _lib.value("mss_conv2d_wgrad_route", ctypes.byref(a), lddy) else "conv_wgrad"


def conv_out_size(h, r, stride, dil, pad):
    return (h + 2 * pad - dil * (r - 1) - 1) // stride + 1


def _conv_args(x, pw, y, stride, dil, pad, in_affine, in_relu, out_affine, out_relu, res, res_mask=False, split=True):
    a = MssConvArgs()
    a.x, a.w, a.y = x.ptr, ptr(pw.t), (y.ptr if y is not None else None)
    a.w_split = w_split_of(pw) if split else None
    if in_affine is not None:
        sc, sh = in_affine
        a.in_scale, a.in_shift = ptr(sc), ptr(sh)
        a.in_ss_stride = sc.shape[1] if sc.dim() == 2 else 0
        assert sc.shape[-1] >= pw.Cp and sc.is_contiguous() and sh.is_contiguous()
    if out_affine is not None:
        a.out_scale, a.out_shift = ptr(out_affine[0]), ptr(out_affine[1])
    if res is not None:
        a.res, a.ldres = res.ptr, res.ld
        a.res_mask = int(res_mask)
    a.N, a.H, a.W, a.C, a.ldx = x.N, x.H, x.W, pw.Cp, x.ld
    a.R, a.S, a.stride, a.dil, a.pad = pw.R, pw.S, stride, dil, pad
    a.K, a.Kpad = pw.K, pw.Kpad
    a.in_relu, a.out_relu = int(in_relu), int(out_relu)
    return a


def conv2d(x, pw, stride=1, dil=1, pad=0, in_affine=None, in_relu=False, out_affine=None, out_relu=False, res=None,
           out=None, want_stats=False, res_mask=False):
    """y = epilogue(conv(prologue(x))). x: Act with C == pw.Cp channels visible. want_stats: the epilogue also leaves
    the per-channel partial sums of y on the returned Act (for the next layer's train-mode BatchNorm). res_mask: `res`
    gates the output (y = res > 0 ? y : 0, a ReLU backward) instead of being added."""
    assert x.C == pw.Cp or (x.C >= pw.C and x.C <= pw.Cp and x.c0 + pw.Cp <= x.ld), (x.C, pw.C, pw.Cp)
    OH = conv_out_size(x.H, pw.R, stride, dil, pad)
    OW = conv_out_size(x.W, pw.S, stride, dil, pad)
    k_total = pw.K + (pw.tail.K if pw.tail is not None else 0)
    if out is None:
        out = Act.empty(x.N, OH, OW, k_total, x.buf.device, ld=_round_up(k_total, 4))
    assert (out.N, out.H, out.W) == (x.N, OH, OW) and out.C >= k_total
    if pw.tail is not None:
        def sub(t, lo, n):
            return None if t is None else t[lo:lo + n]
        conv2d(x, pw.tail, stride, dil, pad, in_affine, in_relu,
               None if out_affine is None else (sub(out_affine[0], pw.K, pw.tail.K), sub(out_affine[1], pw.K, pw.tail.K)),
               out_relu, None if res is None else res.slice(pw.K, pw.tail.K), out=out.slice(pw.K, pw.tail.K), res_mask=res_mask)
        out_affine = None if out_affine is None else (sub(out_affine[0], 0, pw.K), sub(out_affine[1], 0, pw.K))
        res = None if res is None else res.slice(0, pw.K)
        out_main = out.slice(0, pw.K)
        _conv_launch(x, pw, out_main, OH, OW, stride, dil, pad, in_affine, in_relu, out_affine, out_relu, res, res_mask=res_mask)
        return out
    _conv_launch(x, pw, out, OH, OW, stride, dil, pad, in_affine, in_relu, out_affine, out_relu, res, want_stats, res_mask)
    return out


def _conv_launch(x, pw, out, OH, OW, stride, dil, pad, in_affine, in_relu, out_affine, out_relu, res, want_stats=False, res_mask=False):
    a = _conv_args(x, pw, out, stride, dil, pad, in_affine, in_relu, out_affine, out_relu, res, res_mask)
    a.OH, a.OW, a.ldy = OH, OW, out.ld
    out.stats = None
    if want_stats and out.C == pw.K:
        out.stats = torch.empty((-(-(x.N * OH * OW) // 64), 2, pw.K), device=x.buf.device, dtype=torch.float32)
        a.stats = ptr(out.stats)
    with _Timed(_fwd_kind(a), 2.0 * x.N * OH * OW * pw.K * pw.C * pw.R * pw.S,
                (x.N, x.H, x.W, pw.C, pw.K, pw.R, stride, dil)):
        call("mss_conv2d_forward_f32", ctypes.byref(a))


def conv2d_dgrad_s2(dz, pw_flipped, out_hw, in_affine=None, res=None, res_mask=False, out=None):
    """dx = epilogue(data gradient of a stride-2 convolution (3x3 / padding 1 or 1x1 / padding 0) at prologue(dz)): the gather-form
    kernel of csrc/conv_dgrad_s2.hip (MssConvArgs.stride == -2). dz: Act on the strided convolution's output grid with its output
    channels; pw_flipped: pack_weight(w, flip=True) / packed(w, flip=True); out_hw: (OH, OW) of dx -- the caller's, because the
    forward's floor loses a row or column. in_affine (one per-channel affine, in-grid rows only), res / res_mask and out as conv2d's.
    Native fp32 MFMA on either gemm route; every element of dx's channels is written."""
    pw = pw_flipped
    assert dz.C == pw.Cp or (dz.C >= pw.C and dz.C <= pw.Cp and dz.c0 + pw.Cp <= dz.ld), (dz.C, pw.C, pw.Cp)
    OH, OW = int(out_hw[0]), int(out_hw[1])
    k_total = pw.K + (pw.tail.K if pw.tail is not None else 0)
    if out is None:
        out = Act.empty(dz.N, OH, OW, k_total, dz.buf.device, ld=_round_up(k_total, 4))
    assert (out.N, out.H, out.W) == (dz.N, OH, OW) and out.C >= k_total
    parts = [(pw, 0)] if pw.tail is None else [(pw.tail, pw.K), (pw, 0)]
    for part, lo in parts:
        sub_out = out if pw.tail is None else out.slice(lo, part.K)
        sub_res = res if (res is None or pw.tail is None) else res.slice(lo, part.K)
        a = _conv_args(dz, part, sub_out, -2, 1, (part.R - 1) // 2, in_affine, False, None, False, sub_res, res_mask, split=False)
        a.OH, a.OW, a.ldy = OH, OW, sub_out.ld
        sub_out.stats = None
        with _Timed(_fwd_kind(a), 2.0 * dz.M * part.K * part.C * part.R * part.S, (dz.N, OH, OW, part.C, part.K, part.R, -2, 1)):
            call("mss_conv2d_forward_f32", ctypes.byref(a))
    return out


def dropout_compact_wanted(x, pw, in_affine, res=None):
    """True where a 1x1 product with a Dropout2d-folded per-sample prologue takes the channel-compacted form (conv2d_dropped): the
    library's gate -- MSS_DROPOUT_COMPACT (default 1), native route, per-sample affine + ReLU, 128-row tiles that cannot straddle
    images, more than 64 output channels. Everything else keeps the dense per-sample prologue."""
    if in_affine is None or in_affine[0].dim() != 2 or pw.tail is not None or x.ld != pw.Cp:
        return False
    a = _conv_args(x, pw, None, 1, 1, 0, in_affine, True, None, False, res)
    a.OH, a.OW = x.H, x.W
    return bool(_lib.value("mss_chan_compact_wanted", ctypes.byref(a)))


def chan_compact_index(mask, want_col=False):
    """mask [N][C] (device fp32, != 0: kept) -> (idx [N][C] int32: ascending kept channels in the first count[n] entries of row n,
    count [N], k_steps [N] = max(3, ceil(count / 16)), place [N][C]: the channel that goes to each column of the compacted rows
    or -1, in the order that makes the compacted product add its terms as the dense one does). One launch, nothing read back.
    want_col: a fifth answer, col [N][C] -- the inverse of place: the column each channel went to, -1 for a dropped one."""
    N, C = mask.shape
    assert mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous()
    # int32 contents in float allocations: of `idx` only the first count[n] entries of a row are ever written or read
    idx = torch.empty((N, C), device=mask.device, dtype=torch.float32).view(torch.int32)
    place = torch.empty((N, C), device=mask.device, dtype=torch.float32).view(torch.int32)
    meta = torch.empty((2, N), device=mask.device, dtype=torch.float32).view(torch.int32)
    col = torch.empty((N, C), device=mask.device, dtype=torch.float32).view(torch.int32) if want_col else None
    call("mss_chan_compact_index", ptr(mask), N, C, ptr(idx), ptr(place), ptr(meta[0]), ptr(meta[1]), ptr(col))
    return (idx, meta[0], meta[1], place, col) if want_col else (idx, meta[0], meta[1], place)


def conv2d_dropped(x, pw, mask, in_affine, res=None, want_stats=False, out_relu=False):
    """conv2d(x, pw, in_affine=(scale * mask, shift * mask) per sample, in_relu=True, res=res) with the products of the zeroed
    channels left out: sample n's kept channels (mask[n] != 0) are compacted to the front of its rows (prologue applied on the way)
    and of its own copy of the weights, and the GEMM kernel runs k_steps[n] K-steps on image n. The columns are ordered so that every
    output element adds the kept terms in the dense product's order: the result is bit-identical to the dense form. Chosen on the device, per call:
    no host synchronisation. in_affine: the mask-multiplied vectors the dense prologue would take."""
    sc, sh = in_affine
    N, C, dev = x.N, pw.Cp, x.buf.device
    assert tuple(mask.shape) == (N, C) and tuple(sc.shape) == (N, C) and pw.R * pw.S == 1 and pw.tail is None
    HW = x.H * x.W
    _idx, count, k_steps, place = chan_compact_index(mask)
    xc = Act.empty(N, x.H, x.W, C, dev, ld=x.ld)
    wc = torch.empty((N, pw.Kpad, C), device=dev, dtype=torch.float32)
    kept = float(count.sum().item()) if _profile is not None else 0.0       # profiling pass only: the EXECUTED work of this call
    with _Timed("chan_compact", 4.0 * HW * (N * C + kept), ("act", N, x.H, x.W, C)):                # "flops" = algorithmic BYTES
        call("mss_chan_compact_act_f32", x.ptr, x.ld, xc.ptr, xc.ld, N, HW, C, ptr(place), ptr(k_steps), ptr(sc), ptr(sh))
    with _Timed("chan_compact", 4.0 * pw.Kpad * (C + kept), ("weights", N, pw.Kpad, C)):
        call("mss_chan_compact_weights_f32", ptr(pw.t), ptr(wc), N, pw.Kpad, C, ptr(place), ptr(k_steps))
    out = Act.empty(N, x.H, x.W, pw.K, dev, ld=_round_up(pw.K, 4))
    a = _conv_args(xc, pw, out, 1, 1, 0, None, False, None, out_relu, res)
    a.w, a.w_split = ptr(wc), None
    a.k_steps, a.w_img_stride = ptr(k_steps), pw.Kpad * C
    a.OH, a.OW, a.ldy = x.H, x.W, out.ld
    if want_stats:
        out.stats = torch.empty((-(-(N * HW) // 64), 2, pw.K), device=dev, dtype=torch.float32)
        a.stats = ptr(out.stats)
    with _Timed(_fwd_kind(a), 2.0 * HW * pw.K * kept, (N, x.H, x.W, int(kept / N), pw.K, 1, 1, 1)):
        call("mss_conv2d_forward_f32", ctypes.byref(a))
    return out


def _wgrad_workspace(a, Cp, device):
    """Scratch for the partial slabs of a pixel-split weight gradient (deterministic two-stage sum)."""
    nbytes = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), Cp)
    if nbytes <= 0:
        return None, 0
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32), nbytes


def conv2d_wgrad(x, dy, K, C, R, S, stride=1, dil=1, pad=0, in_affine=None, in_relu=False):
    """Weight gradient [K,C,R,S] of y = conv(prologue(x)); dy: Act with K channels."""
    Kpad = _round_up(K, 4)
    Cp = _round_up(C, 4)
    dwp = torch.empty((R * S, Kpad, Cp), device=x.buf.device, dtype=torch.float32)   # fully overwritten by the kernel
    a = MssConvArgs()
    a.x = x.ptr
    if in_affine is not None:
        sc, sh = in_affine
        a.in_scale, a.in_shift = ptr(sc), ptr(sh)
        a.in_ss_stride = sc.shape[1] if sc.dim() == 2 else 0
    a.N, a.H, a.W, a.C, a.ldx = x.N, x.H, x.W, C, x.ld
    a.OH, a.OW, a.K, a.Kpad = dy.H, dy.W, K, Kpad
    a.R, a.S, a.stride, a.dil, a.pad = R, S, stride, dil, pad
    a.in_relu = int(in_relu)
    a.route = 1 if gemm_route() == "bf16x3" else 0
    ws, ws_bytes = _wgrad_workspace(a, Cp, x.buf.device)
    with _Timed(_wgrad_kind(a, dy.ld), 2.0 * x.N * dy.H * dy.W * K * C * R * S, (x.N, x.H, x.W, C, K, R, stride, dil)):
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), dy.ptr, dy.ld, ptr(dwp), Cp, ptr(ws), ws_bytes)
    grad = torch.empty((K, C, R, S), device=x.buf.device, dtype=torch.float32)
    call("mss_conv2d_unpack_wgrad_f32", ptr(dwp), ptr(grad), K, C, R, S, Kpad, Cp, 0, None, None, 0, 0)
    return grad


class WinoWeight:
    """Winograd-domain filter U [(tile+2)^2][Kpad][Cp] of a 3x3 weight. `src` (optional): the contiguous [K][C][3][3] weight it comes
    from; with it `t` may start as None and is made on first use -- the split-bf16 route fills its planes straight from `src`
    (w_split_of -> mss_wino_pack_split_bf16x3) and never reads U in fp32 unless the layer has a narrow native tail."""
    __slots__ = ("_t", "src", "K", "C", "Kpad", "Cp", "tile", "planes", "_src_version")

    def __init__(self, t, K, C, Kpad, Cp, tile, src=None):
        assert t is not None or src is not None
        self._t, self.src, self.K, self.C, self.Kpad, self.Cp, self.tile = t, src, K, C, Kpad, Cp, tile
        self.planes = None
        # `src` may alias the live parameter (detach().contiguous() copies nothing): a lazily made U / planes must come from the SAME
        # weight version as whatever was made first, or one convolution would mix two versions. detach() shares the
        # version counter, so an in-place update of the parameter (optimizer.step) shows here.
        self._src_version = None if src is None else src._version

    def _check_fresh(self):
        if self.src is not None and self.src._version != self._src_version:
            raise RuntimeError("stale WinoWeight: the weight it was packed from has been modified in place since (version "
                               f"{self._src_version} -> {self.src._version}); re-pack it (kernels.packed_wino does, through tensor._version)")

    @property
    def t(self):
        if self._t is None:
            self._check_fresh()
            t = torch.empty(((self.tile + 2) ** 2, self.Kpad, self.Cp), device=self.src.device, dtype=torch.float32)
            call("mss_wino_pack_weights_f32", ptr(self.src), ptr(t), self.K, self.C, self.Kpad, self.Cp, self.tile)
            self._t = t
        return self._t

    def fused_planes(self):
        """The split-bf16 planes of U straight from `src` (bit-identical to split_planes(self.t, ...)), or None where that form does
        not apply (no source weight, a padded Cp, Kpad not a multiple of 128)."""
        if self.src is None or self.Cp != self.C or self.Kpad % 128 or self.C % 16 or self.src.data_ptr() % 16:
            return None
        self._check_fresh()
        nbytes = _lib.value("mss_gemm_split_weights_bytes", (self.tile + 2) ** 2, self.Kpad, self.C)
        if nbytes <= 0:
            return None
        planes = torch.empty(nbytes, device=self.src.device, dtype=torch.uint8)
        call("mss_wino_pack_split_bf16x3", ptr(self.src), ptr(planes), self.K, self.C, self.Kpad, self.tile)
        return planes


def pack_weight_wino(w, flip=False, tile=2):
    """flip=True: the data-gradient filter (K<->C swapped, taps rotated 180 degrees), as pack_weight."""
    if flip:
        w = w.detach().flip(2, 3).transpose(0, 1)
    K, C, R, S = w.shape
    assert R == 3 and S == 3 and C % 16 == 0 and K % 4 == 0 and tile in (2, 4, 6)
    if w.dtype != torch.float32 or not w.is_cuda:
        raise TypeError("pack_weight_wino needs a float32 CUDA tensor")
    w = w.detach().contiguous()
    Kpad = _lib.value("mss_conv2d_kpad", K)
    if gemm_route() == "bf16x3" and Kpad % 128 == 0:
        return WinoWeight(None, K, C, Kpad, C, tile, src=w)          # U in fp32 only if somebody asks for it (WinoWeight.t)
    t = torch.empty(((tile + 2) ** 2, Kpad, C), device=w.device, dtype=torch.float32)
    call("mss_wino_pack_weights_f32", ptr(w), ptr(t), K, C, Kpad, C, tile)
    return WinoWeight(t, K, C, Kpad, C, tile)


def packed_wino(param, flip=False, tile=2):
    return _cached_pack(param, ("wino", flip, tile), lambda: pack_weight_wino(param, flip, tile))


WINO_TILE_OF_P = {16: 2, 36: 4, 64: 6}


def wino_xt_bytes(N, H, W, C, dil):
    """Size of the Winograd-domain input X' of one layer under the tile policy."""
    ts = wino_tile(H, W, dil)
    return (ts + 2) ** 2 * _lib.value("mss_wino_num_tiles", N, H, W, dil, ts) * C * 4


_tile_hook = None


def set_tile_hook(fn):
    """Attribution / test hook (tools/attribute_wino_error.py): fn(info) is asked once per forward 3x3 layer with
    info = dict(H, W, dil, c_in, k_out, stride, policy_tile) and answers None (keep the policy), 0 (direct implicit
    GEMM) or a tile edge 2 / 4 / 6. Not consulted for data or weight gradients."""
    global _tile_hook
    _tile_hook = fn


def conv3x3(x, weight, dil=1, stride=1, in_affine=None, in_relu=False, res=None, out=None, flip=False, keep_xt=None,
            want_stats=False, max_tile=6, xt=None):
    """3x3 convolution with padding = dilation on nn.Conv2d-layout `weight` (flip=True: its data gradient),
    through Winograd when the policy says so, else through the direct implicit GEMM. max_tile: accuracy cap on the
    Winograd tile edge for this layer (0: no Winograd at all). xt: the layer's Winograd-domain input X' when the caller has
    it already (aspp_transforms); its tile edge decides the route."""
    k_out, c_in = (weight.shape[1], weight.shape[0]) if flip else (weight.shape[0], weight.shape[1])
    if xt is not None:
        assert in_affine is None and not in_relu and not flip and stride == 1
        return conv2d_winograd(x, packed_wino(weight, False, WINO_TILE_OF_P[xt.shape[0]]), dil=dil, res=res, out=out,
                               keep_xt=keep_xt, want_stats=want_stats, xt=xt)
    tile = wino_tile(x.H, x.W, dil, max_tile) if max_tile else 0
    if _tile_hook is not None and not flip:
        forced = _tile_hook(dict(H=x.H, W=x.W, dil=dil, c_in=c_in, k_out=k_out, stride=stride, policy_tile=tile))
        if forced == 0:
            return conv2d(x, packed(weight, flip), stride=stride, dil=dil, pad=dil, in_affine=in_affine, in_relu=in_relu,
                          res=res, out=out, want_stats=want_stats)
        if forced:
            tile = forced
    if tile and use_winograd(c_in, k_out, stride, in_affine, tile):
        return conv2d_winograd(x, packed_wino(weight, flip, tile), dil=dil, in_affine=in_affine,
                               in_relu=in_relu, res=res, out=out, keep_xt=keep_xt, want_stats=want_stats)
    return conv2d(x, packed(weight, flip), stride=stride, dil=dil, pad=dil, in_affine=in_affine, in_relu=in_relu, res=res,
                  out=out, want_stats=want_stats)


def conv2d_winograd(x, ww, dil=1, in_affine=None, in_relu=False, res=None, out=None, keep_xt=None, want_stats=False, xt=None):
    """3x3 / stride 1 / padding = dilation convolution through Winograd F(m x m,3x3), m = ww.tile: input
    transform (with the fused BatchNorm+ReLU prologue) -> (m+2)^2 batched MFMA GEMMs -> output transform
    (+ residual). keep_xt: a dict; the transformed input X' is stored under keep_xt["xt"] so that the weight
    gradient of the same layer (conv2d_wgrad_winograd(..., xt=...)) does not have to transform x again."""
    assert x.C == ww.C
    N, H, W, C, K, ts = x.N, x.H, x.W, ww.C, ww.K, ww.tile
    P = (ts + 2) ** 2
    dev = x.buf.device
    T = _lib.value("mss_wino_num_tiles", N, H, W, dil, ts)
    with _Timed("conv_winograd", 2.0 * N * H * W * K * C * 9, (N, H, W, C, K, 3, 1, dil)):
        if xt is None:
            xt = torch.empty((P, T, C), device=dev, dtype=torch.float32)
            sc, sh = in_affine if in_affine is not None else (None, None)
            assert sc is None or sc.dim() == 1
            with _Timed("wino_transform", 4.0 * (N * H * W * C + P * T * C), ("input", N, H, W, C, dil, ts)):   # "flops" = algorithmic BYTES
                call("mss_wino_input_transform_f32", x.ptr, x.ld, N, H, W, C, dil, ts, ptr(sc), ptr(sh), int(in_relu), ptr(xt))
        else:
            assert tuple(xt.shape) == (P, T, C) and in_affine is None and not in_relu
        return _wino_gemm_and_output(xt, ww, N, H, W, dil, res, out, keep_xt, want_stats)


def _set_wino_w(a, ww):
    """MssConvArgs.w of a Winograd-domain product. On the split-bf16 route the kernel reads only the planes (a.w_split): when U has not
    been made in fp32 (WinoWeight._t is None) and the library confirms that exactly these arguments take the split GEMM, U stays
    unmade and `w` carries the planes' address as a non-null stand-in; in every other case it is U (made on demand)."""
    if ww._t is None and a.w_split is not None:
        a.w = a.w_split
        if _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) == 3:
            return
    a.w = ptr(ww.t)


def _wino_args(xt, T, C, K, Kpad, batch, dropped=None):
    """What the MssConvArgs of every Winograd-domain batched product share, forward and weight gradient: `batch` 1x1 products over T
    rows of X' [batch][T][C]. dropped (an AsppDropped): the batch entries are (position, image), T one image's rows, and image n
    multiplies its first C0 + 16 k_steps[n] columns only."""
    a = MssConvArgs()
    a.x = ptr(xt)
    a.N, a.H, a.W, a.C, a.ldx = 1, 1, T, C, C
    a.OH, a.OW, a.K, a.Kpad = 1, T, K, Kpad
    a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
    a.batch, a.x_bs, a.y_bs = batch, T * C, T * K
    if dropped is not None:
        a.k_steps, a.k_base, a.k_imgs = ptr(dropped.k_steps), dropped.C0 // 16, dropped.N
    return a


def _wino_product(xt, ww, dropped=None):
    """Step 2 of the Winograd convolution on a transformed input X' [P][T][C] (2P positions for a packed_wino_pair): the batched MFMA
    products, Y' [P][T][K]. dropped (an AsppDropped; ww then holds one U per image, [P][N][Kpad][C]): _wino_args' per-image form."""
    C, K = ww.C, ww.K
    P, T = xt.shape[0], xt.shape[1]
    yt = torch.empty((P, T, K), device=xt.device, dtype=torch.float32)
    rem = K % 128
    split = K - rem if (K > 128 and 0 < rem <= 64) else 0     # e.g. 304 = 256 + 48: narrow tail on the 64-wide tile
    if dropped is None:
        a = _wino_args(xt, T, C, K, ww.Kpad, P)
        a.w_split = w_split_of(ww)
        executed, cols = float(T) * C, C
    else:
        N = dropped.N
        assert not split and T % N == 0 and ww.Kpad == K
        a = _wino_args(xt, T // N, C, K, ww.Kpad, P * N, dropped)
        executed, cols = float(T // N) * dropped.columns(), int(dropped.columns() / N)
    a.y, a.ldy, a.w_bs = ptr(yt), K, ww.Kpad * ww.Cp
    if split:
        a.K = split
    _set_wino_w(a, ww)
    # (bench.py unpacks this tag as eight numbers; the dropped form reports the mean number of columns an image's rows hold)
    with _Timed(_fwd_kind(a), 2.0 * P * executed * K, (P, 1, T, cols, K, 1, 1, 1)):   # the MFMA work actually executed
        call("mss_conv2d_forward_f32", ctypes.byref(a))
        if split:
            a.K, a.Kpad = rem, ww.Kpad - split
            a.w_split = None                                  # the <= 64-channel tail runs on the native narrow tile
            a.w = ctypes.c_void_p(ww.t.data_ptr() + 4 * split * ww.Cp)
            a.y = ctypes.c_void_p(yt.data_ptr() + 4 * split)
            call("mss_conv2d_forward_f32", ctypes.byref(a))
    return yt


def _wino_output(yt, N, H, W, K, dil, ts, res, out, want_stats):
    """Step 3: the output transform of Y' [P][T][K] into `out` (+ residual, + BatchNorm partial sums left on out.stats)."""
    out.stats = None
    if want_stats and out.C == K:
        out.stats = torch.empty((_lib.value("mss_wino_output_stats_parts", N, H, W, K, dil, ts), 2, K), device=yt.device,
                                dtype=torch.float32)
    with _Timed("wino_transform", 4.0 * (yt.numel() + N * H * W * K * (2 if res is not None else 1)), ("output", N, H, W, K, dil, ts)):
        call("mss_wino_output_transform_f32", ptr(yt), N, H, W, K, dil, ts, res.ptr if res is not None else None,
             res.ld if res is not None else 0, out.ptr, out.ld, ptr(out.stats))
    return out


def _wino_gemm_and_output(xt, ww, N, H, W, dil, res, out, keep_xt, want_stats, dropped=None):
    """Steps 2 and 3 of the Winograd convolution on a transformed input X' [P][T][C] (_wino_product, _wino_output)."""
    if out is None:
        # pixel rows on 128-byte lines: a 304-channel map (the decoder's first data gradient) with ld = 304 shares every other
        # cache line between two pixels that different waves write (0.99 -> 0.94 ms at 2 x 512 x 1024, tools/bench_wino_r04.py)
        out = Act.empty(N, H, W, ww.K, xt.device, ld=_round_up(ww.K, 32) if ww.K % 32 else None)
    yt = _wino_product(xt, ww, dropped)
    if keep_xt is not None:
        keep_xt["xt"] = xt
    del xt
    return _wino_output(yt, N, H, W, ww.K, dil, ww.tile, res, out, want_stats)


def packed_wino_pair(p1, p2, tile):
    """The Winograd-domain forms of two same-shaped 3x3 weights in ONE buffer [2P][Kpad][C] (P = (tile+2)^2), for
    conv3x3_pair. Cached on p1 until either parameter changes; the halves are also installed as the two parameters' own
    packed forms (views of the buffer), so the single-layer path does not keep a second copy."""
    key = (p1._version, p1.data_ptr(), p2._version, p2.data_ptr())
    cache = p1.__dict__.setdefault("_mss_packed", {})
    ent = cache.get(("wino_pair", tile))
    if ent is not None and ent[0] == key:
        return ent[1]
    assert p1.shape == p2.shape and p1.shape[2:] == (3, 3)
    K, C = p1.shape[0], p1.shape[1]
    P = (tile + 2) ** 2
    Kpad = _lib.value("mss_conv2d_kpad", K)
    t = torch.empty((2 * P, Kpad, C), device=p1.device, dtype=torch.float32)
    for j, p in enumerate((p1, p2)):
        w = p.detach().contiguous()
        call("mss_wino_pack_weights_f32", ptr(w), ptr(t[j * P:(j + 1) * P]), K, C, Kpad, C, tile)
        p.__dict__.setdefault("_mss_packed", {})[("wino", False, tile)] = (p._version, p.data_ptr(), WinoWeight(t[j * P:(j + 1) * P], K, C, Kpad, C, tile))
    ww = WinoWeight(t, K, C, Kpad, C, tile)
    cache[("wino_pair", tile)] = (key, ww)
    return ww


def conv3x3_pair_tile(x, w1, w2, dil1, dil2):
    """aspp_plan.pair_tile for two weights on the map x: the tile edge when the two layers share one product launch, else 0."""
    return aspp_plan.pair_tile(x.N, x.H, x.W, w1.shape, w2.shape, dil1, dil2, _tile_hook is not None)


def conv3x3_pair(x, w1, w2, dil1, dil2, out1, out2, tile, want_stats=False, xt=None):
    """conv3x3(x, w1, dil1) -> out1 and conv3x3(x, w2, dil2) -> out2 with the 2 x (tile+2)^2 Winograd-domain products in ONE
    gemm_nt launch (see conv3x3_pair_tile). Same transforms, same products, same results as the two separate calls."""
    ww = packed_wino_pair(w1, w2, tile)
    N, H, W, C, Ko = x.N, x.H, x.W, ww.C, ww.K
    P = (tile + 2) ** 2
    T = _lib.value("mss_wino_num_tiles", N, H, W, dil1, tile)
    with _Timed("conv_winograd", 2 * 2.0 * N * H * W * Ko * C * 9, (N, H, W, C, 2 * Ko, 3, 1, (dil1, dil2))):
        if xt is None:
            xt = torch.empty((2 * P, T, C), device=x.buf.device, dtype=torch.float32)
            for j, d in enumerate((dil1, dil2)):
                with _Timed("wino_transform", 4.0 * (N * H * W * C + P * T * C), ("input", N, H, W, C, d, tile)):
                    call("mss_wino_input_transform_f32", x.ptr, x.ld, N, H, W, C, d, tile, None, None, 0, ptr(xt[j * P:(j + 1) * P]))
        else:
            assert tuple(xt.shape) == (2 * P, T, C)
        assert Ko % 128 == 0                      # (conv3x3_pair_tile's rule: no narrow tail, so ONE launch)
        yt = _wino_product(xt, ww)
        del xt
        for j, (d, out) in enumerate(((dil1, out1), (dil2, out2))):
            _wino_output(yt[j * P:(j + 1) * P], N, H, W, Ko, d, tile, None, out, want_stats)
    return out1, out2


class FactoredAct:
    """The trunk's 4096-channel output x = Wproj . u + W3 . v that the composed ASPP route never forms (deepv3._aspp_composed): its
    two factors u = relu(a0 * aff0) and v = relu(a1 * aff1) (aff1 per sample under Dropout2d), which stand for the map
    w = [u ; v] of C = a0.C + a1.C channels. Has the shape attributes of an Act so that the Winograd wrappers, which only read x's
    shape once they are handed X', take it in x's place."""
    __slots__ = ("a0", "aff0", "a1", "aff1", "mask", "N", "H", "W", "C", "buf")

    def __init__(self, a0, aff0, a1, aff1, mask=None):
        assert (a0.N, a0.H, a0.W) == (a1.N, a1.H, a1.W)
        self.a0, self.aff0, self.a1, self.aff1 = a0, aff0, a1, aff1
        self.mask = mask           # the Dropout2d mask [N, a1.C] folded into aff1 (train mode), or None: what aspp_dropped reads
        self.N, self.H, self.W, self.C, self.buf = a0.N, a0.H, a0.W, a0.C + a1.C, a0.buf

    def materialise(self):
        """w as an Act (mss_affine_relu_nhwc_f32 per source; a per-sample affine image by image): the second formulation of the
        two-source transform, and what a route that needs the map itself reads."""
        w = Act.empty(self.N, self.H, self.W, self.C, self.buf.device)
        c0 = 0
        for a, (sc, sh) in ((self.a0, self.aff0), (self.a1, self.aff1)):
            dst = w.slice(c0, a.C)
            if sc.dim() == 1:
                call("mss_affine_relu_nhwc_f32", a.ptr, a.ld, dst.ptr, dst.ld, a.M, a.C, ptr(sc), ptr(sh), 1)
            else:
                hw = a.H * a.W
                for n in range(a.N):
                    call("mss_affine_relu_nhwc_f32", ctypes.c_void_p(a.ptr.value + 4 * n * hw * a.ld), a.ld,
                         ctypes.c_void_p(dst.ptr.value + 4 * n * hw * dst.ld), dst.ld, hw, a.C, ptr(sc[n]), ptr(sh[n]), 1)
            c0 += a.C
        return w


def aspp_compose_wanted():
    """aspp_plan.compose_wanted under the current tile hook: the switch of the composed ASPP route."""
    return aspp_plan.compose_wanted(_tile_hook is not None)


def aspp_tiles(H, W, C, rates, weights):
    """aspp_plan.tiles for three weights under the current tile hook: the tile edges where the single-read transforms apply, or None."""
    return aspp_plan.tiles(H, W, C, rates, [w.shape for w in weights], _tile_hook is not None)


def _factored_facts(x):
    """What aspp_plan wants to know of a FactoredAct (nothing of an Act)."""
    if not isinstance(x, FactoredAct):
        return {}
    return dict(factored=True, c0=x.a0.C, aff_dims=(x.aff0[0].dim(), x.aff1[0].dim()),
                mask=x.mask is not None and tuple(x.mask.shape) == (x.N, x.a1.C))


def aspp_dropped_wanted(fx, weights):
    """aspp_plan.dropped_wanted for a FactoredAct and the three dilated branches' weights under the current GEMM route."""
    f = _factored_facts(fx)
    return bool(f) and aspp_plan.dropped_wanted(gemm_route(), f["c0"], fx.a1.C, f["aff_dims"], f["mask"], [w.shape for w in weights])


def aspp_plan_for(x, rates, weights, keep=False, wgrad=(False, False, False), budget=aspp_plan.XT_BUDGET_BYTES):
    """The aspp_plan.AsppPlan of one head forward on the map x (an Act or a FactoredAct) with the three dilated branches' weights:
    the facts of x, the GEMM route and the tile hook, read here once."""
    return aspp_plan.plan(x.N, x.H, x.W, x.C, [w.shape for w in weights], rates, keep=keep, wgrad=wgrad, route=gemm_route(),
                          hook=_tile_hook is not None, budget=budget, **_factored_facts(x))


class AsppDropped:
    """One step's channel compaction of a FactoredAct's second factor v (its Dropout2d mask): what the three dilated ASPP products,
    their weight gradients and the transform between them share. place / col / k_steps as chan_compact_index gives them (all on the
    device: nothing is read back); xc: v with its prologue applied, channel-compacted per image (mss_chan_compact_act_f32)."""
    __slots__ = ("N", "C0", "C1", "place", "col", "count", "k_steps", "xc")

    def __init__(self, fx):
        a1 = fx.a1
        sc, sh = fx.aff1
        self.N, self.C0, self.C1 = fx.N, fx.a0.C, a1.C
        _idx, self.count, self.k_steps, self.place, self.col = chan_compact_index(fx.mask, want_col=True)
        self.xc = Act.empty(a1.N, a1.H, a1.W, a1.C, a1.buf.device)
        hw = a1.H * a1.W
        kept = float(self.count.sum().item()) if _profile is not None else 0.0
        with _Timed("chan_compact", 4.0 * hw * (self.N * self.C1 + kept), ("act", self.N, a1.H, a1.W, self.C1)):
            call("mss_chan_compact_act_f32", a1.ptr, a1.ld, self.xc.ptr, self.xc.ld, self.N, hw, self.C1, ptr(self.place), ptr(self.k_steps),
                 ptr(sc), ptr(sh))

    def columns(self):
        """Sum over the images of the columns their rows hold (profiling pass only: reads the counts back; else the dense number)."""
        if _profile is None:
            return float(self.N * (self.C0 + self.C1))
        return float(self.N * self.C0 + 16 * int(self.k_steps.sum().item()))


class AsppXt:
    """The Winograd-domain inputs of the three dilated ASPP branches: xts, the three X' [P][T][C]; both, the ONE [2P][T][C] buffer
    the first two are the halves of when the plan pairs their products (kernels.conv3x3_pair), else None. A branch takes its X':
    the layer owns it then (kept for the weight gradient, or freed)."""
    __slots__ = ("xts", "both")

    def __init__(self, plan, C, dev):
        def empty(m, n=1):
            return torch.empty((n * plan.Ps[m], plan.Ts[m], C), device=dev, dtype=torch.float32)
        self.both = empty(0, 2) if plan.pair_tile else None
        assert self.both is None or (plan.Ts[0] == plan.Ts[1] and plan.tiles[0] == plan.tiles[1] == plan.pair_tile)
        self.xts = ([self.both[:plan.Ps[0]], self.both[plan.Ps[0]:]] if plan.pair_tile else [empty(0), empty(1)]) + [empty(2)]

    def take_pair(self):
        both, self.both, self.xts[0], self.xts[1] = self.both, None, None, None
        return both

    def take(self, m):
        xt, self.xts[m] = self.xts[m], None
        return xt


def aspp_transforms(x, rates, plan, dropped=None):
    """(AsppXt, gap): X' of the ONE map `x` for the three dilated 3x3 branches of ASPP (deepv3.py:84-92; rates d, 2d, 3d) from a
    single read of x (mss_wino_input_transform_aspp3_f32): bit-identical to the three separate input transforms, 1 x instead of
    3 x 1.07 GB read at 2 x 128 x 256 x 4096; gap is None. x a FactoredAct: the two-source kernel
    (mss_wino_input_transform_aspp3_src2_f32) on the map that is never stored, gap [N, C] its global average from the same kernel;
    where the plan takes no X' from it (not single_read: MSS_WINO_ASPP3=0, over budget) the kernel runs in its sums-only mode and the
    answer is (None, gap). dropped (the plan's AsppDropped): mss_wino_input_transform_aspp3_dropped_f32, image n's rows hold
    [u ; kept channels of v] only. The plan (aspp_plan_for) says single_read or gap_from_kernel: a refusal of the kernel is an error."""
    factored = isinstance(x, FactoredAct)
    assert (plan.gap_from_kernel and (plan.single_read or dropped is None)) if factored else (plan.single_read and dropped is None)
    N, H, W, C, d = x.N, x.H, x.W, x.C, rates[0]
    dev = x.buf.device
    out = AsppXt(plan, C, dev) if plan.single_read else None
    xts = [ptr(t) for t in out.xts] if out else [None, None, None]
    ctiles = (ctypes.c_int * 3)(*plan.tiles)
    nbytes = 4.0 * (N * H * W * C + (sum(p * t for p, t in zip(plan.Ps, plan.Ts)) * C if out else 0))
    tag = ("input_aspp3" if out else "aspp_gap", N, H, W, C, d, tuple(plan.tiles)) + (("dropped",) if dropped is not None else ())
    if not factored:
        with _Timed("wino_transform", nbytes, tag):
            call("mss_wino_input_transform_aspp3_f32", x.ptr, x.ld, N, H, W, C, d, ctiles, *xts)
        return out, None
    sums = torch.empty((N, d * d, C), device=dev, dtype=torch.float32)       # fully overwritten by the kernel
    gap = torch.empty((N, C), device=dev, dtype=torch.float32)
    (sc0, sh0), (sc1, sh1) = x.aff0, x.aff1
    assert all(t.is_contiguous() and t.shape[-1] == a.C for a, ts in ((x.a0, x.aff0), (x.a1, x.aff1)) for t in ts)
    src0 = (x.a0.ptr, x.a0.ld, x.a0.C, ptr(sc0), ptr(sh0), x.a0.C if sc0.dim() == 2 else 0)
    with _Timed("wino_transform", nbytes, tag):
        if dropped is not None:
            call("mss_wino_input_transform_aspp3_dropped_f32", *src0, dropped.xc.ptr, dropped.xc.ld, x.a1.C, ptr(dropped.place),
                 ptr(dropped.k_steps), N, H, W, d, ctiles, *xts, ptr(sums), ptr(gap))
        else:
            call("mss_wino_input_transform_aspp3_src2_f32", *src0, x.a1.ptr, x.a1.ld, x.a1.C, ptr(sc1), ptr(sh1),
                 x.a1.C if sc1.dim() == 2 else 0, N, H, W, d, ctiles, *xts, ptr(sums), ptr(gap))
    return out, gap


def aspp_dropped_separate_transforms(fx, rates, plan, dropped):
    """The second formulation of the dropped-channel transform (the plan's dropped_separate: MSS_WINO_ASPP3=0, as for the dense
    route): the compacted map [u ; compacted v] is materialised with its 4096-column pitch and each dilation runs the plain input
    transform on it; GAP(w) comes from the two-source kernel's sums-only mode. The columns an image's rows hold get the bits of the
    single-read kernel; the columns behind them are transformed too (zeros), which nothing reads. (AsppXt, gap) as above."""
    assert plan.dropped_separate and not plan.pair_tile
    N, H, W, C = fx.N, fx.H, fx.W, fx.C
    _none, gap = aspp_transforms(fx, rates, plan)                # (no single_read on this plan: the sums alone)
    dev = fx.buf.device
    wm = Act.zeros(N, H, W, C, dev)
    u = wm.slice(0, fx.a0.C)
    call("mss_affine_relu_nhwc_f32", fx.a0.ptr, fx.a0.ld, u.ptr, u.ld, fx.a0.M, fx.a0.C, ptr(fx.aff0[0]), ptr(fx.aff0[1]), 1)
    hw = H * W
    ks = dropped.k_steps
    # v's compacted columns: what the compaction pass wrote, image by image; 16 * k_steps[n] is a device value, so whole rows are
    # copied from a zero-filled compaction buffer (torch glue on a test route)
    xc0 = Act.zeros(N, H, W, fx.a1.C, dev)
    call("mss_chan_compact_act_f32", fx.a1.ptr, fx.a1.ld, xc0.ptr, xc0.ld, N, hw, fx.a1.C, ptr(dropped.place), ptr(ks), ptr(fx.aff1[0]),
         ptr(fx.aff1[1]))
    wm.buf[..., fx.a0.C:] = xc0.buf
    out = AsppXt(plan, C, dev)
    for r, t, xt in zip(rates, plan.tiles, out.xts):
        with _Timed("wino_transform", 4.0 * (N * hw * C + xt.numel()), ("input", N, H, W, C, r, t)):
            call("mss_wino_input_transform_f32", wm.ptr, wm.ld, N, H, W, C, r, t, None, None, 0, ptr(xt))
    return out, gap


def conv2d_wgrad_winograd(x, dy, K, C, dil=1, in_affine=None, in_relu=False, xt=None, tile=None):
    """[K,C,3,3] weight gradient of a 3x3 / stride-1 / padding = dilation conv in the Winograd domain:
    dU[p] = dY'[p]^T X'[p] ((m+2)^2 batched MFMA products over tiles, 2.25x / 4x fewer FLOPs than the 9-tap
    form). xt: the X' kept by the forward (its leading dimension tells the tile size)."""
    N, H, W = x.N, x.H, x.W
    dev = x.buf.device
    if xt is not None:
        ts = WINO_TILE_OF_P[xt.shape[0]]
    else:
        ts = tile or wino_tile(H, W, dil)
    P = (ts + 2) ** 2
    T = _lib.value("mss_wino_num_tiles", N, H, W, dil, ts)
    Kpad, Cp = _round_up(K, 4), _round_up(C, 4)
    with _Timed("wgrad_winograd", 2.0 * N * H * W * K * C * 9, (N, H, W, C, K, 3, 1, dil)):
        if xt is None:
            xt = torch.empty((P, T, C), device=dev, dtype=torch.float32)
            sc, sh = in_affine if in_affine is not None else (None, None)
            with _Timed("wino_transform", 4.0 * (N * H * W * C + P * T * C), ("input", N, H, W, C, dil, ts)):
                call("mss_wino_input_transform_f32", x.ptr, x.ld, N, H, W, C, dil, ts, ptr(sc), ptr(sh), int(in_relu), ptr(xt))
        assert tuple(xt.shape) == (P, T, C)
        dyt = torch.empty((P, T, K), device=dev, dtype=torch.float32)
        with _Timed("wino_transform", 4.0 * (N * H * W * K + P * T * K), ("grad_output", N, H, W, K, dil, ts)):
            call("mss_wino_grad_output_transform_f32", dy.ptr, dy.ld, N, H, W, K, dil, ts, ptr(dyt))
        du = torch.empty((P, Kpad, Cp), device=dev, dtype=torch.float32)     # fully overwritten by the kernel
        a = _wino_args(xt, T, C, K, Kpad, P)
        a.route = 1 if gemm_route() == "bf16x3" else 0
        ws, ws_bytes = _wgrad_workspace(a, Cp, dev)
        with _Timed(_wgrad_kind(a, K), 2.0 * P * T * K * C, (P, 1, T, C, K, 1, 1, 1)):
            call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), K, ptr(du), Cp, ptr(ws), ws_bytes)
        grad = torch.empty((K, C, 3, 3), device=dev, dtype=torch.float32)
        call("mss_wino_weight_grad_transform_f32", ptr(du), ptr(grad), K, C, Kpad, Cp, ts)
    return grad


def aspp_dropped_weights(rows, K, C, Kpad, ld, tile, dropped):
    """The per-image Winograd-domain weights U'_n of one dilated branch of the dropped-channel ASPP products, [P][N][Kpad][C] as a
    WinoWeight over N * K output channels: `rows` is the branch's composed weight as the compose GEMM left it (tap-major
    [9][Kpad][ld]); its columns are gathered per image into the compacted order (mss_conv2d_unpack_wgrad_f32 with `place`) and the
    N [K][C][3][3] tensors go through the dense filter transform as one. No dense U' is made."""
    assert Kpad == K and K % 128 == 0
    N = dropped.N
    wg = torch.empty((N, K, C, 3, 3), device=rows.device, dtype=torch.float32)
    call("mss_conv2d_unpack_wgrad_f32", ptr(rows), ptr(wg), K, C, 3, 3, Kpad, ld, 0, ptr(dropped.place), ptr(dropped.k_steps), N, dropped.C0)
    P = (tile + 2) ** 2
    u = torch.empty((P, N * K, C), device=rows.device, dtype=torch.float32)
    call("mss_wino_pack_weights_f32", ptr(wg), ptr(u), N * K, C, N * K, C, tile)
    return WinoWeight(u, K, C, Kpad, C, tile)


def conv3x3_dropped(x, ww, dil, out, keep_xt, want_stats, xt, dropped):
    """One dilated ASPP branch on the dropped-channel X' (aspp_transforms(..., dropped=)) with aspp_dropped_weights."""
    N, H, W, C, K = x.N, x.H, x.W, ww.C, ww.K
    assert dropped.N == N
    with _Timed("conv_winograd", 2.0 * N * H * W * K * C * 9, (N, H, W, C, K, 3, 1, dil)):
        return _wino_gemm_and_output(xt, ww, N, H, W, dil, None, out, keep_xt, want_stats, dropped=dropped)


def conv3x3_wgrad_dropped(x, dy, K, C, dil, xt, dropped):
    """Weight gradient of a dilated ASPP branch from the dropped-channel X': dU'_n = dY'_n^T X'_n per (position, image) over that
    image's rows and columns only (gemm_tn_direct_kernel's per-image form), G^T dU' G of all of them in one launch. The answer is
    [N][K][C][3][3] in each image's COMPACTED column order; deepv3's projection pack gathers the columns back to their channels and
    adds the images in ascending order (mss_conv2d_pack_weights_f32 with `col`)."""
    N, H, W = x.N, x.H, x.W
    dev = xt.device
    ts = WINO_TILE_OF_P[xt.shape[0]]
    P, T = xt.shape[0], xt.shape[1]
    Ti = T // N
    assert T % N == 0 and dropped.N == N and K % 128 == 0 and C % 128 == 0 and tuple(xt.shape) == (P, T, C)
    with _Timed("wgrad_winograd", 2.0 * N * H * W * K * C * 9, (N, H, W, C, K, 3, 1, dil)):
        dyt = torch.empty((P, T, K), device=dev, dtype=torch.float32)
        with _Timed("wino_transform", 4.0 * (N * H * W * K + P * T * K), ("grad_output", N, H, W, K, dil, ts)):
            call("mss_wino_grad_output_transform_f32", dy.ptr, dy.ld, N, H, W, K, dil, ts, ptr(dyt))
        du = torch.empty((P, N * K, C), device=dev, dtype=torch.float32)     # tiles behind an image's extent stay unwritten, and unread
        a = _wino_args(xt, Ti, C, K, K, P * N, dropped)
        # optional scratch: with it the packed job plan cuts its last, partial round by rows
        ws = torch.empty(_lib.MSS_WGRAD_PERIMG_TAIL_BYTES // 4, device=dev, dtype=torch.float32)
        with _Timed("conv_wgrad", 2.0 * P * Ti * K * dropped.columns(), ("aspp_dropped", P, N, Ti, C, K)):
            call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), K, ptr(du), C, ptr(ws), _lib.MSS_WGRAD_PERIMG_TAIL_BYTES)
        grad = torch.empty((N, K, C, 3, 3), device=dev, dtype=torch.float32)
        call("mss_wino_weight_grad_transform_f32", ptr(du), ptr(grad), N * K, C, N * K, C, ts)
    return grad


def conv3x3_wgrad(x, dy, K, C, dil=1, in_affine=None, in_relu=False, xt=None, max_tile=6):
    """Weight gradient of a 3x3 / stride-1 layer. max_tile caps the Winograd tile edge (as conv3x3's): the F(6x6) weight-gradient
    transform G^T dU G carries ~20x the rounding error of F(4x4)'s (measured on the pixel decoder's 3x3 layer, round 4)."""
    tile = WINO_TILE_OF_P[xt.shape[0]] if xt is not None else wino_tile(x.H, x.W, dil, max_tile)
    if use_winograd(C, K, 1, in_affine, tile):
        return conv2d_wgrad_winograd(x, dy, K, C, dil, in_affine, in_relu, xt=xt, tile=tile)
    return conv2d_wgrad(x, dy, K, C, 3, 3, dil=dil, pad=dil, in_affine=in_affine, in_relu=in_relu)


def image_to_nhwc(img, Cp=16):
    n, c, h, w = img.shape
    img = img.contiguous()
    out = Act.empty(n, h, w, Cp, img.device)
    call("mss_nchw_to_nhwc_pad_f32", ptr(img), out.ptr, n, c, h, w, Cp)
    return out


def stem_im2col(img):
    """[N,3,H,W] NCHW image -> Act [N,H,W,32]: the 27 taps of a 3x3 / padding-1 window per pixel (+5 zero channels)."""
    n, c, h, w = img.shape
    if c != 3:
        raise ValueError(f"the stem expects a 3-channel image, got {c}")
    img = img.contiguous()
    out = Act.empty(n, h, w, 32, img.device)
    call("mss_im2col3x3_c3_f32", ptr(img), out.ptr, n, h, w)
    return out


def stem_conv_pool(img, weight):
    """[N,3,H,W] NCHW image, mod1.conv1.weight [64,3,3,3] -> Act [N,(H-1)//2+1,(W-1)//2+1,64] = MaxPool2d(3,2,1)(conv3x3(img)) in
    ONE kernel (csrc/stem.hip): the full-resolution 64-channel map never exists."""
    n, c, h, w = img.shape
    if c != 3 or tuple(weight.shape) != (64, 3, 3, 3):
        raise ValueError(f"the fused stem expects a 3-channel image and a [64,3,3,3] weight, got {tuple(img.shape)} / {tuple(weight.shape)}")
    img = img.contiguous()
    wt = weight.detach().contiguous()
    out = Act.empty(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64, img.device)
    call("mss_stem_conv_pool_f32", ptr(img), ptr(wt), out.ptr, out.ld, n, h, w)
    return out


def packed_stem(param):
    """mod1.conv1.weight [64,3,3,3] as the 1x1 weight [64,32,1,1] that matches stem_im2col's channel order."""
    def make():
        k = param.shape[0]
        w = torch.zeros((k, 32, 1, 1), device=param.device, dtype=torch.float32)
        w[:, :27, 0, 0] = param.detach().reshape(k, 27)
        return pack_weight(w)
    return _cached_pack(param, ("stem",), make)


def packed_stem7(param):
    """stem.conv1.weight [64,3,7,7] as the [49][64][4] pack of the 7x7 stem kernel (csrc/stem7.hip): the fourth input channel is zero."""
    def make():
        w = param.detach().contiguous()
        t = torch.empty((49, 64, 4), device=w.device, dtype=torch.float32)
        call("mss_conv2d_pack_weights_f32", ptr(w), ptr(t), 64, 3, 7, 7, 64, 4, 0, None, 0, 0)
        return PackedWeight(t, 64, 3, 7, 7, 64, 4)
    return _cached_pack(param, ("stem7",), make)


def stem7_conv(img_nchw, weight, out_affine, relu=True):
    """[N,3,H,W] NCHW image, stem.conv1.weight [64,3,7,7] -> Act [N,(H-1)//2+1,(W-1)//2+1,64] = relu(conv7x7(img, stride 2, padding 3) *
    scale + shift) (detectron2 BasicStem before its max-pool) on the 16x16x4 fp32 MFMA, one filter tap per instruction. The image
    goes through image_to_nhwc(Cp=4); the kernel's contract is that this pad channel is zero."""
    n, c, h, w = img_nchw.shape
    if c != 3 or tuple(weight.shape) != (64, 3, 7, 7):
        raise ValueError(f"the 7x7 stem expects a 3-channel image and a [64,3,7,7] weight, got {tuple(img_nchw.shape)} / {tuple(weight.shape)}")
    if weight.dtype != torch.float32 or not weight.is_cuda or img_nchw.dtype != torch.float32 or not img_nchw.is_cuda:
        raise TypeError("stem7_conv needs float32 CUDA tensors")
    x = image_to_nhwc(img_nchw, Cp=4)
    pw = packed_stem7(weight)
    OH, OW = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = Act.empty(n, OH, OW, 64, img_nchw.device)
    _conv_launch(x, pw, out, OH, OW, 2, 1, 3, None, False, out_affine, relu, None)
    return out


def stem7_wgrad(img_nchw, dy, a0=None):
    """Weight gradient [64,3,7,7] of the 7x7 / stride-2 / padding-3 stem convolution (csrc/stem7_wgrad.hip, through
    mss_conv2d_wgrad_f32) of the [N,3,H,W] NCHW image. a0 None: dy is the gradient dz at the convolution's output grid, Act
    [N,(H-1)//2+1,(W-1)//2+1,64]. a0 (Act, the stored stem output after norm and ReLU): dy is the gradient at the max-pooled map
    (3x3, stride 2, padding 1) and the kernel forms dz = [a0 > 0] * max-pool backward itself, the arg-max recomputed from a0 by
    F.max_pool2d's rule (first maximum in row-major order). The image goes through image_to_nhwc(Cp=4), as stem7_conv's.
    Native fp32 MFMA on either gemm route; deterministic."""
    n, c, h, w = img_nchw.shape
    if c != 3:
        raise ValueError(f"the 7x7 stem expects a 3-channel image, got {tuple(img_nchw.shape)}")
    if img_nchw.dtype != torch.float32 or not img_nchw.is_cuda:
        raise TypeError("stem7_wgrad needs a float32 CUDA image")
    OH, OW = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    grid = (n, OH, OW) if a0 is None else (n, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1)
    if (dy.N, dy.H, dy.W) != grid or dy.C != 64 or (a0 is not None and ((a0.N, a0.H, a0.W) != (n, OH, OW) or a0.C != 64)):
        raise ValueError(f"stem7_wgrad: dy {(dy.N, dy.H, dy.W, dy.C)} / a0 {None if a0 is None else (a0.N, a0.H, a0.W, a0.C)} do not "
                         f"belong to a {tuple(img_nchw.shape)} image")
    x = image_to_nhwc(img_nchw, Cp=4)
    dev = img_nchw.device
    dwp = torch.empty((49, 64, 4), device=dev, dtype=torch.float32)                  # fully overwritten by the kernel
    a = MssConvArgs()
    a.x = x.ptr
    a.N, a.H, a.W, a.C, a.ldx = n, h, w, 4, 4
    a.OH, a.OW, a.K, a.Kpad = OH, OW, 64, 64
    a.R, a.S, a.stride, a.dil, a.pad = 7, 7, 2, 1, 3
    if a0 is not None:
        a.res, a.ldres, a.res_mask = a0.ptr, a0.ld, 1
    ws, ws_bytes = _wgrad_workspace(a, 4, dev)
    with _Timed("conv_wgrad", 2.0 * n * OH * OW * 64 * 3 * 49, (n, h, w, 3, 64, 7, 2, 1)):
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), dy.ptr, dy.ld, ptr(dwp), 4, ptr(ws), ws_bytes)
    grad = torch.empty((64, 3, 7, 7), device=dev, dtype=torch.float32)
    call("mss_conv2d_unpack_wgrad_f32", ptr(dwp), ptr(grad), 64, 3, 7, 7, 64, 4, 0, None, None, 0, 0)
    return grad


class BNState:
    """Folded BatchNorm: y = x*scale + shift (+ what the backward needs in train mode)."""
    __slots__ = ("scale", "shift", "save_mean", "save_invstd", "M", "train")


def _col_accum(M, C, device):
    """Scratch of the deterministic two-stage per-channel reductions: [2C] sums + the first stage's partial rows."""
    return torch.empty(_lib.value("mss_col_reduce_accum_doubles", M, C), device=device, dtype=torch.float64)


def bn_fold(bn, x=None, train=False, M=None, x_rows=None, out=None):
    """Fold nn.BatchNorm2d `bn` into (scale, shift). train=True computes batch statistics of the
    NHWC activation x (Act) and updates the running buffers exactly like F.batch_norm
    (momentum 0.1, unbiased running variance; mynn.py:8-12). out: (scale, shift) to write into -- e.g. a 256-channel
    slice of the 1280-channel vectors of the ASPP concat, instead of a copy afterwards."""
    C = bn.num_features
    dev = bn.weight.device
    st = BNState()
    st.train = train
    if out is not None:
        st.scale, st.shift = out
        assert st.scale.numel() == C and st.shift.numel() == C and st.scale.is_contiguous() and st.shift.is_contiguous()
    else:
        st.scale = torch.empty(C, device=dev, dtype=torch.float32)
        st.shift = torch.empty(C, device=dev, dtype=torch.float32)
    st.save_mean = st.save_invstd = None
    if not train:
        call("mss_bn_fold_eval_f32", ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
             float(bn.eps), C, ptr(st.scale), ptr(st.shift))
        st.M = None
        return st
    if x_rows is not None:          # plain [M, C] matrix (image-pooling branch)
        M = x_rows.shape[0]
        accum = _col_accum(M, C, dev)
        call("mss_bn_stats_nhwc_f32", ptr(x_rows), M, C, x_rows.shape[1], ptr(accum))
    elif x.stats is not None and x.stats.shape[2] == C and x.C == C:   # left by the producing kernel: no re-read of x
        M = x.M
        accum = _col_accum(x.stats.shape[0], C, dev)
        st.M = M
        st.save_mean = torch.empty(C, device=dev, dtype=torch.float32)
        st.save_invstd = torch.empty(C, device=dev, dtype=torch.float32)
        mom = 0.1 if bn.momentum is None else float(bn.momentum)
        track = bn.track_running_stats and bn.running_mean is not None
        # partial sums -> column sums -> folded affine + running statistics: two launches (the second stage and the fold are one)
        call("mss_bn_fold_train_from_partials_f32", ptr(x.stats), x.stats.shape[0], C, ptr(accum), M, ptr(bn.weight), ptr(bn.bias),
             float(bn.eps), mom, ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None, ptr(st.scale),
             ptr(st.shift), ptr(st.save_mean), ptr(st.save_invstd))
        x.stats = None
        if track and bn.num_batches_tracked is not None:
            if _nbt_pending is not None:
                _nbt_pending.append(bn.num_batches_tracked)
            else:
                bn.num_batches_tracked += 1
        return st
    else:
        M = x.M
        accum = _col_accum(M, C, dev)
        call("mss_bn_stats_nhwc_f32", x.ptr, M, C, x.ld, ptr(accum))
    st.M = M
    st.save_mean = torch.empty(C, device=dev, dtype=torch.float32)
    st.save_invstd = torch.empty(C, device=dev, dtype=torch.float32)
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    track = bn.track_running_stats and bn.running_mean is not None
    call("mss_bn_finalize_train_f32", ptr(accum), M, C, ptr(bn.weight), ptr(bn.bias), float(bn.eps), mom,
         ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None, ptr(st.scale),
         ptr(st.shift), ptr(st.save_mean), ptr(st.save_invstd))
    if track and bn.num_batches_tracked is not None:
        if _nbt_pending is not None:
            _nbt_pending.append(bn.num_batches_tracked)      # one launch for all layers of a forward (43 tiny kernels otherwise)
        else:
            bn.num_batches_tracked += 1
    return st


_nbt_pending = None


class batched_counters:
    """with batched_counters(): every train-mode bn_fold inside defers its `num_batches_tracked += 1`; they are applied by ONE
    multi-tensor add on exit (nn.BatchNorm2d's counter, F.batch_norm's bookkeeping: same values, 1 launch instead of one per layer)."""

    def __enter__(self):
        global _nbt_pending
        self.prev, _nbt_pending = _nbt_pending, []
        return self

    def __exit__(self, *exc):
        global _nbt_pending
        pending, _nbt_pending = _nbt_pending, self.prev
        if pending:
            if self.prev is not None:
                self.prev.extend(pending)
            else:
                torch._foreach_add_(pending, 1)
        return False


def bn_relu_backward(dy, x, st, relu=True, want_param_grads=False, x_rows=None, dy_rows=None):
    """Backward of y = relu(x*scale+shift) with (scale, shift) = folded BN `st`.
    Returns (dx Act or [M,C] tensor, dgamma, dbeta)."""
    if x_rows is not None:
        M, C = x_rows.shape
        xp, ldx, dyp, lddy = ptr(x_rows), x_rows.shape[1], ptr(dy_rows), dy_rows.shape[1]
        dx = torch.empty_like(x_rows)
        dxp, lddx = ptr(dx), C
        dev = x_rows.device
    else:
        M, C = x.M, x.C
        xp, ldx, dyp, lddy = x.ptr, x.ld, dy.ptr, dy.ld
        dx = Act.empty(x.N, x.H, x.W, C, x.buf.device)
        dxp, lddx = dx.ptr, dx.ld
        dev = x.buf.device
    dgamma = dbeta = None
    accum = None
    if st.train:
        accum = _col_accum(M, C, dev)
        call("mss_bn_relu_bwd_reduce_f32", dyp, lddy, xp, ldx, M, C, ptr(st.scale), ptr(st.shift), ptr(st.save_mean),
             ptr(st.save_invstd), int(relu), ptr(accum))
        if want_param_grads:
            dgamma = torch.zeros(C, device=dev, dtype=torch.float32)
            dbeta = torch.zeros(C, device=dev, dtype=torch.float32)
    elif want_param_grads:
        raise NotImplementedError("BatchNorm affine gradients in eval mode")
    call("mss_bn_relu_bwd_apply_f32", dyp, lddy, xp, ldx, dxp, lddx, M, C, None, ptr(st.scale), ptr(st.shift),
         ptr(st.save_mean), ptr(st.save_invstd), int(relu), ptr(accum), ptr(dgamma), ptr(dbeta))
    return dx, dgamma, dbeta


def conv3x3_on_upsampled_concat(a, small, weight, want_stats=False):
    """conv3x3(concat([a, upsample_ac(small -> a.H x a.W)], channels), weight) -- the decoder's first 3x3 layer on dec0 =
    cat(bot_fine(m2), Upsample(bot_aspp(...))) (deepv3.py:269-275) -- with the bilinear upsample interpolated inside the Winograd
    input transform (mss_wino_input_transform_upcat_f32): the full-resolution upsampled map is never written or read.
    Returns None where that transform does not apply (non-Winograd or small shapes, MSS_UPCAT_FUSED=0): the caller builds the concat."""
    k_out, c_in = weight.shape[0], weight.shape[1]
    N, H, W = a.N, a.H, a.W
    tile = wino_tile(H, W, 1)
    if not (os.environ.get("MSS_UPCAT_FUSED", "1") != "0" and _tile_hook is None and tile >= 4 and a.C + small.C == c_in and a.C % 4 == 0
            and small.N == N and use_winograd(c_in, k_out, 1, None, tile)):
        return None
    dev = a.buf.device
    ww = packed_wino(weight, False, tile)
    P = (tile + 2) ** 2
    T = _lib.value("mss_wino_num_tiles", N, H, W, 1, tile)
    with _Timed("conv_winograd", 2.0 * N * H * W * k_out * c_in * 9, (N, H, W, c_in, k_out, 3, 1, 1)):
        xt = torch.empty((P, T, c_in), device=dev, dtype=torch.float32)
        with _Timed("wino_transform", 4.0 * (N * H * W * a.C + small.M * small.C + P * T * c_in), ("input+upsample", N, H, W, c_in, 1, tile)):
            rc = _lib.status("mss_wino_input_transform_upcat_f32", a.ptr, a.ld, a.C, small.ptr, small.ld, small.H, small.W, N, H, W, c_in,
                             tile, ptr(xt))
        if rc == _lib.MSS_ERR_UNSUPPORTED:
            return None
        if rc != 0:
            raise _lib.MssError(f"mss_wino_input_transform_upcat_f32 failed with code {rc}")
        return _wino_gemm_and_output(xt, ww, N, H, W, 1, None, None, None, want_stats)


def conv3x3_dgrad_after_bn(dy, x, st, weight, relu=True):
    """conv3x3(bn_relu_backward(dy, x, st)[0], weight, flip=True) -- the data gradient of the 3x3 layer in FRONT of a train-mode
    BatchNorm+ReLU -- with the BatchNorm backward's apply pass folded into the Winograd input transform of that convolution
    (mss_wino_input_transform_bnbwd_f32): the gradient w.r.t. the BatchNorm input is never written or read back. Falls back to the
    two separate steps where the fused transform does not apply (eval-mode statistics, non-Winograd or small shapes,
    MSS_BNBWD_FUSED=0). Same arithmetic per element, so the two routes agree bit for bit."""
    k_out, c_in = weight.shape[1], weight.shape[0]
    tile = wino_tile(x.H, x.W, 1)
    fused = (st.train and os.environ.get("MSS_BNBWD_FUSED", "1") != "0" and _tile_hook is None and tile >= 4
             and use_winograd(c_in, k_out, 1, None, tile) and dy.C == c_in and x.C == c_in)
    if fused:
        N, H, W, C = x.N, x.H, x.W, c_in
        dev = x.buf.device
        accum = _col_accum(x.M, C, dev)
        call("mss_bn_relu_bwd_reduce_f32", dy.ptr, dy.ld, x.ptr, x.ld, x.M, C, ptr(st.scale), ptr(st.shift), ptr(st.save_mean),
             ptr(st.save_invstd), int(relu), ptr(accum))
        ww = packed_wino(weight, True, tile)
        P = (tile + 2) ** 2
        T = _lib.value("mss_wino_num_tiles", N, H, W, 1, tile)
        with _Timed("conv_winograd", 2.0 * N * H * W * k_out * C * 9, (N, H, W, C, k_out, 3, 1, 1)):
            xt = torch.empty((P, T, C), device=dev, dtype=torch.float32)
            with _Timed("wino_transform", 4.0 * (2 * N * H * W * C + P * T * C), ("input+bn_bwd", N, H, W, C, 1, tile)):
                rc = _lib.status("mss_wino_input_transform_bnbwd_f32", dy.ptr, dy.ld, x.ptr, x.ld, N, H, W, C, 1, tile, ptr(st.scale),
                                 ptr(st.shift), ptr(st.save_mean), ptr(st.save_invstd), ptr(accum), int(relu), ptr(xt))
            if rc == 0:
                return _wino_gemm_and_output(xt, ww, N, H, W, 1, None, None, None, False)
            if rc != _lib.MSS_ERR_UNSUPPORTED:
                raise _lib.MssError(f"mss_wino_input_transform_bnbwd_f32 failed with code {rc}")
            del xt
    dx, _, _ = bn_relu_backward(dy, x, st, relu=relu)
    return conv3x3(dx, weight, flip=True)


def maxpool3s2(x):
    OH, OW = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
    y = Act.empty(x.N, OH, OW, x.C, x.buf.device)
    call("mss_maxpool3s2_nhwc_f32", x.ptr, x.ld, y.ptr, y.ld, x.N, x.H, x.W, x.C, OH, OW)
    return y


def gap(x):
    y = torch.empty((x.N, x.C), device=x.buf.device, dtype=torch.float32)
    # the producing kernel's epilogue left per-64-row column sums (x.stats, wanted for BatchNorm statistics or asked for by the
    # caller): the mean comes from those few MB instead of another pass over the map (r04; MSS_GAP_FROM_STATS=0: always the pass)
    if x.stats is not None and (x.H * x.W) % 64 == 0 and x.stats.shape[0] * 64 == x.M and x.stats.shape[2] == x.C \
            and os.environ.get("MSS_GAP_FROM_STATS", "1") != "0":
        call("mss_gap_from_partials_f32", ptr(x.stats), x.N, x.H * x.W, x.C, ptr(y))
        return y
    ws = torch.empty(_lib.value("mss_colsum_workspace_floats", x.N, x.H * x.W, x.C), device=x.buf.device, dtype=torch.float32)
    call("mss_gap_nhwc_f32", x.ptr, x.ld, ptr(y), x.N, x.H * x.W, x.C, ptr(ws))
    return y


def colsum(dy):
    y = torch.empty((dy.N, dy.C), device=dy.buf.device, dtype=torch.float32)
    ws = torch.empty(_lib.value("mss_colsum_workspace_floats", dy.N, dy.H * dy.W, dy.C), device=dy.buf.device, dtype=torch.float32)
    call("mss_colsum_nhwc_f32", dy.ptr, dy.ld, ptr(y), dy.N, dy.H * dy.W, dy.C, ptr(ws))
    return y


def broadcast_rows(v, out, scale=None, shift=None, relu=False):
    call("mss_broadcast_rows_nhwc_f32", ptr(v), out.ptr, out.ld, out.N, out.H * out.W, out.C, ptr(scale), ptr(shift),
         int(relu))
    return out


def upsample_ac(x, OH, OW, out=None):
    if out is None:
        out = Act.empty(x.N, OH, OW, x.C, x.buf.device)
    call("mss_upsample_ac_nhwc_f32", x.ptr, x.ld, out.ptr, out.ld, x.N, x.H, x.W, OH, OW, x.C)
    return out


def upsample_ac_bwd(dy, IH, IW):
    dx = Act.empty(dy.N, IH, IW, dy.C, dy.buf.device)
    call("mss_upsample_ac_nhwc_bwd_f32", dy.ptr, dy.ld, dx.ptr, dx.ld, dy.N, IH, IW, dy.H, dy.W, dy.C)
    return dx


def ood_score(dec2, dec1, OH, OW, want_score=True, want_logit=True, want_label=False):
    """The OOD-score tail (deepv3.py:279-283). dec2/dec1: Acts at half res, one channel per class (1..100; both the same)."""
    ref = dec2 if dec2 is not None else dec1
    C = ref.C
    if dec2 is not None and dec1 is not None and dec1.C != dec2.C:
        raise ValueError(f"ood_score: dec2 has {dec2.C} classes, dec1 has {dec1.C}")
    dev = ref.buf.device
    N = ref.N
    score = torch.empty((N, OH, OW), device=dev, dtype=torch.float32) if want_score else None
    logit = torch.empty((N, C, OH, OW), device=dev, dtype=torch.float32) if want_logit else None
    label = torch.empty((N, OH, OW), device=dev, dtype=torch.uint8) if want_label else None
    call("mss_ood_score_f32", dec2.ptr if dec2 is not None else None, dec2.ld if dec2 is not None else 0,
         dec1.ptr if dec1 is not None else None, dec1.ld if dec1 is not None else 0, N, ref.H, ref.W, C, OH, OW,
         ptr(score), ptr(logit), ptr(label))
    return score, logit, label


def ood_score_bwd(dec2, dscore, dlogit, ddec2, ddec1, OH, OW):
    call("mss_ood_score_bwd_f32", dec2.ptr, dec2.ld, ptr(dscore), ptr(dlogit), dec2.N, dec2.H, dec2.W, dec2.C, OH, OW,
         ddec2.ptr if ddec2 is not None else None, ddec2.ld if ddec2 is not None else 0,
         ddec1.ptr if ddec1 is not None else None, ddec1.ld if ddec1 is not None else 0)


def m2f_score(class_logits, mask_logits, size):
    """train_m2f.py:387-407 -> [B,H,W]."""
    B, Q, C1 = class_logits.shape
    _, _, Hm, Wm = mask_logits.shape
    H, W = size
    cls = class_logits.contiguous().float()
    mask = mask_logits.contiguous().float()
    out = torch.empty((B, H, W), device=cls.device, dtype=torch.float32)
    call("mss_m2f_score_f32", ptr(cls), ptr(mask), B, Q, C1 - 1, H, W, Hm, Wm, ptr(out))
    return out


def m2f_mask_logits(mask_embed, mask_features):
    """einsum("bqc,bchw->bqhw", mask_embed, mask_features) (mask2former_transformer_decoder.py:544-548) as ONE batched
    MFMA GEMM, written pixel-major: returns [B, h, w, Q] (queries contiguous), the layout m2f_score_fused reads."""
    B, Q, C = mask_embed.shape
    Bf, Cf, h, w = mask_features.shape
    if (B, C) != (Bf, Cf):
        raise ValueError(f"mask_embed {tuple(mask_embed.shape)} does not match mask_features {tuple(mask_features.shape)}")
    return m2f_mask_logits_act(mask_embed, Act.from_nchw(mask_features.float()), Q)


def m2f_mask_logits_act(mask_embed, x, ldq):
    """m2f_mask_logits on mask features that are already an Act [B, h, w, C] (the transformer decoder converts them once for
    its 10 mask predictions) -> [B, h, w, ldq]; ldq >= Q pads the query axis (columns Q .. ldq-1 are written as zeros)."""
    B, Q, C = mask_embed.shape
    h, w = x.H, x.W
    if (B, C) != (x.N, x.C) or ldq < Q:
        raise ValueError(f"mask_embed {tuple(mask_embed.shape)} does not match mask features [{x.N}, {h}, {w}, {x.C}] / ldq {ldq}")
    Kpad = _lib.value("mss_conv2d_kpad", ldq)
    wp = torch.zeros((B, Kpad, C), device=x.buf.device, dtype=torch.float32)
    wp[:, :Q] = mask_embed.detach().float()
    out = torch.empty((B, h, w, ldq), device=x.buf.device, dtype=torch.float32)
    a = MssConvArgs()
    a.x, a.w, a.y = x.ptr, ptr(wp), ptr(out)
    a.N, a.H, a.W, a.C, a.ldx = 1, 1, h * w, C, x.ld
    a.OH, a.OW, a.K, a.Kpad, a.ldy = 1, h * w, ldq, Kpad, ldq
    a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
    a.batch, a.x_bs, a.w_bs, a.y_bs = B, h * w * x.ld, Kpad * C, h * w * ldq
    with _Timed(_fwd_kind(a), 2.0 * B * h * w * C * Q, (B, 1, h * w, C, Q, 1, 1, 1)):
        call("mss_conv2d_forward_f32", ctypes.byref(a))
    return out


# ---- masked attention of the Mask2Former transformer decoder (csrc/m2f_attn.hip) ----------------------------------------------
def m2f_attn_mask_bits(mask_logits_nhwc, Q, size):
    """Pixel-major mask logits [B, hm, wm, ldq] -> (bits [B, 2, h*w, W], allowed [B, 2, W]) int32 views, W = ceil(Q / 32):
    the foreground (logit < 0) / background (logit > 0) attention masks of a level of `size` = (h, w) as bit rows over the
    queries, and per query the "some key is allowed" bits (include/mss_hip.h). Both live in one float32-typed buffer."""
    B, hm, wm, ldq = mask_logits_nhwc.shape
    h, w = size
    _need_f32_cuda("m2f_attn_mask_bits", mask_logits_nhwc)
    lg = mask_logits_nhwc.contiguous()
    W = (Q + 31) // 32
    words = torch.empty(B * 2 * (h * w + 1) * W, device=lg.device, dtype=torch.float32).view(torch.int32)
    bits = words[:B * 2 * h * w * W].view(B, 2, h * w, W)
    allowed = words[B * 2 * h * w * W:].view(B, 2, W)
    call("mss_m2f_attn_mask_bits_f32", ptr(lg), B, Q, ldq, hm, wm, h, w, ptr(bits), ptr(allowed))
    return bits, allowed


def m2f_attn_chunks(B, A, NK):
    """Pieces the key range is cut into so that 8 heads x A attentions x B images x pieces is ~2048 workgroups (two waves each:
    ~4 waves per SIMD of the 256 CUs), never less than 64 keys a piece."""
    return max(1, min(-(-NK // 64), 2048 // (8 * A * B)))


def _attn_check(name, q, k, v, B, Q, NK, A, bits, allowed):
    for t in (q, k, v):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"{name} takes row-major 2-d float32 CUDA tensors (there is no CPU path)")
    if q.shape[0] != B * Q or k.shape[0] != B * NK or v.shape[0] != B * NK:
        raise ValueError(f"rows {q.shape[0]} / {k.shape[0]} / {v.shape[0]} do not match B {B}, Q {Q}, NK {NK}")
    if (bits is None) != (allowed is None):
        raise ValueError("bits and allowed come together")
    if bits is not None:
        W = (Q + 31) // 32
        if tuple(bits.shape) != (B, A, NK, W) or tuple(allowed.shape) != (B, A, W) or not bits.is_contiguous() or not allowed.is_contiguous() \
                or bits.dtype != torch.int32 or allowed.dtype != torch.int32:
            raise ValueError(f"bits {tuple(bits.shape)} / allowed {tuple(allowed.shape)} must be contiguous int32 [{B}, {A}, {NK}, {W}] / [{B}, {A}, {W}]")


def _attn_forward(name, want_lse, q, k, v, B, Q, NK, A, bits, allowed, chunks, out, scale, ws):
    """The forward of m2f_masked_attention (want_lse False -> (out, None)) and m2f_masked_attention_lse (-> (out, lse))."""
    _attn_check(name, q, k, v, B, Q, NK, A, bits, allowed)
    if chunks is None:
        chunks = m2f_attn_chunks(B, A, NK)
    if out is None:
        out = torch.empty((B * Q, A * 256), device=q.device, dtype=torch.float32)
    lse = torch.empty((B, A, 8, Q), device=q.device, dtype=torch.float32) if want_lse else None
    if ws is None and chunks > 1:
        ws = torch.empty(_lib.value("mss_m2f_attn_workspace_bytes", B, Q, A, chunks) // 4, device=q.device, dtype=torch.float32)
    args = (ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(bits), ptr(allowed), B, Q, NK, A,
            float(scale if scale is not None else 32 ** -0.5), chunks, ptr(ws), ptr(out), out.stride(0))
    if want_lse:
        call("mss_m2f_masked_attention_lse_f32", *args, ptr(lse))
    else:
        call("mss_m2f_masked_attention_f32", *args)
    return out, lse


def m2f_masked_attention(q, k, v, B, Q, NK, A=1, bits=None, allowed=None, chunks=None, out=None, scale=None, ws=None):
    """softmax(scale q k^T + mask) v for 8 heads of 32 channels and A attentions side by side: q [B*Q, >= A*256], k / v
    [B*NK, >= A*256] (row-major 2-d, attention a in columns a*256 ...), -> out [B*Q, A*256]. bits / allowed: from
    m2f_attn_mask_bits (or [B, A, NK, W] / [B, A, W] int32 made by hand); None = no mask. chunks: pieces of the key range
    (default m2f_attn_chunks); ws: the float32 chunk workspace (allocated here when None; its contents do not matter)."""
    return _attn_forward("m2f_masked_attention", False, q, k, v, B, Q, NK, A, bits, allowed, chunks, out, scale, ws)[0]


def m2f_masked_attention_lse(q, k, v, B, Q, NK, A=1, bits=None, allowed=None, chunks=None, out=None, scale=None, ws=None):
    """m2f_masked_attention for training: the same kernels (`out` has the same bits for the same arguments and chunk count) ->
    (out [B*Q, A*256], lse [B, A, 8, Q]); lse is the log-sum-exp of the scaled, masked scores in the log2 domain
    (include/mss_hip.h), which m2f_masked_attention_backward takes."""
    return _attn_forward("m2f_masked_attention_lse", True, q, k, v, B, Q, NK, A, bits, allowed, chunks, out, scale, ws)


def m2f_masked_attention_backward(q, k, v, out, lse, dout, B, Q, NK, A=1, bits=None, allowed=None, chunks=None, scale=None, ws=None,
                                  need=(True, True, True), grads=None):
    """Gradients of m2f_masked_attention_lse -> (dq [B*Q, A*256], dk, dv [B*NK, A*256]); an entry of `need` that is False is not
    computed (None). out / lse: what the forward returned; dout: the cotangent of out. grads: optional (dq, dk, dv) buffers to
    write into; ws: the float32 workspace (mss_m2f_attn_bwd_workspace_bytes). Neither needs zeroing: every element is assigned.
    No float atomics: the same bits every run for a given chunk count."""
    _attn_check("m2f_masked_attention_backward", q, k, v, B, Q, NK, A, bits, allowed)
    for t in (out, dout):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or tuple(t.shape) != (B * Q, A * 256):
            raise RuntimeError("m2f_masked_attention_backward takes row-major 2-d float32 CUDA tensors (there is no CPU path)")
    if tuple(lse.shape) != (B, A, 8, Q) or not lse.is_contiguous() or lse.dtype != torch.float32:
        raise ValueError(f"lse {tuple(lse.shape)} must be contiguous float32 [{B}, {A}, 8, {Q}]")
    if chunks is None:
        chunks = m2f_attn_chunks(B, A, NK)
    shapes = ((B * Q, A * 256), (B * NK, A * 256), (B * NK, A * 256))
    res = []
    for i in range(3):
        g = None
        if need[i]:
            g = grads[i] if grads is not None and grads[i] is not None else torch.empty(shapes[i], device=q.device, dtype=torch.float32)
            if tuple(g.shape) != shapes[i] or not g.is_contiguous() or g.dtype != torch.float32:
                raise ValueError(f"gradient buffer {i} must be contiguous float32 {shapes[i]}")
        res.append(g)
    if ws is None:
        ws = torch.empty(_lib.value("mss_m2f_attn_bwd_workspace_bytes", B, Q, A, chunks) // 4, device=q.device, dtype=torch.float32)
    call("mss_m2f_masked_attention_bwd_f32", ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(bits), ptr(allowed),
         ptr(out), out.stride(0), ptr(lse), ptr(dout), dout.stride(0), B, Q, NK, A, float(scale if scale is not None else 32 ** -0.5),
         chunks, ptr(ws), ptr(res[0]), ptr(res[1]), ptr(res[2]))
    return tuple(res)


class _MaskedAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, B, Q, NK, A, bits, allowed, chunks, scale):
        out, lse = m2f_masked_attention_lse(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed, chunks=chunks, scale=scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.masks = (bits, allowed)
        ctx.geom = (B, Q, NK, A, chunks, scale)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        B, Q, NK, A, chunks, scale = ctx.geom
        bits, allowed = ctx.masks
        dq, dk, dv = m2f_masked_attention_backward(q, k, v, out, lse, gout.contiguous(), B, Q, NK, A=A, bits=bits, allowed=allowed,
                                                   chunks=chunks, scale=scale, need=ctx.needs_input_grad[:3])
        return (dq, dk, dv) + (None,) * 8


def masked_attention(q, k, v, B, Q, NK, A=1, bits=None, allowed=None, chunks=None, scale=None):
    """Differentiable m2f_masked_attention: softmax(scale q k^T + mask) v for 8 heads of 32 channels and A attentions side by
    side, forward and backward on csrc/m2f_attn.hip. Gradients go to q, k and v (each computed only where asked for); bits /
    allowed are not differentiated. q / k / v may be column slices of wider row-major tensors."""
    return _MaskedAttentionFn.apply(q, k, v, B, Q, NK, A, bits, allowed, chunks, scale)


class _MaskLogitsFn(torch.autograd.Function):
    """logits[b] = feat[b] mask_embed[b]^T, pixel-major (m2f_mask_logits_act); backward: d mask_embed[b] = dlogits[b]^T feat[b] on the
    weight-gradient kernel, d feat[b] = dlogits[b] mask_embed[b] on the forward GEMM. The cotangent's padded query columns
    Q .. ldq-1 are dropped before either product."""

    @staticmethod
    def forward(ctx, mask_embed, feat, C, ldq):
        x = Act(feat, C=C)
        out = m2f_mask_logits_act(mask_embed, x, ldq)
        ctx.save_for_backward(mask_embed, feat)
        ctx.C = C
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        me, feat = ctx.saved_tensors
        B, Q, C = me.shape
        _, h, w, ld = feat.shape
        Qp = max(32, _round_up(Q, 16))
        dl = torch.zeros((B, h, w, Qp), device=g.device, dtype=torch.float32)
        dl[..., :Q] = g[..., :Q]
        dme = dfeat = None
        if ctx.needs_input_grad[0]:
            dme = torch.empty((B, Q, C), device=g.device, dtype=torch.float32)
            for b in range(B):
                gw = conv2d_wgrad(Act(feat[b:b + 1], C=C), Act(dl[b:b + 1]), Qp, C, 1, 1)
                dme[b] = gw.view(Qp, C)[:Q]
        if ctx.needs_input_grad[1]:
            dfeat = torch.empty_like(feat) if ld == C else torch.zeros_like(feat)
            mt = torch.zeros((B, C, Qp), device=g.device, dtype=torch.float32)
            mt[:, :, :Q] = me.detach().transpose(1, 2)
            for b in range(B):
                conv2d(Act(dl[b:b + 1]), pack_weight(mt[b].view(C, Qp, 1, 1)), out=Act(dfeat[b:b + 1], C=C))
        return dme, dfeat, None, None


def mask_logits(mask_embed, feat, ldq):
    """Differentiable m2f_mask_logits_act: mask_embed [B, Q, C] x feat (an Act [B, h, w, C] over a tensor that may require grad) ->
    pixel-major logits [B, h, w, ldq], with the forward's bits. Both gradients run on the MFMA GEMM / weight-gradient kernels."""
    if not mask_embed.is_cuda or not feat.buf.is_cuda:
        raise RuntimeError("mask_logits runs on an MI355X only (float32 CUDA tensors); there is no CPU path")
    if feat.c0 != 0:
        raise ValueError("mask_logits takes an Act that starts at channel 0 of its buffer")
    return _MaskLogitsFn.apply(mask_embed, feat.buf, feat.C, ldq)


class _NchwToRowsFn(torch.autograd.Function):
    """nchw_to_act as an autograd node -> the Act's buffer [N, H, W, Cp]; backward: nhwc_to_nchw of the first C channels."""

    @staticmethod
    def forward(ctx, t):
        ctx.c = t.shape[1]
        return nchw_to_act(t).buf

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return nhwc_to_nchw(Act(g.contiguous(), C=ctx.c))


class _RowsToNchwFn(torch.autograd.Function):
    """nhwc_to_nchw of the first C channels of [N, H, W, ld] as an autograd node; backward: the zero-padded inverse."""

    @staticmethod
    def forward(ctx, buf, C):
        ctx.ld = buf.shape[-1]
        return nhwc_to_nchw(Act(buf, C=C))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return nchw_to_act(g, Cp=ctx.ld).buf, None


def m2f_score_fused(class_logits, mask_logits_nhwc, image_size, size=None):
    """Anomaly score from LOW-resolution pixel-major mask logits [B,hm,wm,Q]: bilinear upsample to `image_size`
    (align_corners=False, maskformer_model.py:264-277) + train_m2f.py:387-407, cropped to `size` -> [B,H,W]."""
    B, Q, C1 = class_logits.shape
    Bm, hm, wm, ldq = mask_logits_nhwc.shape
    Hi, Wi = image_size
    H, W = size if size is not None else image_size
    cls = class_logits.contiguous().float()
    lg = mask_logits_nhwc.contiguous()
    out = torch.empty((B, H, W), device=cls.device, dtype=torch.float32)
    prob = torch.empty((B, Q, 32), device=cls.device, dtype=torch.float32)      # class-probability table of the MFMA kernel
    call("mss_m2f_fused_score_ws_f32", ptr(cls), ptr(lg), B, Q, C1 - 1, hm, wm, ldq, Hi, Wi, H, W, ptr(out), ptr(prob))
    return out


# ---- what the Mask2Former matcher, criterion and class mix share -----------------------------------------------------------------
def _need_f32_cuda(name, *tensors):
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"{name} runs on an MI355X only (float32 CUDA tensors); there is no CPU path")


def _steps(tensors):
    """One tensor (= one prediction step) or a list of them -> list."""
    return [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)


def _m2f_table(table, tensors):
    """Fill a 16-slot per-step pointer table of include/mss_hip.h (MssM2fMaps / MssM2fSteps / MssM2fGrads) from contiguous tensors,
    which the caller keeps alive. A longer list fills the 16 slots only: the entry point refuses its S (MSS_ERR_UNSUPPORTED)."""
    for s, t in enumerate(tensors[:_lib.MSS_M2F_MAX_STEPS]):
        table.step[s] = t.data_ptr()
    return table


def _m2f_layout(name, shape, pixel_major, Q):
    """Shape of mask logits, NCHW [B,Q,h,w] or with pixel_major [B,h,w,ldq] (Q <= ldq, default ldq) -> ((image, query, pixel) strides
    in floats, B, Q, h, w, ldq)."""
    if pixel_major:
        B, h, w, ldq = shape
        strides = (h * w * ldq, 1, ldq)
    else:
        B, ldq, h, w = shape
        strides = (h * w * ldq, h * w, 1)
    Q = ldq if Q is None else int(Q)
    if Q < 1 or Q > ldq or (not pixel_major and Q != ldq):
        raise ValueError(f"{name}: Q {Q} does not fit mask logits {tuple(shape)}")
    return strides, B, Q, h, w, ldq


def _m2f_maps(name, mask_logits, pixel_major, Q):
    """The mask logits of the S prediction steps of a call -> (a filled MssM2fMaps, the contiguous tensors its pointers belong to)."""
    masks = _steps(mask_logits)
    _need_f32_cuda(name, *masks)
    masks = [m.contiguous() for m in masks]
    if masks[0].dim() != 4 or any(m.shape != masks[0].shape for m in masks):
        raise ValueError(f"{name}: the mask logits of all steps share one 4-d shape, got {[tuple(m.shape) for m in masks]}")
    strides, B, Q, h, w, _ = _m2f_layout(name, masks[0].shape, pixel_major, Q)
    mp = _lib.MssM2fMaps(img_stride=strides[0], query_stride=strides[1], pixel_stride=strides[2], S=len(masks), B=B, Q=Q, h=h, w=w)
    return _m2f_table(mp, masks), masks


def _m2f_targets(name, S, B, tstart, tmask=None, labels=None, match=None, more=()):
    """The target pack of a call -- tmask uint8 [sum T,H,W] and / or labels int32 [sum T], tstart int32 [B+1] -- and, where the call
    has one, the matcher's table match int32 [S,B,Tmax] -> (a filled MssM2fTargets, the contiguous tensors its pointers belong to,
    match contiguous). `more`: further tensors of the call that only have to be on the device."""
    ints = [t for t in (tstart, labels, match) if t is not None]
    for t in ([] if tmask is None else [tmask]) + ints + list(more):
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on an MI355X only (CUDA tensors); there is no CPU path")
    if (tmask is not None and tmask.dtype != torch.uint8) or any(t.dtype != torch.int32 for t in ints):
        raise RuntimeError(f"{name} takes uint8 target masks and int32 tstart / labels / match on the device")
    total_t = labels.numel() if tmask is None else tmask.shape[0]
    if (tmask is not None and tmask.dim() != 3) or tstart.numel() != B + 1 or (labels is not None and labels.numel() != total_t) \
            or (match is not None and (match.dim() != 3 or tuple(match.shape[:2]) != (S, B) or match.shape[2] < 1)):
        raise ValueError(f"{name}: tmask {None if tmask is None else tuple(tmask.shape)} / tstart {tuple(tstart.shape)} / labels "
                         f"{None if labels is None else tuple(labels.shape)} / match {None if match is None else tuple(match.shape)} "
                         f"do not match S {S}, B {B}")
    H, W = (0, 0) if tmask is None else tmask.shape[1:]
    keep = tuple(None if t is None else t.contiguous() for t in (tmask, tstart, labels))
    tg = _lib.MssM2fTargets(ptr(keep[0]) if total_t else None, ptr(keep[1]), ptr(keep[2]) if total_t else None, total_t, H, W)
    return tg, keep, None if match is None else match.contiguous()


# ---- Hungarian matching of Mask2Former (csrc/m2f_match.hip) ---------------------------------------------------------------------
def _match_ints(S, B, Tmax, device):
    """match [S,B,Tmax] and status [S,B] as views of ONE int32 buffer (one device-to-host copy brings both), pre-filled: integer
    buffers are never handed out uninitialised (tests/poison.py)."""
    buf = torch.full((S * B * (Tmax + 1),), -1, device=device, dtype=torch.int32)
    return buf, buf[:S * B * Tmax].view(S, B, Tmax), buf[S * B * Tmax:].view(S, B)


def m2f_match_cost(mask_logits, class_logits, tmask, tstart, labels, point_coords, weights=(1.0, 1.0, 1.0), Tmax=None,
                   pixel_major=False, solve=False):
    """The matching cost of matcher.py:105-148 for S prediction steps x B images in two launches. mask_logits / class_logits:
    lists of S tensors (or one tensor = one step): NCHW [B,Q,h,w], or with pixel_major the decoder's [B,h,w,ldq]
    (m2f_mask_logits_act; ldq >= Q) / [B,Q,C+1]. tmask uint8 [sum T,H,W], labels int32 [sum T], tstart int32 [B+1] (device);
    point_coords [S,B,P,2] (x, y) in [0,1); weights = (cost_class, cost_mask, cost_dice); Tmax >= max T_b (host int, default
    sum T). -> cost [S,B,Q,Tmax] fp32 (columns >= T_b are 0); with solve also (match [S,B,Tmax], status [S,B], their shared
    int32 buffer) from the same second launch."""
    name = "m2f_match_cost"
    clss = _steps(class_logits)
    _need_f32_cuda(name, *clss, point_coords)
    B, Q, C1 = clss[0].shape
    mp, masks = _m2f_maps(name, mask_logits, pixel_major, Q)
    tg, keep, _ = _m2f_targets(name, len(clss), B, tstart, tmask=tmask, labels=labels)
    S = len(masks)
    clss = [c.contiguous() for c in clss]
    if len(clss) != S or masks[0].shape[0] != B or any(c.shape != clss[0].shape for c in clss):
        raise ValueError(f"{S} mask logits {tuple(masks[0].shape)} do not match {len(clss)} class logits {tuple(clss[0].shape)}")
    P = point_coords.shape[2]
    if tuple(point_coords.shape) != (S, B, P, 2):
        raise ValueError(f"point_coords {tuple(point_coords.shape)} does not match S {S}, B {B}")
    Tmax = max(1, tg.total_t if Tmax is None else int(Tmax))
    dev = clss[0].device
    nbytes = _lib.value("mss_m2f_match_workspace_bytes", S, B, Q, Tmax, P)
    if nbytes <= 0:
        raise _lib.MssError(f"m2f_match_cost: unsupported shape S {S}, Q {Q}, Tmax {Tmax} (S <= 16, T <= Q <= 128)")
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
    cost = torch.empty((S, B, Q, Tmax), device=dev, dtype=torch.float32)
    buf = match = status = None
    if solve:
        buf, match, status = _match_ints(S, B, Tmax, dev)
    pts = point_coords.contiguous()
    call("mss_m2f_match_cost_f32", ctypes.byref(mp), ctypes.byref(_m2f_table(_lib.MssM2fSteps(), clss)), ctypes.byref(tg), ptr(pts), C1, P, Tmax,
         float(weights[0]), float(weights[1]), float(weights[2]), ptr(ws), ptr(cost), ptr(match), ptr(status))
    return (cost, match, status, buf) if solve else cost


def m2f_match_assign(cost, tcount):
    """linear_sum_assignment (matcher.py:151) of every [Q, T_b] block of cost [S,B,Q,Tmax] fp32 on the device, one wave per
    problem, float64 shortest augmenting paths; tcount: T_b per image (int32 device tensor [B], or a list). -> (match [S,B,Tmax]
    int32: the query of target m, -1 in the padding; status [S,B] int32: 0 solved, 1 = scipy's ValueError case)."""
    if not cost.is_cuda or cost.dtype != torch.float32 or cost.dim() != 4:
        raise RuntimeError("m2f_match_assign runs on an MI355X only (a float32 CUDA tensor [S,B,Q,Tmax]); there is no CPU path")
    S, B, Q, Tmax = cost.shape
    if not isinstance(tcount, torch.Tensor):
        tcount = torch.tensor([int(t) for t in tcount], device=cost.device, dtype=torch.int32)
    if not tcount.is_cuda or tcount.dtype != torch.int32 or tcount.numel() != B:
        raise ValueError(f"tcount must be {B} int32 counts on the device")
    if Q > 128 or Tmax > 128 or Tmax < 1:
        raise NotImplementedError(f"m2f_match_assign: Q {Q} / Tmax {Tmax} outside 1..128")
    _, match, status = _match_ints(S, B, Tmax, cost.device)
    call("mss_m2f_match_assign_f32", ptr(cost.contiguous()), ptr(tcount.contiguous()), S, B, Q, Tmax, ptr(match), ptr(status))
    return match, status


# ---- Mask2Former targets from label maps (csrc/m2f_targets.hip) ----------------------------------------------------------------
_SEM_DTYPES = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}


def _targets_sem(name, sem, label_threshold):
    if not isinstance(sem, torch.Tensor) or not sem.is_cuda:
        raise RuntimeError(f"{name} runs on an MI355X only (a CUDA label map); there is no CPU path")
    if sem.dtype not in _SEM_DTYPES:
        raise RuntimeError(f"{name} takes int64, int32 or uint8 label maps, got {sem.dtype}")
    if sem.dim() != 3 or sem.numel() == 0:
        raise ValueError(f"{name}: the label maps are [B,H,W] with no empty dimension, got {tuple(sem.shape)}")
    if not 1 <= int(label_threshold) <= 128:
        raise NotImplementedError(f"{name}: label_threshold {label_threshold} outside 1..128")
    return sem.contiguous(), _SEM_DTYPES[sem.dtype]


def m2f_targets_count(sem, label_threshold=100):
    """Which classes each label map holds (train_m2f.py:355-357: np.unique, `classes < label_threshold`), two launches, nothing read
    back. sem [B,H,W] int64 / int32 / uint8 on the device; a class is a value in [0, label_threshold), label_threshold <= 128.
    -> (tstart int32 [B+1], labels_buf int32 [B * label_threshold]: image b's classes ascending from tstart[b], the entries past
    tstart[B] are 0; rank int32 [B, label_threshold]: the row of class v inside image b or -1; present int64 [B,2]: the 128-bit
    class set of image b)."""
    name = "m2f_targets_count"
    sem, nbytes = _targets_sem(name, sem, label_threshold)
    B, H, W = sem.shape
    thr = int(label_threshold)
    dev = sem.device
    # integer buffers are never handed out uninitialised (tests/poison.py)
    tstart = torch.zeros(B + 1, device=dev, dtype=torch.int32)
    labels = torch.zeros(B * thr, device=dev, dtype=torch.int32)
    rank = torch.full((B, thr), -1, device=dev, dtype=torch.int32)
    present = torch.zeros((B, 2), device=dev, dtype=torch.int64)
    call("mss_m2f_targets_from_labels", ptr(sem), nbytes, B, H, W, H, W, thr, 255, 0, ptr(present), ptr(tstart), ptr(labels), ptr(rank), 0,
         None, None)
    return tstart, labels, rank, present


def m2f_targets_fill(sem, tstart, rank, total_t, padded_size, label_threshold=100, ignore_label=255, tmask=None, ood=None):
    """The target masks and the OOD map of train_m2f.py:360-361 (`sem_seg == class_id`, `(sem_seg > label_threshold) & (sem_seg !=
    ignore_label)`), zero padded to padded_size = (Hp, Wp) (maskformer_model.py:316-339), in one launch that writes every byte of
    both. tstart / rank: m2f_targets_count's; total_t: tstart[B] as a host int. tmask uint8 [total_t,Hp,Wp] / ood uint8 [B,Hp,Wp]:
    buffers of the caller's to write into (default: new ones). -> (tmask, ood)."""
    name = "m2f_targets_fill"
    sem, nbytes = _targets_sem(name, sem, label_threshold)
    B, H, W = sem.shape
    thr, total_t = int(label_threshold), int(total_t)
    Hp, Wp = (int(v) for v in padded_size)
    dev = sem.device
    for t in (tstart, rank) + tuple(o for o in (tmask, ood) if o is not None):
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on an MI355X only (CUDA tensors); there is no CPU path")
    if tstart.dtype != torch.int32 or rank.dtype != torch.int32 or any(o is not None and o.dtype != torch.uint8 for o in (tmask, ood)):
        raise RuntimeError(f"{name} takes int32 tstart / rank and uint8 tmask / ood on the device")
    if tstart.numel() != B + 1 or tuple(rank.shape) != (B, thr):
        raise ValueError(f"{name}: tstart {tuple(tstart.shape)} / rank {tuple(rank.shape)} do not match B {B}, label_threshold {thr}")
    if Hp < H or Wp < W or not 0 <= total_t <= B * thr:
        raise ValueError(f"{name}: padded size {(Hp, Wp)} / total_t {total_t} do not fit label maps {tuple(sem.shape)}")
    if tmask is None:
        tmask = torch.zeros((total_t, Hp, Wp), device=dev, dtype=torch.uint8)
    if ood is None:
        ood = torch.zeros((B, Hp, Wp), device=dev, dtype=torch.uint8)
    if tuple(tmask.shape) != (total_t, Hp, Wp) or tuple(ood.shape) != (B, Hp, Wp) or not tmask.is_contiguous() or not ood.is_contiguous():
        raise ValueError(f"{name}: tmask {tuple(tmask.shape)} / ood {tuple(ood.shape)} must be contiguous [{total_t},{Hp},{Wp}] / [{B},{Hp},{Wp}]")
    call("mss_m2f_targets_from_labels", ptr(sem), nbytes, B, H, W, Hp, Wp, thr, int(ignore_label), 1, None, ptr(tstart.contiguous()), None,
         ptr(rank.contiguous()), total_t, ptr(tmask) if total_t else None, ptr(ood))
    return tmask, ood


# ---- SetCriterion of Mask2Former: class and sampled-mask losses (csrc/m2f_loss.hip) -----------------------------------------------
_LOSS_MODES = {"uncertain": 1, "clean": 2}


def _loss_ws(R, K, P, device):
    nbytes = _lib.value("mss_m2f_loss_workspace_bytes", R, K, P)
    return torch.empty(max(1, nbytes // 4), device=device, dtype=torch.float32)


def _loss_groups(name, scales, split, total_t):
    """(scale0,) = one group of rows (loss_masks), (scale0, scale1) + split = two (loss_masks_aug) -> (split, scale0, scale1, ncols)."""
    scales = tuple(float(v) for v in scales)
    if len(scales) == 1:
        return total_t, scales[0], 0.0, 3
    if len(scales) != 2 or split is None or not 0 <= int(split) <= total_t:
        raise ValueError(f"{name}: scales {scales} / split {split} for {total_t} targets")
    return int(split), scales[0], scales[1], 5


def m2f_point_select(mask_logits, tmask, tstart, match, candidates, random_points, k, num_points, mode="uncertain", sel_start=0,
                     pixel_major=False, Q=None):
    """The sampled points of every matched mask (criterion.py:335-341 = detectron2's get_uncertain_point_coords_with_randomness,
    mode "uncertain": key -|x|; :371-407, mode "clean": key -BCEWithLogits(x, t); :365-369 for the rows before sel_start) in one
    launch. mask_logits: list of S tensors, NCHW [B,Q,h,w] or with pixel_major [B,h,w,ldq] (then Q <= ldq); tmask uint8
    [sum T,H,W], tstart int32 [B+1], match int32 [S,B,Tmax] (the matcher's device table). Row r = s * sum T + g (target g).
    candidates [S, sum T - sel_start, K, 2] ((x, y) in [0,1); None where k == 0): a row with g >= sel_start keeps its k candidates
    with the largest key, in ascending candidate index -- ties at the k-th largest go to the lowest index, -0.0 == +0.0, a NaN key
    ranks last -- followed by the first num_points - k of random_points [S * sum T, Pr, 2]; a row before sel_start takes its
    first num_points random points. -> points [S * sum T, num_points, 2]; all 0 for a row whose table entry is -1."""
    name = "m2f_point_select"
    mp, masks = _m2f_maps(name, mask_logits, pixel_major, Q)
    _need_f32_cuda(name, *[t for t in (candidates, random_points) if t is not None])
    tg, keep, mt = _m2f_targets(name, mp.S, mp.B, tstart, tmask=tmask, match=match)
    S, total_t = mp.S, tg.total_t
    P, k, sel_start = int(num_points), int(k), int(sel_start)
    if mode not in _LOSS_MODES:
        raise ValueError(f"{name}: mode {mode!r} is not one of {sorted(_LOSS_MODES)}")
    R = S * total_t
    K = 0
    if k > 0:
        if candidates is None or candidates.dim() != 4 or tuple(candidates.shape[:2]) != (S, total_t - sel_start) or candidates.shape[3] != 2:
            raise ValueError(f"{name}: candidates {None if candidates is None else tuple(candidates.shape)} for S {S}, {total_t - sel_start} selecting targets")
        K = candidates.shape[2]
    need = P if (sel_start > 0 or k == 0) else P - k
    Pr = 0
    if random_points is not None:
        if random_points.shape[-1] != 2 or random_points.numel() != R * random_points.shape[-2] * 2:
            raise ValueError(f"{name}: random_points {tuple(random_points.shape)} for {R} rows")
        Pr = random_points.shape[-2]
    if P < 1 or k < 0 or k > min(K, P) or not 0 <= sel_start <= total_t or Pr < need:
        raise ValueError(f"{name}: num_points {P}, k {k}, K {K}, sel_start {sel_start}, {Pr} random points per row ({need} needed)")
    dev = masks[0].device
    points = torch.empty((R, P, 2), device=dev, dtype=torch.float32)
    ws = _loss_ws(R, K, P, dev)
    cand = candidates.contiguous() if k > 0 else None
    rnd = random_points.contiguous() if random_points is not None else None
    call("mss_m2f_loss_select_f32", ctypes.byref(mp), ctypes.byref(tg), ptr(mt), ptr(cand), ptr(rnd), mt.shape[2], K, k, P, Pr, _LOSS_MODES[mode],
         sel_start, ptr(ws), ptr(points))
    return points


def m2f_mask_loss(mask_logits, tmask, tstart, match, points, pixel_major=False, Q=None):
    """The four sums both mask losses need (criterion.py:343-358, sigmoid_ce_loss :49-66, dice_loss :22-41) of every row at its
    points [S * sum T, P, 2]: -> rows [S * sum T, 4] float64 = sum_p BCEWithLogits(x, t), sum_p sigmoid(x) t, sum_p sigmoid(x),
    sum_p t (NaN for a row whose table entry is -1), x / t = the source / target map sampled bilinearly. One launch, one order."""
    name = "m2f_mask_loss"
    mp, masks = _m2f_maps(name, mask_logits, pixel_major, Q)
    tg, keep, mt = _m2f_targets(name, mp.S, mp.B, tstart, tmask=tmask, match=match, more=(points,))
    R = mp.S * tg.total_t
    if points.dtype != torch.float32 or points.dim() != 3 or points.shape[0] != R or points.shape[2] != 2 or points.shape[1] < 1:
        raise ValueError(f"{name}: points {tuple(points.shape)} {points.dtype} for {R} rows")
    rows = torch.empty((R, 4), device=masks[0].device, dtype=torch.float64)
    call("mss_m2f_loss_mask_forward_f32", ctypes.byref(mp), ctypes.byref(tg), ptr(mt), ptr(points.contiguous()), mt.shape[2], points.shape[1],
         ptr(rows))
    return rows


def m2f_label_loss(class_logits, labels, tstart, match, weight, rows, num_points, scales, split=None):
    """loss_labels (criterion.py:189-205) of S steps and the fold of the row table into the per-step mask losses (:301-306,
    :356-359), one workgroup per step. class_logits: list of S [B,Q,C+1]; labels int32 [sum T]; weight [C+1] (empty_weight);
    rows: m2f_mask_loss's table (None: no mask losses, their columns are 0). scales = (1 / num_masks,) -> loss [S,3] =
    (loss_ce, loss_mask, loss_dice); scales = (2 / n_original, 1 / n_aug) with split = the first target of the aug half ->
    loss [S,5] = (loss_ce, loss_original_mask, loss_original_dice, loss_aug_mask, loss_aug_dice). Also returns tclass [S,B,Q]
    int32 (target_classes), bad [S] int32 (1: a table entry of -1 or a label outside the classes; the step's losses are NaN) and
    wsum [S] float64 (sum of the class weights): what m2f_label_loss_backward / m2f_mask_loss_backward take."""
    name = "m2f_label_loss"
    clss = _steps(class_logits)
    _need_f32_cuda(name, *clss, weight)
    clss = [c.contiguous() for c in clss]
    S = len(clss)
    if clss[0].dim() != 3 or any(c.shape != clss[0].shape for c in clss):
        raise ValueError(f"{name}: the class logits of all steps share one [B,Q,C+1] shape, got {[tuple(c.shape) for c in clss]}")
    B, Q, C1 = clss[0].shape
    tg, keep, mt = _m2f_targets(name, S, B, tstart, labels=labels, match=match)
    total_t = tg.total_t
    if weight.numel() != C1 or C1 < 2:
        raise ValueError(f"{name}: weight {tuple(weight.shape)} does not match C+1 {C1}")
    split, scale0, scale1, ncols = _loss_groups(name, scales, split, total_t)
    dev = clss[0].device
    if rows is None:
        rows = torch.zeros((S * total_t, 4), device=dev, dtype=torch.float64)
        scale0 = scale1 = 0.0
    if not rows.is_cuda or rows.dtype != torch.float64 or tuple(rows.shape) != (S * total_t, 4):
        raise ValueError(f"{name}: rows {tuple(rows.shape)} {rows.dtype} for {S * total_t} rows")
    tclass = torch.full((S, B, Q), C1 - 1, device=dev, dtype=torch.int32)
    bad = torch.zeros((S,), device=dev, dtype=torch.int32)
    wsum = torch.empty((S,), device=dev, dtype=torch.float64)
    loss = torch.empty((S, ncols), device=dev, dtype=torch.float32)
    call("mss_m2f_loss_finalize_f32", ctypes.byref(_m2f_table(_lib.MssM2fSteps(), clss)), ctypes.byref(tg), ptr(mt), ptr(weight.contiguous()),
         ptr(rows.contiguous()) if total_t else None, S, B, Q, C1, mt.shape[2], int(num_points), split, scale0, scale1, ncols, ptr(tclass), ptr(bad),
         ptr(wsum), ptr(loss))
    return loss, tclass, bad, wsum


def m2f_mask_loss_backward(mask_logits, tmask, tstart, match, bad, points, rows, gloss, scales, split=None, pixel_major=False, Q=None):
    """d / d mask_logits of m2f_label_loss's mask columns: gloss [S,ncols] fp32 is the upstream gradient of its loss table.
    -> one tensor [S, *mask_logits[0].shape] (step s = its slice) in the layout of the input: the map of every matched query
    is written whole by its row's workgroup from an int64 fixed-point window (no float atomics: bit-reproducible), every other
    element -- unmatched queries, the padding columns of a pixel-major layout, the steps marked bad -- is 0."""
    name = "m2f_mask_loss_backward"
    mp, masks = _m2f_maps(name, mask_logits, pixel_major, Q)
    S = mp.S
    tg, keep, mt = _m2f_targets(name, S, mp.B, tstart, tmask=tmask, match=match, more=(bad, points, rows, gloss))
    total_t = tg.total_t
    R = S * total_t
    split, scale0, scale1, ncols = _loss_groups(name, scales, split, total_t)
    if points.dtype != torch.float32 or points.dim() != 3 or points.shape[0] != R or points.shape[2] != 2 or points.shape[1] < 1 \
            or rows.dtype != torch.float64 or tuple(rows.shape) != (R, 4) or gloss.dtype != torch.float32 or tuple(gloss.shape) != (S, ncols) \
            or bad.dtype != torch.int32 or bad.numel() != S:
        raise ValueError(f"{name}: points {tuple(points.shape)} / rows {tuple(rows.shape)} / gloss {tuple(gloss.shape)} / bad {tuple(bad.shape)} "
                         f"do not match {R} rows, S {S}, {ncols} loss columns")
    P = points.shape[1]
    dev = masks[0].device
    grads = torch.zeros((S,) + tuple(masks[0].shape), device=dev, dtype=torch.float32)
    ws = _loss_ws(R, 0, P, dev)
    call("mss_m2f_loss_mask_backward_f32", ctypes.byref(mp), ctypes.byref(tg), ptr(mt), ptr(bad.contiguous()), ptr(points.contiguous()),
         ptr(rows.contiguous()), ptr(gloss.contiguous()), mt.shape[2], P, split, scale0, scale1, ncols, ptr(ws),
         ctypes.byref(_m2f_table(_lib.MssM2fGrads(), list(grads))))
    return grads


def m2f_label_loss_backward(class_logits, tclass, bad, weight, wsum, gloss):
    """d loss_ce / d class_logits: -> [S,B,Q,C+1] = weight[c] / wsum (softmax - onehot) gloss[s,0] (0 for a step marked bad);
    tclass / bad / wsum from m2f_label_loss, gloss [S,ncols] the upstream gradient of its loss table."""
    name = "m2f_label_loss_backward"
    clss = _steps(class_logits)
    _need_f32_cuda(name, *clss, weight, gloss)
    if not (tclass.is_cuda and bad.is_cuda and wsum.is_cuda):
        raise RuntimeError(f"{name} runs on an MI355X only (CUDA tensors); there is no CPU path")
    clss = [c.contiguous() for c in clss]
    S = len(clss)
    B, Q, C1 = clss[0].shape
    if any(c.shape != clss[0].shape for c in clss) or tuple(tclass.shape) != (S, B, Q) or tclass.dtype != torch.int32 or bad.dtype != torch.int32 \
            or bad.numel() != S or wsum.dtype != torch.float64 or wsum.numel() != S or weight.numel() != C1 or gloss.dim() != 2 \
            or gloss.shape[0] != S or gloss.shape[1] not in (3, 5):
        raise ValueError(f"{name}: tclass {tuple(tclass.shape)} / bad {tuple(bad.shape)} / wsum {tuple(wsum.shape)} / gloss {tuple(gloss.shape)} "
                         f"do not match {S} class logits {tuple(clss[0].shape)}")
    grads = torch.empty((S, B, Q, C1), device=clss[0].device, dtype=torch.float32)
    call("mss_m2f_loss_label_backward_f32", ctypes.byref(_m2f_table(_lib.MssM2fSteps(), clss)), ptr(tclass.contiguous()), ptr(bad.contiguous()),
         ptr(weight.contiguous()), ptr(wsum.contiguous()), ptr(gloss.contiguous()), S, B, Q, C1, gloss.shape[1],
         ctypes.byref(_m2f_table(_lib.MssM2fGrads(), list(grads))))
    return grads


# ---- SetCriterion.loss_ood, RCL branch: the class mix, forward and backward (csrc/m2f_mix.hip) ----------------------------------------
_MIX_MODES = {"logits": 0, "neg_max": 1}
MIX_LOGIT_CHANNELS = 19             # criterion.py:166: logits[:, :19]
MIX_MAX_QUERIES, MIX_MAX_CLASSES = 128, 32


def _mix_inputs(name, class_logits, mask_logits, pixel_major, Q):
    """Class logits [B,Q,C+1] and mask logits (NCHW [B,Q,h,w], or pixel-major [B,h,w,ldq]) -> (both contiguous, the (image,
    query, pixel) strides, B, Q, C, h, w)."""
    _need_f32_cuda(name, class_logits, mask_logits)
    cls, x = class_logits.contiguous(), mask_logits.contiguous()
    if cls.dim() != 3 or x.dim() != 4 or x.shape[0] != cls.shape[0]:
        raise ValueError(f"{name}: class logits {tuple(cls.shape)} / mask logits {tuple(x.shape)}")
    B, Qc, C1 = cls.shape
    strides, B, Q, h, w, ldq = _m2f_layout(name, x.shape, pixel_major, Qc if Q is None and pixel_major else Q)
    if pixel_major and ldq % 4:
        raise ValueError(f"{name}: the pitch {ldq} of pixel-major mask logits is no multiple of 4")
    C = C1 - 1
    if Q != Qc or not 1 <= Q <= MIX_MAX_QUERIES or not 1 <= C <= MIX_MAX_CLASSES or h < 1 or w < 1:
        raise ValueError(f"{name}: {Qc} queries x {C} classes of class logits, Q {Q} of mask logits {tuple(x.shape)} "
                         f"(Q <= {MIX_MAX_QUERIES}, 1 <= C <= {MIX_MAX_CLASSES})")
    return cls, x, strides, B, Q, C, h, w


def _mix_sizes(name, mix, size, crop):
    _need_f32_cuda(name, mix)
    if mix.dim() != 4:
        raise ValueError(f"{name}: mix {tuple(mix.shape)} is not [B,C,h,w]")
    (H, W), (Ht, Wt) = (int(v) for v in size), (int(v) for v in (size if crop is None else crop))
    if not (1 <= Ht <= H and 1 <= Wt <= W):
        raise ValueError(f"{name}: crop {(Ht, Wt)} does not lie inside size {(H, W)}")
    return H, W, Ht, Wt


def m2f_class_mix(class_logits, mask_logits, pixel_major=False, Q=None):
    """The class mix of loss_ood at the low resolution (criterion.py:133-138): -> (mix [B,C,h,w] = einsum("bqc,bqhw->bchw",
    softmax(class_logits, -1)[..., :-1], sigmoid(mask_logits)), prob [B,Q,C] = that softmax, which m2f_class_mix_backward reuses).
    class_logits [B,Q,C+1]; mask_logits NCHW [B,Q,h,w], or with pixel_major [B,h,w,ldq] (ldq % 4 == 0; the columns Q..ldq-1 are
    never read). Q <= 128, 1 <= C <= 32. The queries are summed in index order: both layouts give the same bits."""
    name = "m2f_class_mix"
    cls, x, strides, B, Q, C, h, w = _mix_inputs(name, class_logits, mask_logits, pixel_major, Q)
    prob = torch.empty((B, Q, C), device=x.device, dtype=torch.float32)
    mix = torch.empty((B, C, h, w), device=x.device, dtype=torch.float32)
    call("mss_m2f_mix_forward_f32", ptr(cls), ptr(x), strides[0], strides[1], strides[2], B, Q, C, h, w, ptr(prob), ptr(mix))
    return mix, prob


def m2f_mix_upsample(mix, size, crop=None, mode="logits"):
    """F.interpolate(mix, size=(H, W), mode="bilinear", align_corners=False)[:, :, :Ht, :Wt] (criterion.py:166-168, :177-179) without
    the uncropped tensor. mode "logits": the first min(C, 19) channels -> [B,Cl,Ht,Wt] contiguous, what RelContrastiveLoss takes;
    "neg_max": -max over all C channels (:181) -> [B,Ht,Wt]; the C full-size channels are never stored. The scale is h / H."""
    name = "m2f_mix_upsample"
    H, W, Ht, Wt = _mix_sizes(name, mix, size, crop)
    if mode not in _MIX_MODES:
        raise ValueError(f"{name}: mode {mode!r} is not one of {sorted(_MIX_MODES)}")
    mix = mix.contiguous()
    B, C, h, w = mix.shape
    shape = (B, Ht, Wt) if mode == "neg_max" else (B, min(C, MIX_LOGIT_CHANNELS), Ht, Wt)
    out = torch.empty(shape, device=mix.device, dtype=torch.float32)
    call("mss_m2f_mix_upsample_f32", ptr(mix), B, C, h, w, H, W, Ht, Wt, _MIX_MODES[mode], ptr(out))
    return out


def m2f_mix_upsample_backward(mix, size, crop=None, dlogits=None, dscore=None):
    """d / d mix of m2f_mix_upsample: dlogits [B,Cl,Ht,Wt] is the upstream gradient of its "logits" output, dscore [B,Ht,Wt] that of
    "neg_max"; either or both. -> dmix [B,C,h,w], written whole: a low-resolution pixel sums, rows then columns ascending, over the
    output pixels of the crop whose taps contain it. For dscore the C interpolated values are recomputed per output pixel and
    -dscore goes to the largest; among equal values the lowest class index takes it (torch.max leaves that unspecified)."""
    name = "m2f_mix_upsample_backward"
    H, W, Ht, Wt = _mix_sizes(name, mix, size, crop)
    mix = mix.contiguous()
    B, C, h, w = mix.shape
    Cl = min(C, MIX_LOGIT_CHANNELS)
    for t, shape in ((dlogits, (B, Cl, Ht, Wt)), (dscore, (B, Ht, Wt))):
        if t is None:
            continue
        _need_f32_cuda(name, t)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: an upstream gradient {tuple(t.shape)} where {shape} belongs")
    if dlogits is None and dscore is None:
        raise ValueError(f"{name}: neither dlogits nor dscore")
    dmix = torch.empty_like(mix)
    call("mss_m2f_mix_upsample_backward_f32", ptr(dlogits.contiguous() if dlogits is not None else None),
         ptr(dscore.contiguous() if dscore is not None else None), ptr(mix), B, C, h, w, H, W, Ht, Wt, ptr(dmix))
    return dmix


def m2f_class_mix_backward(dmix, prob, class_logits, mask_logits, pixel_major=False, Q=None, want_dmasks=True):
    """d / d (mask_logits, class_logits) of m2f_class_mix from dmix [B,C,h,w]; prob is its second result. -> (dmasks in the layout
    of mask_logits, every pad column Q..ldq-1 of a pixel-major layout 0; dcls [B,Q,C+1]). dmasks = sigmoid'(x) sum_c prob dmix;
    dcls = the softmax backward, with the dropped column, of dP[b,q,c] = sum_p dmix[b,c,p] sigmoid(x[b,q,p]): per-workgroup partial
    sums folded in index order, no float atomics -- two runs give the same bits, and so do the two layouts.
    want_dmasks=False (frozen masks, stage 1): -> (None, dcls) with the same bits of dcls; dmasks is neither computed nor allocated."""
    name = "m2f_class_mix_backward"
    cls, x, strides, B, Q, C, h, w = _mix_inputs(name, class_logits, mask_logits, pixel_major, Q)
    _need_f32_cuda(name, dmix, prob)
    if tuple(dmix.shape) != (B, C, h, w) or tuple(prob.shape) != (B, Q, C):
        raise ValueError(f"{name}: dmix {tuple(dmix.shape)} / prob {tuple(prob.shape)} for B {B}, Q {Q}, C {C}, {h} x {w}")
    chunks = _lib.value("mss_m2f_mix_backward_chunks", h * w)
    partial = torch.empty((B, chunks, Q, C), device=x.device, dtype=torch.float64)
    dmasks = torch.empty_like(x) if want_dmasks else None
    dcls = torch.empty((B, Q, C + 1), device=x.device, dtype=torch.float32)
    call("mss_m2f_mix_backward_f32", ptr(dmix.contiguous()), ptr(prob.contiguous()), ptr(cls), ptr(x), strides[0], strides[1], strides[2],
         B, Q, C, h, w, ptr(partial), ptr(dmasks), ptr(dcls))
    return dmasks, dcls


# ---- Mask2Former stage 1: the per-class sem_seg map and the differentiable anomaly score ---------------------------
STAGE1_BUDGET_ENV = "MSS_M2F_STAGE1_U_BYTES"
STAGE1_BUDGET_DEFAULT = 1 << 30


def stage1_budget():
    """Most bytes of upsampled mask logits U alive at once in m2f_semantic_inference: MSS_M2F_STAGE1_U_BYTES, default 1 GiB.
    A memory cap, not a tuned number: the results do not depend on it."""
    return int(os.environ.get(STAGE1_BUDGET_ENV, STAGE1_BUDGET_DEFAULT))


def stage1_chunks(B, Hp, Wp, ldq, budget=None):
    """The batch of B images as [(first image, images)] chunks of whole images whose U [images, Hp, Wp, ldq] float32 stays within
    `budget` bytes; an image that alone exceeds the budget is a chunk of its own. Plain Python."""
    budget = stage1_budget() if budget is None else int(budget)
    if B < 1 or Hp < 1 or Wp < 1 or ldq < 1:
        raise ValueError(f"stage1_chunks: B {B}, {Hp} x {Wp} x {ldq}")
    per = max(1, min(B, budget // (4 * Hp * Wp * ldq)))
    return [(s, min(per, B - s)) for s in range(0, B, per)]


def _semantic_forward(cls, cls_ood, lg, Q, Hp, Wp, H, W, budget):
    """-> (sem_seg [B,Cl,H,W], ood_score [B,H,W] or None, prob_ood [B,Q,C] or None, mix_ood [B,C,Hp,Wp] or None), chunk by chunk"""
    B, _, _, ldq = lg.shape
    sem, score, probs, mixes = [], [], [], []
    for s, n in stage1_chunks(B, Hp, Wp, ldq, budget):
        U = upsample_bilinear_nhwc(lg[s:s + n], (Hp, Wp))
        mix, _ = m2f_class_mix(cls[s:s + n], U, pixel_major=True, Q=Q)
        sem.append(m2f_mix_upsample(mix, (Hp, Wp), (H, W), "logits"))          # identity scale: the crop of sem_seg_postprocess
        if cls_ood is not None:
            mix_o, prob_o = m2f_class_mix(cls_ood[s:s + n], U, pixel_major=True, Q=Q)
            score.append(m2f_mix_upsample(mix_o, (Hp, Wp), (H, W), "neg_max"))
            probs.append(prob_o)
            mixes.append(mix_o)
        del U
    one = len(sem) == 1
    join = lambda parts: parts[0] if one else torch.cat(parts, 0)
    if cls_ood is None:
        return join(sem), None, None, None
    return join(sem), 1 + join(score), join(probs), join(mixes)                # train_m2f.py:407: 1 - max_c


class _SemanticInferenceFn(torch.autograd.Function):
    """m2f_semantic_inference as one node, differentiable in class_logits_ood only. Saved: the low-resolution logits, prob_ood and
    mix_ood; U is recomputed per chunk in the backward."""

    @staticmethod
    def forward(ctx, cls_ood, cls, lg, Q, Hp, Wp, H, W, budget):
        sem, score, prob, mix = _semantic_forward(cls, cls_ood, lg, Q, Hp, Wp, H, W, budget)
        ctx.save_for_backward(cls_ood, lg, prob, mix)
        ctx.cfg = (Q, Hp, Wp, H, W, budget)
        ctx.mark_non_differentiable(sem)
        return sem, score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _gsem, g):
        cls_ood, lg, prob, mix = ctx.saved_tensors
        Q, Hp, Wp, H, W, budget = ctx.cfg
        B, _, _, ldq = lg.shape
        g = g.contiguous().float()                                              # d (1 + neg_max) / d neg_max = 1
        dcls = []
        for s, n in stage1_chunks(B, Hp, Wp, ldq, budget):
            U = upsample_bilinear_nhwc(lg[s:s + n], (Hp, Wp))
            dmix = m2f_mix_upsample_backward(mix[s:s + n], (Hp, Wp), (H, W), dscore=g[s:s + n])
            dcls.append(m2f_class_mix_backward(dmix, prob[s:s + n], cls_ood[s:s + n], U, pixel_major=True, Q=Q, want_dmasks=False)[1])
            del U, dmix
        return (dcls[0] if len(dcls) == 1 else torch.cat(dcls, 0)), None, None, None, None, None, None, None, None


def m2f_semantic_inference(class_logits, mask_logits_nhwc, image_size, size=None, class_logits_ood=None, Q=None, budget=None):
    """MaskFormer.semantic_inference on LOW-resolution pixel-major mask logits [B,hm,wm,ldq] in the reference's order
    (maskformer_model.py:264-277, 343-345; sem_seg_postprocess is the crop): bilinear upsample to the padded `image_size`
    (align_corners=False), sigmoid, einsum("qc,qhw->chw") with softmax(class_logits)[..., :-1], crop to `size` -> sem_seg
    [B, min(C,19), H, W] (the reference's per-instance channels beyond the classes are what every caller slices off). With
    class_logits_ood also the anomaly score of train_m2f.py:387-407 on the upsampled masks, ood_score [B,H,W] = 1 - max_c: ->
    (sem_seg, ood_score). Q: the queries among the ldq columns (default: those of class_logits). The batch is processed in
    chunks of whole images (stage1_chunks; `budget` bytes, default the MSS_M2F_STAGE1_U_BYTES switch); every chunking gives the
    same bits. Differentiable in class_logits_ood only: sem_seg never requires grad, mask logits that require grad raise (stage 1
    freezes the masks; stage 2 has criterion.class_mix_upsample)."""
    name = "m2f_semantic_inference"
    heads = [class_logits] + ([class_logits_ood] if class_logits_ood is not None else [])
    _need_f32_cuda(name, mask_logits_nhwc, *heads)
    if torch.is_grad_enabled() and mask_logits_nhwc.requires_grad:
        raise NotImplementedError(f"{name}: no gradient to the mask logits (stage 1 freezes them; stage 2: criterion.class_mix_upsample)")
    if mask_logits_nhwc.dim() != 4 or any(c.dim() != 3 or c.shape != class_logits.shape or c.shape[0] != mask_logits_nhwc.shape[0] for c in heads):
        raise ValueError(f"{name}: class logits {[tuple(c.shape) for c in heads]} / mask logits {tuple(mask_logits_nhwc.shape)}")
    ldq = mask_logits_nhwc.shape[-1]
    Q = class_logits.shape[1] if Q is None else int(Q)
    C = class_logits.shape[2] - 1
    if Q != class_logits.shape[1] or not 1 <= Q <= min(ldq, MIX_MAX_QUERIES) or ldq % 4 or not 1 <= C <= MIX_MAX_CLASSES:
        raise ValueError(f"{name}: Q {Q} of class logits {tuple(class_logits.shape)} and a pitch of {ldq} (a multiple of 4; "
                         f"Q <= {MIX_MAX_QUERIES}, 1 <= C <= {MIX_MAX_CLASSES})")
    (Hp, Wp), (H, W) = (int(v) for v in image_size), (int(v) for v in (image_size if size is None else size))
    if not (1 <= H <= Hp and 1 <= W <= Wp):
        raise ValueError(f"{name}: size {(H, W)} does not lie inside image_size {(Hp, Wp)}")
    budget = stage1_budget() if budget is None else int(budget)
    cls, lg = class_logits.detach().contiguous(), mask_logits_nhwc.detach().contiguous()
    if class_logits_ood is None:
        return _semantic_forward(cls, None, lg, Q, Hp, Wp, H, W, budget)[0]
    return _SemanticInferenceFn.apply(class_logits_ood.contiguous(), cls, lg, Q, Hp, Wp, H, W, budget)


# ---- Mask2Former pixel-decoder glue (csrc/norm.hip) --------------------------------------------------------------------
def groupnorm(x, gn, relu=False, out=None, out_sample_stride=None, out_ld=None, want_stat=False):
    """nn.GroupNorm `gn` on an Act (NHWC). `out`: optional float tensor to write into (e.g. the encoder's token buffer
    [N, sum(HW), C] at a level's offset) with pixel stride `out_ld` and sample stride `out_sample_stride` floats.
    want_stat: also return the [N*groups, 2] (mean, rstd) view the backward needs."""
    N, HW, C = x.N, x.H * x.W, x.C
    dev = x.buf.device
    ws = torch.empty(_lib.value("mss_groupnorm_workspace_floats", N, HW, C, gn.num_groups), device=dev, dtype=torch.float32)
    if out is None:
        y = Act.empty(N, x.H, x.W, C, dev)
        optr, old, oss = y.ptr, y.ld, HW * y.ld
    else:
        y, optr, old, oss = out, ptr(out), out_ld, out_sample_stride
    call("mss_groupnorm_nhwc_f32", x.ptr, x.ld, HW * x.ld, N, HW, C, gn.num_groups, ptr(gn.weight), ptr(gn.bias), float(gn.eps),
         int(relu), optr, old, oss, ptr(ws))
    if want_stat:
        off = _lib.value("mss_groupnorm_stat_offset", N, HW, C)
        return y, ws[off:off + 2 * N * gn.num_groups]
    return y


def groupnorm_backward(gy_ptr, gy_ld, gy_ss, x, gn, stat, relu=False):
    """Backward of groupnorm(x, gn, relu): gy given as (pointer, pixel stride, sample stride) so that it may live inside a
    token buffer. Returns (dx Act, dgamma, dbeta)."""
    N, HW, C = x.N, x.H * x.W, x.C
    dev = x.buf.device
    dx = Act.empty(N, x.H, x.W, C, dev)
    dg = torch.empty(C, device=dev, dtype=torch.float32)
    db = torch.empty(C, device=dev, dtype=torch.float32)
    ws = torch.empty(_lib.value("mss_groupnorm_bwd_workspace_floats", N, HW, C, gn.num_groups), device=dev, dtype=torch.float32)
    call("mss_groupnorm_nhwc_bwd_f32", gy_ptr, gy_ld, gy_ss, x.ptr, x.ld, HW * x.ld, N, HW, C, gn.num_groups, ptr(stat), ptr(gn.weight),
         ptr(gn.bias), int(relu), dx.ptr, dx.ld, ptr(dg), ptr(db), ptr(ws))
    return dx, dg, db


def upsample_bilinear_bwd(dy, dtop_ptr, dtop_ld, dtop_ss, IH, IW, accumulate):
    """Transpose of the bilinear part of upsample_bilinear_add: dtop (+)= B^T dy, dtop given as (pointer, strides)."""
    call("mss_upsample_bilinear_bwd_nhwc_f32", dy.ptr, dy.ld, dy.N, dy.H, dy.W, dtop_ptr, dtop_ld, dtop_ss, IH, IW, dy.C, int(accumulate))


def nchw_into_rows(g, dst_ptr, dst_ld, dst_ss, accumulate=False):
    """NCHW gradient tensor -> rows of an NHWC / token buffer given as (pointer, pixel stride, sample stride)."""
    n, c, h, w = g.shape
    g = g.contiguous().float()
    call("mss_nchw_to_nhwc_strided_f32", ptr(g), n, c, h * w, dst_ptr, dst_ld, dst_ss, int(accumulate))


class TokenLevel:
    """One level of a token buffer [N, S, C] seen as an NHWC map: rows [start, start + H*W) of every sample."""
    __slots__ = ("buf", "start", "N", "H", "W", "C", "ld", "sample_stride")

    def __init__(self, buf, start, H, W):
        assert buf.dim() == 3 and buf.is_contiguous() and buf.dtype == torch.float32
        self.buf, self.start, self.H, self.W = buf, start, H, W
        self.N, S, self.C = buf.shape
        self.ld, self.sample_stride = self.C, S * self.C

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.start * self.C)


def _strided(x):
    """(pointer, pixel stride, sample stride) of an Act or a TokenLevel."""
    return (x.ptr, x.ld, x.sample_stride if isinstance(x, TokenLevel) else x.H * x.W * x.ld)


def upsample_bilinear_add(top, lat):
    """lat + F.interpolate(top, size=lat.shape[-2:], mode="bilinear", align_corners=False) (msdeformattn.py:344).
    top: Act or TokenLevel, lat: Act."""
    assert top.C == lat.C and top.N == lat.N
    y = Act.empty(lat.N, lat.H, lat.W, lat.C, lat.buf.device)
    tp, tld, tss = _strided(top)
    call("mss_upsample_bilinear_add_nhwc_f32", tp, tld, tss, top.N, top.H, top.W, lat.ptr, lat.ld, y.ptr, y.ld, lat.H, lat.W, lat.C)
    return y


def upsample_bilinear_nhwc(x, size):
    """F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False) of an NHWC float32 tensor [N,IH,IW,C] (C % 4 == 0) ->
    [N,OH,OW,C]: the kernel of upsample_bilinear_add without a lateral (lat == NULL), equal to it over an all-zero lateral."""
    _need_f32_cuda("upsample_bilinear_nhwc", x)
    if x.dim() != 4 or x.shape[-1] % 4:
        raise ValueError(f"upsample_bilinear_nhwc: {tuple(x.shape)} is not [N,IH,IW,C] with C a multiple of 4")
    x = x.contiguous()
    N, IH, IW, C = x.shape
    OH, OW = int(size[0]), int(size[1])
    y = torch.empty((N, OH, OW, C), device=x.device, dtype=torch.float32)
    call("mss_upsample_bilinear_add_nhwc_f32", ptr(x), C, IH * IW * C, N, IH, IW, None, 0, ptr(y), C, OH, OW, C)
    return y


def nhwc_to_nchw(x):
    """Act or TokenLevel -> contiguous NCHW tensor (module boundary of the pixel decoder)."""
    y = torch.empty((x.N, x.C, x.H, x.W), device=x.buf.device, dtype=torch.float32)
    xp, xld, xss = _strided(x)
    call("mss_nhwc_to_nchw_f32", xp, xld, xss, x.N, x.H * x.W, x.C, ptr(y))
    return y


def nchw_to_act(t, Cp=None):
    """NCHW tensor -> Act with the channel count padded up to a multiple of 16 (the MFMA kernels' K granularity)."""
    n, c, h, w = t.shape
    Cp = Cp or _round_up(c, 16)
    t = t.contiguous().float()
    out = Act.empty(n, h, w, Cp, t.device)
    call("mss_nchw_to_nhwc_pad_f32", ptr(t), out.ptr, n, c, h, w, Cp)
    return out


class _AddLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + res) in one HIP pass each way (msdeformattn.py:116-131 norm1 / norm2 sites)."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        C = x.shape[-1]
        x2, r2 = x.contiguous(), (res.contiguous() if res is not None else None)
        rows = x2.numel() // C
        y = torch.empty_like(x2)
        stat = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        call("mss_add_layernorm_f32", ptr(x2), ptr(r2), rows, C, ptr(weight), ptr(bias), float(eps), ptr(y), ptr(stat))
        ctx.save_for_backward(x2, r2, weight, stat)
        ctx.has_res = res is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, res, weight, stat = ctx.saved_tensors
        C = x.shape[-1]
        rows = x.numel() // C
        gy = gy.contiguous()
        dz = torch.empty_like(x)
        dg = torch.empty_like(weight)
        db = torch.empty_like(weight)
        ws = torch.empty(_lib.value("mss_add_layernorm_bwd_workspace_floats", rows, C), device=x.device, dtype=torch.float32)
        call("mss_add_layernorm_bwd_f32", ptr(gy), ptr(x), ptr(res), ptr(stat), rows, C, ptr(weight), ptr(dz), ptr(dg), ptr(db), ptr(ws))
        return dz, (dz if ctx.has_res else None), dg, db, None


def add_layernorm(x, res, ln):
    """nn.LayerNorm `ln` applied to x + res (res may be None). Falls back to torch for shapes the kernel does not take."""
    C = x.shape[-1]
    if x.is_cuda and x.dtype == torch.float32 and C % 256 == 0 and C <= 1024 and ln.elementwise_affine and ln.bias is not None \
            and tuple(ln.normalized_shape) == (C,):
        return _AddLayerNormFn.apply(x, res, ln.weight, ln.bias, ln.eps)
    return ln(x if res is None else x + res)
