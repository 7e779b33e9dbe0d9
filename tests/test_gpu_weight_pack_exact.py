"""mss_conv2d_pack_weights_f32 and mss_conv2d_unpack_wgrad_f32 alone (csrc/conv_igemm.hip): both only move values -- or,
for the gather-sum, add the images in ascending order in fp32 -- so every mode is compared with a torch permute / index reference by
torch.equal. Destinations are NaN-filled with NaN behind their extent: every element that must be written is written, nothing behind
is touched; NaN also stands in every source element that must not be read. The shapes cross the kernels' edges: a ragged last
128-channel chunk (130), one whole chunk and a chunk boundary (256), rows too short for the line form (C = 3, the stem's), 1, 9 and 49
taps, K below and at Kpad."""
import pytest
import torch

from multishiftseg_amd._lib import call, ptr

pytestmark = pytest.mark.gpu

CANARY = 64
NAN = float("nan")


def _nan_buffer(n):
    return torch.full((n + CANARY,), NAN, device="cuda", dtype=torch.float32)


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)))


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("R,S", [(1, 1), (3, 3), (7, 7)])
def test_pack_is_the_permuted_weight_zero_padded(R, S, flip):
    T = R * S
    for K in (19, 128):
        for C, Cpad in ((3, 4), (48, 48), (130, 144), (256, 256)):
            g = _gen(R, flip, K, C)
            w = torch.randn((K, C, R, S), device="cuda", generator=g)
            if flip:       # rows run over the convolution's input channels, columns over its output channels, taps rotated by 180 degrees
                rows, cols = C, K
                Kpad, Cp = (64 if C <= 64 else 256), (32 if K == 19 else 128)
                body = w.flip(2, 3).permute(2, 3, 1, 0).reshape(T, C, K)
            else:
                rows, cols = K, C
                Kpad, Cp = (64 if K == 19 else 128), Cpad
                body = w.permute(2, 3, 0, 1).reshape(T, K, C)
            want = torch.zeros((T, Kpad, Cp), device="cuda")
            want[:, :rows, :cols] = body
            got = _nan_buffer(T * Kpad * Cp)
            call("mss_conv2d_pack_weights_f32", ptr(w), ptr(got), K, C, R, S, Kpad, Cp, flip, None, 0, 0)
            assert torch.equal(got[:T * Kpad * Cp].view(T, Kpad, Cp), want), (K, C)
            assert torch.isnan(got[T * Kpad * Cp:]).all(), (K, C)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("R,S", [(1, 1), (3, 3), (7, 7)])
def test_unpack_is_the_permuted_rows_assigned_or_added(R, S, accumulate):
    T = R * S
    for K, Kpad in ((19, 64), (128, 128)):
        for C, Cp in ((3, 4), (48, 48), (130, 144), (256, 256)):
            g = _gen(R, accumulate, K, C)
            packed = torch.full((T, Kpad, Cp), NAN, device="cuda")        # padding rows and columns: never read
            packed[:, :K, :C] = torch.randn((T, K, C), device="cuda", generator=g)
            val = packed[:, :K, :C].permute(1, 2, 0).reshape(K, C, R, S)
            got = _nan_buffer(K * C * T)
            want = val
            if accumulate:
                before = torch.randn((K, C, R, S), device="cuda", generator=g)
                got[:K * C * T] = before.reshape(-1)
                want = before + val
            call("mss_conv2d_unpack_wgrad_f32", ptr(packed), ptr(got), K, C, R, S, Kpad, Cp, accumulate, None, None, 0, 0)
            assert torch.equal(got[:K * C * T].view(K, C, R, S), want), (K, C)
            assert torch.isnan(got[K * C * T:]).all(), (K, C)


C0, C1 = 64, 64


def _keeps(n, g):
    """[n][C1] bool: which channels of the second source each image keeps, and the 16-column steps of each image."""
    keep = torch.rand((n, C1), device="cuda", generator=g) >= 0.5
    if n == 1:
        keep[0] = True                                        # one image that keeps every column
    elif n == 2:
        keep[:, 5] = False                                    # a channel no image keeps
        keep[:, 7] = True                                     # a channel all images keep
    else:
        keep[0] = True
        keep[1] = False                                       # an image that keeps none: k_steps = 0
        keep[2, 5] = False
    return keep


def _index(keep):
    """place [n][C1] (the channel compacted column p holds, -1: none), col [n][C1] (the column that holds channel c, -1: none),
    k_steps [n] (16-column steps that cover the kept channels), all int32 on the device."""
    n = keep.shape[0]
    place = torch.full((n, C1), -1, dtype=torch.int32)
    col = torch.full((n, C1), -1, dtype=torch.int32)
    steps = torch.zeros(n, dtype=torch.int32)
    for i, row in enumerate(keep.cpu()):
        kept = torch.nonzero(row).flatten().to(torch.int32)
        place[i, :len(kept)] = kept
        col[i, kept.long()] = torch.arange(len(kept), dtype=torch.int32)
        steps[i] = -(-len(kept) // 16)
    return place.cuda(), col.cuda(), steps.cuda()


@pytest.mark.parametrize("K,Kpad", [(19, 64), (128, 128)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_unpack_with_place_gathers_each_images_columns_and_zeroes_the_rest(n, K, Kpad):
    R = S = 3
    T, C = 9, C0 + C1
    g = _gen(n, K, 1)
    keep = _keeps(n, g)
    place, _col, steps = _index(keep)
    assert n == 1 or bool((16 * steps < C1).any())            # an extent shorter than C1 is among the images
    ld = C + 16
    packed = torch.full((T, Kpad, ld), NAN, device="cuda")
    packed[:, :K, :C] = torch.randn((T, K, C), device="cuda", generator=g)
    dense = packed[:, :K, :C].permute(1, 2, 0)                # [K][C][T]
    want = torch.zeros((n, K, C, T), device="cuda")
    want[:, :, :C0] = dense[:, :C0]
    p = torch.arange(C1, device="cuda")
    for i in range(n):
        valid = (place[i] >= 0) & (p < 16 * steps[i])
        src_c = C0 + place[i].clamp(min=0).long()
        want[i, :, C0:] = torch.where(valid[None, :, None], dense[:, src_c], torch.zeros((), device="cuda"))
    got = _nan_buffer(n * K * C * T)
    call("mss_conv2d_unpack_wgrad_f32", ptr(packed), ptr(got), K, C, R, S, Kpad, ld, 0, ptr(place), ptr(steps), n, C0)
    assert torch.equal(got[:n * K * C * T].view(n, K, C, T), want)
    assert torch.isnan(got[n * K * C * T:]).all()
    if n == 3:
        assert int(steps[1]) == 0 and float(got[:n * K * C * T].view(n, K, C, T)[1, :, C0:].abs().max()) == 0.0


@pytest.mark.parametrize("K,Kpad", [(19, 64), (128, 128)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_pack_with_col_adds_the_images_in_ascending_order(n, K, Kpad):
    R = S = 3
    T, C = 9, C0 + C1
    g = _gen(n, K, 2)
    keep = _keeps(n, g)
    _place, col, _steps = _index(keep)
    src = torch.randn((n, K, C, T), device="cuda", generator=g)
    for i in range(n):                                        # columns behind an image's kept channels: never read
        src[i, :, C0 + int(keep[i].sum()):] = NAN
    acc = torch.zeros((K, C, T), device="cuda")               # every sum starts from 0.f
    for i in range(n):
        term = torch.zeros((K, C, T), device="cuda")
        term[:, :C0] = src[i, :, :C0]
        held = col[i] >= 0
        term[:, C0:][:, held] = src[i][:, C0 + col[i][held].long()]
        acc = acc + term
    want = torch.zeros((T, Kpad, C), device="cuda")
    want[:, :K] = acc.permute(2, 0, 1)
    got = _nan_buffer(T * Kpad * C)
    call("mss_conv2d_pack_weights_f32", ptr(src), ptr(got), K, C, R, S, Kpad, C, 0, ptr(col), n, C0)
    out = got[:T * Kpad * C].view(T, Kpad, C)
    assert torch.equal(out, want)
    assert torch.isnan(got[T * Kpad * C:]).all()
    nobody = ~keep.any(dim=0)
    if n == 2:
        assert bool(nobody[5]) and float(out[:, :, C0:][:, :, nobody].abs().max()) == 0.0     # exact zeros where no image holds the channel
