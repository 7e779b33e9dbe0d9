"""GPU: mss_seg_hist / SegMeter (csrc/metric.hip, multishiftseg_amd/metric.py) -- the confusion matrix of the closed-set segmentation
metrics with the argmax fused. Every comparison is exact integer equality of the table against the numpy restatement
(tests/ref_seg_metric.py, which tests/test_seg_metric_cpu.py holds to the reference's own outputs); the scores derive from equal
integers by the same float64 numpy operations and are compared bit for bit as well.

Shapes: the launch plan has one workgroup per SegMeter._CHUNK pixels of an image, four rounds of 256 lanes x 4 pixels inside it, a
16-byte path and an element path per image: the edges below are 1, the 4-pixel lane, the 64-lane wave, the 256-lane round and the
chunk, each +-1, with one and three images (three: image bases of every alignment where H*W is odd)."""
import numpy as np
import pytest
import torch

import ref_seg_metric as R
from conftest import golden
from poison import POISONS, poisoned

pytestmark = pytest.mark.gpu

CASES = ("all", "absent", "ignore", "lattice")


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table(n_cl, pred, label):
    """SegMeter's table after one update"""
    from multishiftseg_amd.metric import SegMeter
    m = SegMeter(n_cl)
    m.update(pred, label)
    return m


@pytest.mark.parametrize("tag", CASES)
def test_golden_all_three_operand_kinds(tag):
    from multishiftseg_amd import metric as M
    g = golden("seg_metrics")
    logits, label = cuda(g[tag + "_logits"]), cuda(g[tag + "_label"])
    pred = g[tag + "_pred"]
    for p in (logits, cuda(pred), cuda(pred.astype(np.int64)), cuda(pred.astype(np.int32))):
        for lab in (label, label.long()):
            m = table(19, p, lab)
            assert np.array_equal(m.hist(), g[tag + "_hist"])
            assert same(m.compute(), g[tag + "_metric"])
            mean_iu, acc, iu, class_acc = m.compute(per_class=True)
            assert same([mean_iu, acc], g[tag + "_metric_per_class"]) and same(iu, g[tag + "_iu_per_class"]) and same(class_acc, g[tag + "_class_acc"])
    hist, labeled, correct = M.hist_info(19, cuda(pred.astype(np.int64)), label.long())
    assert isinstance(hist, np.ndarray) and hist.dtype == np.int64 and np.array_equal(hist, g[tag + "_hist"])
    assert type(labeled) is int and type(correct) is int and (labeled, correct) == (int(g[tag + "_labeled"]), int(g[tag + "_correct"]))
    assert np.array_equal(M.hist_info(19, logits, label)[0], g[tag + "_hist"])
    assert same(M.compute_metric([{"hist": hist, "labeled": labeled, "correct": correct}]), g[tag + "_metric"])


def _edges():
    from multishiftseg_amd.metric import SegMeter
    C = SegMeter._CHUNK
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3]


@pytest.mark.parametrize("n_cl", [2, 19, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_launch_plan_edges_on_lattice_logits(B, n_cl):
    rng = np.random.default_rng(100 * n_cl + B)
    for HW in _edges():
        logits = R.lattice_logits(rng, B, n_cl, HW)
        label = rng.integers(0, n_cl + 1, (B, 1, HW)).astype(np.int64)          # n_cl itself: an unlabelled pixel
        want, _, _ = R.hist_info(n_cl, np.argmax(logits, axis=1), label)
        got = table(n_cl, cuda(logits.reshape(B, n_cl, 1, HW)), cuda(label))
        assert np.array_equal(got.hist(), want), (HW, B, n_cl)
        assert int(got._host()[-1]) == 0
        got8 = table(n_cl, cuda(logits.reshape(B, n_cl, 1, HW)), cuda(np.where(label == n_cl, 255, label).astype(np.uint8)))
        assert np.array_equal(got8.hist(), want), (HW, B, n_cl, "uint8 labels")


@pytest.mark.parametrize("n_cl", [2, 19, 32])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 9), (65, 63), (64, 66)])
def test_channel_slices_aligned_and_unaligned(H, W, n_cl):
    """logits = x[:, 2:2+n_cl] of a [B, n_cl+5, H, W] tensor: img_stride != n_cl * HW, and with H*W odd the plane bases take every
    alignment (element path), with H*W % 4 == 0 they stay 16-byte aligned (vector path). The surrounding channels hold values
    above any logit: a wrong stride shows as a wrong argmax."""
    from multishiftseg_amd.metric import SegMeter
    rng = np.random.default_rng(H * 1000 + W * 10 + n_cl)
    B = 3
    x = np.full((B, n_cl + 5, H, W), 1e6, dtype=np.float32)
    x[:, 2:2 + n_cl] = R.lattice_logits(rng, B, n_cl, H * W).reshape(B, n_cl, H, W)
    label = rng.integers(0, n_cl, (B, H, W)).astype(np.int64)
    want, _, _ = R.hist_info(n_cl, np.argmax(x[:, 2:2 + n_cl], axis=1), label)
    xd, ld = cuda(x), cuda(label)
    view = xd[:, 2:2 + n_cl]
    assert not view.is_contiguous()
    m = SegMeter(n_cl)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    m.update(view, ld)
    # the slice went in as it is: only the table was allocated, nothing of the size of a contiguous copy
    assert torch.cuda.max_memory_allocated() - before < min(view.numel() * 4, 16384)
    assert np.array_equal(m.hist(), want)
    # a layout the kernel does not take (channels last) is copied, not misread
    cl = cuda(np.ascontiguousarray(x[:, 2:2 + n_cl].transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert np.array_equal(table(n_cl, cl, cuda(label)).hist(), want)


def test_argmax_semantics_of_numpy():
    nan, inf = np.float32("nan"), np.float32("inf")
    cols = np.array([
        [1, 5, 5, 2, 5],              # the first of several maxima
        [0.0, -0.0, -1, -1, -1],      # 0.0 then -0.0: a tie, the first
        [-0.0, 0.0, -1, -1, -1],      # -0.0 then 0.0: a tie, the first
        [-1, nan, 7, 2, 1],           # a NaN before a larger finite value
        [-1, 7, nan, 2, 1],           # ... and after it
        [1, nan, 3, nan, 9],          # two NaNs: the first
        [1, inf, 3, inf, 2],          # +inf ties
        [-inf, -inf, -inf, -inf, -inf],
        [-inf, -3, -inf, -3, -inf],
        [nan, nan, nan, nan, nan],
    ], dtype=np.float32)
    want_idx = np.argmax(cols, axis=1)
    assert want_idx.tolist() == [1, 0, 0, 1, 2, 1, 1, 0, 1, 0]
    assert want_idx.tolist() == torch.from_numpy(cols).argmax(1).tolist()
    P = cols.shape[0]
    for reps in (1, 7):                                               # 10 pixels (element tail) and 70 (vector path + tail)
        logits = np.tile(cols.T.reshape(1, 5, 1, P), (1, 1, 1, reps))
        label = np.tile(np.arange(P) % 5, reps).reshape(1, 1, P * reps).astype(np.int64)
        want, _, _ = R.hist_info(5, np.tile(want_idx, reps), label)
        assert np.array_equal(table(5, cuda(logits), cuda(label)).hist(), want)


def test_labels_outside_the_classes_are_not_counted():
    n_cl, HW = 19, 300
    rng = np.random.default_rng(8)
    logits = R.lattice_logits(rng, 2, n_cl, HW)
    pred = np.argmax(logits, axis=1)
    l8 = rng.integers(0, n_cl, (2, 1, HW)).astype(np.uint8)
    l8[:, :, ::3] = 255
    l8[:, :, 1::7] = 254
    l8[:, :, 2::11] = n_cl
    want, labeled, _ = R.hist_info(n_cl, pred, l8)
    assert labeled == int((l8 < n_cl).sum()) < 2 * HW
    assert np.array_equal(table(n_cl, cuda(logits.reshape(2, n_cl, 1, HW)), cuda(l8)).hist(), want)
    l64 = rng.integers(0, n_cl, (2, 1, HW)).astype(np.int64)
    for k, v in enumerate((-1, n_cl, 255, (1 << 32) + 3, -(1 << 32) + 3, np.iinfo(np.int64).min, np.iinfo(np.int64).max)):
        l64[:, :, k::9] = v
    want, labeled, _ = R.hist_info(n_cl, pred, l64)
    assert labeled == int(((l64 >= 0) & (l64 < n_cl)).sum()) == 2 * len(range(7, HW, 9)) + 2 * len(range(8, HW, 9))
    for p in (cuda(logits.reshape(2, n_cl, 1, HW)), cuda(pred.reshape(2, 1, HW).astype(np.uint8)), cuda(pred.reshape(2, 1, HW))):
        m = table(n_cl, p, cuda(l64))
        assert np.array_equal(m.hist(), want) and int(m._host()[-1]) == 0


def test_maps_equal_the_fused_route_and_invalid_predictions_fill_the_last_slot():
    from multishiftseg_amd.metric import SegMeter
    n_cl = 19
    rng = np.random.default_rng(9)
    for B, HW in ((1, 5), (3, 4099), (2, SegMeter._CHUNK + 1)):
        logits = R.lattice_logits(rng, B, n_cl, HW)
        label = rng.integers(0, n_cl + 2, (B, 1, HW)).astype(np.int64)
        fused = table(n_cl, cuda(logits.reshape(B, n_cl, 1, HW)), cuda(label)).hist()
        pred = np.argmax(logits, axis=1).reshape(B, 1, HW)
        assert np.array_equal(fused, R.hist_info(n_cl, pred, label)[0])
        for p in (pred.astype(np.uint8), pred.astype(np.int64), pred.astype(np.int16)):
            assert np.array_equal(table(n_cl, cuda(p), cuda(label)).hist(), fused)
    # predictions n_cl, 255 and -1 under valid labels
    B, HW = 2, 1031
    pred = rng.integers(0, n_cl, (B, 1, HW)).astype(np.int64)
    label = rng.integers(0, n_cl, (B, 1, HW)).astype(np.int64)
    label[:, :, ::5] = 255
    pred[:, :, 1::4] = n_cl
    pred[:, :, 2::13] = 255
    pred[:, :, 3::17] = -1
    pred[0, 0, 0] = 255                                               # ... and one under an ignored label: not counted anywhere
    want, invalid = R.split_invalid(n_cl, pred, label)
    assert invalid > 0
    m = table(n_cl, cuda(pred), cuda(label))
    assert np.array_equal(m.hist(), want) and int(m._host()[-1]) == invalid
    with pytest.raises(ValueError, match=f"{invalid} labelled pixels"):
        m.compute()
    p8 = np.where(pred < 0, 200, pred).astype(np.uint8)              # a byte map has no -1: 200 stands in
    m8 = table(n_cl, cuda(p8), cuda(label))
    assert np.array_equal(m8.hist(), want) and int(m8._host()[-1]) == invalid


def test_accumulation_reset_and_64_bit_carries():
    from multishiftseg_amd.metric import SegMeter
    n_cl = 19
    rng = np.random.default_rng(10)
    parts = [(R.lattice_logits(rng, b, n_cl, 24 * 40).reshape(b, n_cl, 24, 40), rng.integers(0, n_cl, (b, 24, 40)).astype(np.int64)) for b in (1, 2, 3)]
    m = SegMeter(n_cl)
    for lg, lab in parts:
        m.update(cuda(lg), cuda(lab))
    one = table(n_cl, cuda(np.concatenate([p[0] for p in parts])), cuda(np.concatenate([p[1] for p in parts])))
    assert np.array_equal(m.hist(), one.hist()) and int(m.hist().sum()) == 6 * 24 * 40
    m.reset()
    assert not m.hist().any() and m.compute() is None
    m.update(cuda(parts[0][0]), cuda(parts[0][1]))
    assert np.array_equal(m.hist(), R.hist_info(n_cl, np.argmax(parts[0][0], axis=1), parts[0][1])[0])
    # a cell just below 2^33: the adds are 64-bit (a 32-bit add would wrap at 2^32 and lose the carry into the upper word)
    m = SegMeter(n_cl)
    lab = np.full((1, 8, 8), 4, np.int64)
    lg = np.zeros((1, n_cl, 8, 8), np.float32)
    lg[:, 6] = 1
    m.update(cuda(lg), cuda(lab))
    m._table[4 * n_cl + 6] = (1 << 33) - 10
    m._table[5] = (1 << 32) - 1
    m.update(cuda(lg), cuda(lab))
    lab5 = np.zeros((1, 8, 8), np.int64)
    lg5 = np.zeros((1, n_cl, 8, 8), np.float32)
    lg5[:, 5] = 1
    m.update(cuda(lg5), cuda(lab5))
    h = m.hist()
    assert int(h[4, 6]) == (1 << 33) + 54 and int(h[0, 5]) == (1 << 32) + 63 and int(h.sum()) == (1 << 33) + 54 + (1 << 32) + 63


@pytest.mark.parametrize("value", POISONS)
def test_updates_on_dirty_memory(value):
    from multishiftseg_amd.metric import SegMeter
    g = golden("seg_metrics")
    logits, label, pred = cuda(g["ignore_logits"]), cuda(g["ignore_label"]), cuda(g["ignore_pred"])
    a, b = SegMeter(), SegMeter()
    with poisoned(value) as ctx:
        a.update(logits, label)
        b.update(pred, label.long())
    assert not ctx.unlisted
    assert np.array_equal(a.hist(), g["ignore_hist"]) and np.array_equal(b.hist(), g["ignore_hist"])


def _maskformer_shell():
    """The smallest full configuration (tests/test_gpu_maskformer_eval.py): the R50, a pixel decoder with one encoder layer, a
    predictor with two decoder layers, 8 queries and 19 classes."""
    import ref_resnet as RR
    import ref_transformer_decoder as RT
    from multishiftseg_amd import MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, build_resnet_backbone
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(3)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=128,
                                       transformer_enc_layers=1, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=19, hidden_dim=256, num_queries=8, nheads=8, dim_feedforward=128,
                                                       dec_layers=2, pre_norm=False, mask_dim=256, enforce_input_project=False)
    predictor.load_state_dict(RT.synth_state_dict(41, num_layers=2, num_queries=8, dim_feedforward=128), strict=True)
    m = MaskFormer(backbone, decoder, predictor).cuda().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_maskformer_evaluate_feeds_both_meters():
    from multishiftseg_amd.metric import OODMeter, SegMeter
    shell = _maskformer_shell()
    g = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(2):
        images = torch.rand((2, 3, 70, 100), generator=g).cuda()
        target = torch.randint(0, 21, (2, 70, 100), generator=g).cuda()      # 19, 20: unlabelled for the closed set
        batches.append((images, target))
    ood_batches = [(i, (t % 2)) for i, t in batches]
    seg = SegMeter()
    got_ood, got_seg = shell.evaluate(batches, seg_meter=seg)
    want = np.zeros((19, 19), np.int64)
    for images, target in batches:
        sem = shell.semantic_inference(images)
        assert sem.shape == (2, 19, 70, 100)
        want += R.hist_info(19, sem.argmax(1).cpu().numpy(), target.cpu().numpy())[0]
    assert np.array_equal(seg.hist(), want) and want.sum() > 0
    assert same(got_seg, R.metric(want)) and same(got_seg, seg.compute())
    # the OOD half is what evaluate returns without a seg_meter
    assert got_ood == shell.evaluate(batches) == shell.evaluate(batches, meter=OODMeter())
    both = shell.evaluate(ood_batches, meter=OODMeter(), seg_meter=SegMeter())
    assert both[0] is not None and both[0] == shell.evaluate(ood_batches)


def test_deeplab_evaluate_feeds_both_meters(deeplab_params):
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.metric import OODMeter, SegMeter
    m = DeepWV3Plus(19)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
    m = m.cuda().eval()
    rng = np.random.default_rng(12)
    batches = []
    for seed in (21, 22):
        img = torch.from_numpy(synth.synth_image(seed, 2, 96, 96)).cuda()
        batches.append((img, cuda(rng.integers(0, 21, (2, 96, 96)).astype(np.int64))))
    ood_batches = [(i, t % 2) for i, t in batches]
    for score_only in (False, True):
        m.score_only = score_only
        seg = SegMeter()
        got_ood, got_seg = m.evaluate(ood_batches, seg_meter=seg)
        assert not m.training and m.score_only == score_only
        m.score_only = False
        want = np.zeros((19, 19), np.int64)
        with torch.no_grad():
            for img, target in ood_batches:
                _, logit = m(img)
                want += R.hist_info(19, logit.argmax(1).cpu().numpy(), target.cpu().numpy())[0]
        m.score_only = score_only
        assert np.array_equal(seg.hist(), want) and want.sum() == 4 * 96 * 96
        assert same(got_seg, R.metric(want))
        assert got_ood is not None and got_ood == m.evaluate(ood_batches) == m.evaluate(ood_batches, meter=OODMeter())
    m.score_only = False
    seg = SegMeter()
    m.evaluate(batches, seg_meter=seg)                                # labels 2..20: 19 and 20 drop out of the closed set
    want = np.zeros((19, 19), np.int64)
    with torch.no_grad():
        for img, target in batches:
            want += R.hist_info(19, m(img)[1].argmax(1).cpu().numpy(), target.cpu().numpy())[0]
    assert np.array_equal(seg.hist(), want) and 0 < want.sum() < 4 * 96 * 96
    m.train()
    m.evaluate(ood_batches[:1])
    assert m.training                                                  # the mode is restored
