"""GPU: the per-sample channel compaction in front of the Dropout2d-folded 1x1 products (csrc/chan_compact.hip, the per-image mode
of gemm_nt_kernel, kernels.conv2d_dropped) -- kernel by kernel against numpy, the product against float64 with the bounds of
test_gpu_ops.py::test_bf16x3_gemm_fused_prologue_and_epilogue, and the whole model with the switch on and off against the reference
fixture. Every call runs on NaN-poisoned scratch and padding (tests/poison.py): the index / count buffers are float allocations
viewed as int32, so even the unwritten tail of `idx` carries a poison no kernel may read."""
import numpy as np
import pytest
import torch

from conftest import golden
from poison import poisoned

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as g
    g.build()
    from multishiftseg_amd import kernels
    return kernels


def _mask(rng, n, c, kept):
    """[n][c] fp32 masks with exactly kept[i] non-zero entries (arbitrary positive values) at random places."""
    m = np.zeros((n, c), np.float32)
    for i, k in enumerate(kept):
        m[i, rng.choice(c, size=k, replace=False)] = rng.uniform(0.5, 3.0, size=k).astype(np.float32)
    return m


def _fma32(x, s, h):
    """round_f32(x * s + h) with ONE rounding, as v_fma_f32 / v_pk_fma_f32 compute the prologue: the float64 product of two fp32
    values is exact; the float64 sum is made round-to-odd (TwoSum error term), which rounds to fp32 like the exact sum."""
    p = x.astype(np.float64) * s.astype(np.float64)
    hh = h.astype(np.float64)
    t = p + hh
    bb = t - p
    err = (p - (t - bb)) + (hh - bb)
    bits = t.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(t)
    toward = np.where(err > 0, np.inf, -np.inf)
    t = np.where(fix, np.nextafter(t, toward), t)
    return t.astype(np.float32)


def _place_ref(m_row):
    """numpy form of the placement (include/mss_hip.h): the kept channels sorted by the position the GEMM kernel's fma chain visits
    them at in the dense product (per 8-deep chunk k = 0, 4, 1, 5, 2, 6, 3, 7); the r-th of them goes to the column visited r-th."""
    kept = np.flatnonzero(m_row != 0)
    order = kept[np.argsort(8 * (kept >> 3) + 2 * (kept & 3) + ((kept >> 2) & 1), kind="stable")]
    place = np.full(m_row.shape[0], -1, np.int32)
    r = np.arange(len(order))
    place[8 * (r >> 3) + ((r & 7) >> 1) + 4 * (r & 1)] = order
    return place


def _index(K, mask):
    with poisoned(NAN):
        idx, count, ks, place = K.chan_compact_index(mask)
    torch.cuda.synchronize()
    return idx, count, ks, place


@pytest.mark.parametrize("n", [1, 2, 16])
@pytest.mark.parametrize("c", [128, 1024, 2048])
def test_index_builder_vs_numpy(K, n, c):
    rng = np.random.default_rng(n * 7 + c)
    cases = [0, 1, 15, 16, 17, c - 1, c]
    # every case on every sample position, neighbours differing; then all samples alike, then random counts
    lists = [[cases[(i + o) % len(cases)] for i in range(n)] for o in range(len(cases))]
    lists += [[17] * n, [int(rng.integers(0, c + 1)) for _ in range(n)]]
    for kept in lists:
        m = _mask(rng, n, c, kept)
        idx, count, ks, place = (t.cpu().numpy() for t in _index(K, torch.from_numpy(m).cuda()))
        for i in range(n):
            ref = np.flatnonzero(m[i] != 0)
            assert count[i] == len(ref) == kept[i]
            assert np.array_equal(idx[i, :len(ref)], ref)                       # ascending kept channels
            assert ks[i] == max(3, -(-len(ref) // 16))
            # the tail of the row was never written: it still holds the NaN poison's bit pattern
            assert (idx[i, len(ref):] == np.float32(NAN).view(np.int32)).all()
            # placement: written whole, a permutation of idx inside the first 8 * ceil(K_n / 8) <= 16 * k_steps columns, -1 elsewhere
            assert np.array_equal(place[i], _place_ref(m[i]))
            assert np.array_equal(np.sort(place[i][place[i] >= 0]), ref) and (place[i, 16 * ks[i]:] == -1).all()


@pytest.mark.parametrize("n,rows,c,ld", [(2, 37, 128, 128), (3, 24, 1024, 1024), (2, 19, 2048, 2048), (2, 16, 256, 320)])
def test_activation_compaction_is_bit_equal_to_the_dense_prologue(K, n, rows, c, ld):
    from multishiftseg_amd._lib import call, ptr
    rng = np.random.default_rng(c + rows)
    kept = ([0, 17, c] + [c // 2])[:n] if c != 128 else [c - 1, 1]
    m = _mask(rng, n, c, kept)
    x = rng.standard_normal((n * rows, ld)).astype(np.float32)
    sc = ((rng.random((n, c)) + 0.5) * m).astype(np.float32)
    sh = (rng.standard_normal((n, c)) * 0.3 * m).astype(np.float32)
    mt, xt, sct, sht = (torch.from_numpy(a).cuda() for a in (m, x, sc, sh))
    _idx, _count, ks, place = _index(K, mt)
    out = torch.full((n * rows, ld), NAN, device="cuda")
    call("mss_chan_compact_act_f32", ptr(xt), ld, ptr(out), ld, n, rows, c, ptr(place), ptr(ks), ptr(sct), ptr(sht))
    got = out.cpu().numpy()
    for i in range(n):
        sel = np.flatnonzero(m[i] != 0)
        blk, xb = got[i * rows:(i + 1) * rows], x[i * rows:(i + 1) * rows, :c]
        dense = np.maximum(_fma32(xb, sc[i][None, :], sh[i][None, :]), np.float32(0))      # what the dense prologue feeds the MFMA
        fill = 16 * max(3, -(-len(sel) // 16))
        pl = _place_ref(m[i])[:fill]
        assert np.array_equal(blk[:, :fill][:, pl >= 0].view(np.int32), dense[:, pl[pl >= 0]].view(np.int32))
        assert (blk[:, :fill][:, pl < 0].view(np.int32) == 0).all()                       # fill columns: exact (+0) zeros
        assert np.isnan(blk[:, fill:]).all()                                              # untouched: the poison survives


@pytest.mark.parametrize("n,kpad,c", [(2, 256, 128), (3, 128, 1024), (2, 256, 2048)])
def test_weight_compaction_is_bit_equal_to_a_column_gather(K, n, kpad, c):
    from multishiftseg_amd._lib import call, ptr
    rng = np.random.default_rng(kpad + c)
    kept = [0, c - 1, 33][:n]
    m = _mask(rng, n, c, kept)
    w = rng.standard_normal((kpad, c)).astype(np.float32)
    _idx, _count, ks, place = _index(K, torch.from_numpy(m).cuda())
    wt = torch.from_numpy(w).cuda()
    out = torch.full((n, kpad, c), NAN, device="cuda")
    call("mss_chan_compact_weights_f32", ptr(wt), ptr(out), n, kpad, c, ptr(place), ptr(ks))
    got = out.cpu().numpy()
    for i in range(n):
        sel = np.flatnonzero(m[i] != 0)
        fill = 16 * max(3, -(-len(sel) // 16))
        pl = _place_ref(m[i])[:fill]
        assert np.array_equal(got[i][:, :fill][:, pl >= 0].view(np.int32), w[:, pl[pl >= 0]].view(np.int32))
        assert (got[i][:, :fill][:, pl < 0].view(np.int32) == 0).all()
        assert np.isnan(got[i][:, fill:]).all()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hw,c,k", [(128 * 5, 128, 256), (32768, 1024, 2048), (32768, 2048, 4096)])
def test_compact_product_vs_float64(K, monkeypatch, n, hw, c, k):
    """conv2d_dropped (compaction passes + gemm_nt_kernel<false, 3, BN, true>) with residual, output ReLU and statistics against a float64
    product of the same fp32 operands, next to the dense per-sample prologue (MSS_DROPOUT_COMPACT=0) on the same inputs. One sample
    keeps no channel at all (y = res). Bounds: test_bf16x3_gemm_fused_prologue_and_epilogue's; and bit-equal to the dense form."""
    torch.manual_seed(hw + c + n)
    rng = np.random.default_rng(c + n)
    keep = {128: [0, 100, 128], 1024: [0, 717, 1024], 2048: [0, 1024, 1031]}[c][:n]
    mask = torch.from_numpy(_mask(rng, n, c, keep)).cuda()
    x = K.Act(torch.randn(n, 1, hw, c, device="cuda"))
    wt = torch.nn.Parameter(torch.randn(k, c, 1, 1, device="cuda") / c ** 0.5)
    pw = K.pack_weight(wt)
    sc = ((torch.rand(n, c, device="cuda") + 0.5) * mask).contiguous()
    sh = ((torch.randn(n, c, device="cuda") * 0.3) * mask).contiguous()
    res = K.Act(torch.randn(n, 1, hw, k, device="cuda"))
    ref = torch.empty(n * hw, k, device="cuda", dtype=torch.float64)
    for i in range(n):                         # float64 product of the fp32 operands the prologue forms
        xa = torch.relu(x.buf[i, 0].double() * sc[i].double() + sh[i].double())
        ref[i * hw:(i + 1) * hw] = torch.relu(xa @ wt.detach()[:, :, 0, 0].double().T + res.buf[i, 0].double())
    scale = ref.abs().max().item()

    assert K.dropout_compact_wanted(x, pw, (sc, sh), res)
    with poisoned(NAN):
        yc = K.conv2d_dropped(x, pw, mask, (sc, sh), res=res, want_stats=True, out_relu=True)
    monkeypatch.setenv("MSS_DROPOUT_COMPACT", "0")
    assert not K.dropout_compact_wanted(x, pw, (sc, sh), res)
    with poisoned(NAN):
        yd = K.conv2d(x, pw, in_affine=(sc, sh), in_relu=True, res=res, want_stats=True, out_relu=True)
    got_c, got_d = yc.buf.view(n * hw, k), yd.buf.view(n * hw, k)
    assert torch.isfinite(got_c).all()
    e_c = (got_c.double() - ref).abs().max().item() / scale
    e_d = (got_d.double() - ref).abs().max().item() / scale
    print(f"compact product n={n} hw={hw} c={c} k={k}: e_compact {e_c:.3e}  e_dense {e_d:.3e}")
    assert e_c < 2e-6 and e_c < 2 * e_d + 1e-7, (e_c, e_d)
    assert torch.equal(got_c[:hw], torch.relu(res.buf.view(n * hw, k)[:hw]))          # the sample without a kept channel: y = relu(res), exactly
    # the placement makes every output element's chain of fused multiply-adds the dense one with the zero terms left out
    assert torch.equal(got_c, got_d) and torch.equal(yc.stats, yd.stats)
    yp = got_c.double().view(-1, 64, k)
    np.testing.assert_allclose(yc.stats[:, 0].double().cpu().numpy(), yp.sum(1).cpu().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(yc.stats[:, 1].double().cpu().numpy(), (yp * yp).sum(1).cpu().numpy(), rtol=1e-4, atol=1e-3)


def test_straddling_and_split_route_shapes_keep_the_dense_path(K):
    """700 x 700 crops (88 x 88 = 7744 rows per image, not a multiple of the 128-row tile) and the split-bf16 route do not qualify."""
    c, k = 1024, 2048
    pw = K.pack_weight(torch.nn.Parameter(torch.randn(k, c, 1, 1, device="cuda")))
    aff = (torch.rand(2, c, device="cuda"), torch.rand(2, c, device="cuda"))
    assert not K.dropout_compact_wanted(K.Act(torch.zeros(2, 88, 88, c, device="cuda")), pw, aff)
    assert K.dropout_compact_wanted(K.Act(torch.zeros(2, 16, 16, c, device="cuda")), pw, aff)
    assert not K.dropout_compact_wanted(K.Act(torch.zeros(2, 16, 16, c, device="cuda")), pw, (aff[0][0], aff[1][0]))
    K.set_gemm_route("bf16x3")
    try:
        assert not K.dropout_compact_wanted(K.Act(torch.zeros(2, 16, 16, c, device="cuda")), pw, aff)
    finally:
        K.set_gemm_route(None)


def test_whole_model_compact_vs_dense_vs_reference_2x1024x2048(K, deeplab_params, monkeypatch):
    """Train-mode step at 2 x 1024 x 2048 with the reference fixture's Dropout2d masks, once with MSS_DROPOUT_COMPACT=1 and once with
    0: both within 1e-3 of the reference's logits and scores, argmax flips within test_gpu_fullsize.py's bound, and the running
    statistics of every BatchNorm (bn3 of the two dropout blocks and all later ones included) equal between the two runs to 1e-6 of
    the tensor's largest magnitude.

    The compacted product adds each output element's kept terms in the dense product's order (the placement of
    mss_chan_compact_index), so the two runs are expected to agree bit for bit, far inside the bound."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import TrainStep
    from test_gpu_fullsize import C3_FLIPS_MAX, LOSS_PARAMS, _flip_report
    g = golden("deepwv3plus_train_step_2x1024x2048")
    pairs, h, w = (int(v) for v in g["shape"])
    ss, ls = int(g["score_stride"]), int(g["logit_stride"])
    pre = "stage2_"
    img = torch.from_numpy(synth.synth_image(int(g["image_seed"]), 2 * pairs, h, w)).cuda()
    perms = [torch.from_numpy(g[pre + f"perm{i}"].astype(np.int64)) for i in range(3)]
    stats = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("MSS_DROPOUT_COMPACT", switch)
        m = DeepWV3Plus(19)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
        m = m.cuda()
        m.uncertainty_func_init()
        step = TrainStep(m, RelContrastiveLoss(LOSS_PARAMS), stage=2)
        step.keep_outputs = True
        m.dropout_masks = {"mod6": torch.from_numpy(g[pre + "drop_mod6"]), "mod7": torch.from_numpy(g[pre + "drop_mod7"])}
        target = torch.from_numpy(g["target"].astype(np.int64)).cuda()
        with poisoned(NAN):
            step(img, target, perms=perms)
        score, logit = step.last_outputs
        e_s = float(np.abs(score.detach().cpu().numpy()[:, ::ss, ::ss] - g[pre + "score"]).max())
        e_l = float(np.abs(logit.detach().cpu().numpy()[:, :, ::ls, ::ls] - g[pre + "logit_sub"]).max())
        flips = _flip_report(logit.detach(), g, pre, 2 * pairs, h, w)
        print(f"MSS_DROPOUT_COMPACT={switch}: max|dscore| {e_s:.3e} max|dlogit| {e_l:.3e} flips {flips}")
        assert e_s < 1e-3 and e_l < 1e-3, (switch, e_s, e_l)
        assert flips["flips_where_ref_margin_gt_1e3"] == 0 and flips["flips_all_pixels"] <= C3_FLIPS_MAX["winograd"], (switch, flips)
        stats[switch] = {k: v.detach().double().cpu() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}
        del step, m
    worst = ("", 0.0)
    for k, a in stats["1"].items():
        b = stats["0"][k]
        rel = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
        worst = max(worst, (k, rel), key=lambda t: t[1])
    print(f"running statistics, compact vs dense: worst {worst}")
    assert worst[1] < 1e-6, worst
