"""GPU parity of the fused RelContrastiveLoss against the reference's own outputs (golden, with the
reference's recorded permutations injected) and against the CPU oracle at a larger size."""
import ast

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import loss as oloss

pytestmark = pytest.mark.gpu


def run(params, logits, score, target, perms, **kw):
    from multishiftseg_amd.loss import RelContrastiveLoss
    crit = RelContrastiveLoss(params, **kw)
    lt = torch.from_numpy(logits).cuda().requires_grad_(True)
    st = torch.from_numpy(score).cuda().requires_grad_(True)
    tt = torch.from_numpy(target.astype(np.int64)).cuda()
    loss = crit(lt, st, tt, perms=perms)
    if torch.isfinite(loss):
        loss.backward()
    return loss, lt.grad, st.grad, tt


@pytest.mark.parametrize("tag", ["deeplab_4x32x32", "m2f_4x32x32", "ratio1_4x16x16", "no_ood_4x16x16",
                                 "no_in_aug_4x16x16", "deeplab_8x48x40"])
def test_golden(tag):
    g = golden("rcl_" + tag)
    params = ast.literal_eval(str(g["params"]))
    B, C, H, W = (int(v) for v in g["shape"])
    logits = g["logits"] if g["logits"].size else \
        np.random.default_rng(int(g["seed"])).standard_normal((B, C, H, W), dtype=np.float32) * 3
    perms = [torch.from_numpy(g[f"perm{i}"].astype(np.int64)) for i in range(3)]
    loss, dl, ds, tt = run(params, logits, g["score"], g["target"], perms)
    if np.isnan(g["loss"]):
        assert torch.isnan(loss)      # mean of an empty tensor, reproduced not "fixed"
    else:
        np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-5)
        np.testing.assert_allclose(ds.cpu().numpy(), g["dscore"], rtol=1e-4, atol=1e-8)
        d = dl.cpu().numpy()
        if "dlogit" in g:
            np.testing.assert_allclose(d, g["dlogit"], rtol=1e-3, atol=1e-7)
        else:
            np.testing.assert_allclose(d[:, :, ::3, ::3], g["dlogit_sub"], rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(np.abs(d.astype(np.float64)).sum(), g["dlogit_abs_sum"], rtol=1e-4)
    np.testing.assert_array_equal(tt.cpu().numpy().astype(np.uint8), g["target_mut"])


def test_seeded_reference_pairing_matches_oracle():
    """pairing='reference' draws torch.randperm on the CPU generator exactly as loss.py:129-131."""
    from multishiftseg_amd import synth
    rng = np.random.default_rng(77)
    B, H, W = 4, 96, 80
    logits = rng.standard_normal((B, 19, H, W), dtype=np.float32) * 3
    score = rng.standard_normal((B, H, W), dtype=np.float32) * 4
    target = synth.synth_targets(77, B // 2, H, W)
    params = {"ce_weights": [50, 10], "conduct_pixel_selection": True, "selection_ratio": 0.8,
              "inoutaug_contras_margins_tri": [10, 5, 5]}
    torch.manual_seed(5)
    loss, dl, ds, tt = run(params, logits, score, target, None)
    # replay the same three CPU permutations for the oracle
    t = target.copy()
    n_orig = int((t[:B // 2] < 99).sum()); n_aug = int((t[B // 2:] < 99).sum()); n_ood = int(((t > 99) & (t != 255)).sum())
    torch.manual_seed(5)
    perms = [torch.randperm(k).numpy() for k in (n_orig, n_aug, n_ood)]
    r = oloss.rel_contrastive_loss(logits, score, t, params, perms)
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    np.testing.assert_allclose(ds.cpu().numpy(), r["dscore"], rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(dl.cpu().numpy(), r["dlogit"], rtol=1e-3, atol=1e-7)
    np.testing.assert_array_equal(tt.cpu().numpy(), t)


def test_device_pairing_statistics():
    """pairing='device' (Feistel bijections): same terms except the two randomly paired hinges,
    which must agree with the reference pairing in expectation; every non-random term is exact."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.loss import RelContrastiveLoss
    rng = np.random.default_rng(78)
    B, H, W = 4, 128, 128
    logits = torch.from_numpy(rng.standard_normal((B, 19, H, W), dtype=np.float32) * 3).cuda()
    score = torch.from_numpy(rng.standard_normal((B, H, W), dtype=np.float32) * 4).cuda()
    target = torch.from_numpy(synth.synth_targets(78, B // 2, H, W)).cuda()
    params = {"ce_weights": [50, 10], "conduct_pixel_selection": True, "selection_ratio": 0.8,
              "inoutaug_contras_margins_tri": [10, 5, 5]}
    a = RelContrastiveLoss(params, pairing="reference")
    b = RelContrastiveLoss(params, pairing="device")
    torch.manual_seed(1)
    a(logits, score, target.clone())
    sr = score.clone().requires_grad_(True)
    lb = b(logits, sr, target.clone())
    lb.backward()
    ta, tb = a.last_terms.cpu().numpy(), b.last_terms.cpu().numpy()
    np.testing.assert_allclose(tb[[1, 2, 5]], ta[[1, 2, 5]], rtol=1e-6)      # ce_orig, ce_aug, c_in: deterministic
    np.testing.assert_allclose(tb[[3, 4]], ta[[3, 4]], rtol=0.05)            # c_orig, c_aug: same expectation
    assert torch.isfinite(sr.grad).all() and abs(float(sr.grad.sum())) < 1e-3  # +coef/-coef pairs cancel


def test_odd_batch_is_refused():
    """[orig...; aug...] pairs: an odd batch has no pairing (and used to overrun the augmented-CE buffer)."""
    from multishiftseg_amd.loss import RelContrastiveLoss
    crit = RelContrastiveLoss({"ce_weights": [50, 10], "conduct_pixel_selection": True, "selection_ratio": 0.8,
                               "inoutaug_contras_margins_tri": [10, 5, 5]})
    lt = torch.zeros(3, 19, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="odd"):
        crit(lt, torch.zeros(3, 8, 8, device="cuda"), torch.zeros(3, 8, 8, dtype=torch.int64, device="cuda"))


def _mix32(x):
    """mix32 of csrc/loss.hip on a uint32 array (products wrap modulo 2^32)."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _feistel_perm(i, n, seed):
    """feistel_perm of csrc/loss.hip for a uint32 array `i` of indices below n: four balanced Feistel rounds on 2*hb bits, walked
    again from its own output while that is >= n."""
    bits = max(int(max(n - 1, 1)).bit_length(), 2)
    hb = (bits + 1) >> 1
    hm = np.uint32((1 << hb) - 1)
    keys = [np.uint32((seed + 0x9e3779b9 * (rd + 1)) & 0xFFFFFFFF) for rd in range(4)]
    x = np.asarray(i, dtype=np.uint32).copy()
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        l, r = x[todo] >> np.uint32(hb), x[todo] & hm
        for key in keys:
            l, r = r, l ^ (_mix32(r ^ key) & hm)
        x[todo] = (l << np.uint32(hb)) | r
        todo &= x >= n
    return x


@pytest.mark.parametrize("n_sets,cap", [((5000, 4000, 900), 1 << 20), ((70000, 90000, 150000), 60000), ((300, 0, 50), 1 << 20), ((1, 1, 1), 1),
                                        ((180000, 190000, 170000), 1 << 20)])
def test_pair_launch_equals_the_restated_pairing(n_sets, cap):
    """mss_rcl_pairs_device2_f32 (both hinge terms in one launch, no atomics: thread i is the only writer of the three
    score-gradient elements pair i touches) against the pairing restated in numpy: the kernel's keyed Feistel bijections in uint32
    arithmetic and v = score[p] + margin - score[po] in float32, in the kernel's order. The three permutations are bijections over
    disjoint sets, so every score-gradient element is 0, coef, -coef or -coef + -coef with coef = float32(grad_w / float32(n)), all
    exact in fp32: bit-identical gradients. Each hinge sum adds at most two terms per thread and a 256-thread fp32 block sum before
    it reaches the float64 counter: about 9 * 2^-24 = 5.4e-7 of relative error against the float64 sum of the fp32 terms."""
    from multishiftseg_amd._lib import call, ptr
    s0, m0, m1, wc = 0x1234567, 10.0, 5.0, 1.0
    seeds = (s0 + 1, s0 + 2, s0 + 7)
    for n_set, seed in zip(n_sets, seeds):        # on the CPU, before any launch: the restated Feistel is a bijection of [0, n_set)
        if n_set:
            assert np.array_equal(np.sort(_feistel_perm(np.arange(n_set, dtype=np.uint32), n_set, seed)), np.arange(n_set, dtype=np.uint32))
    g = torch.Generator(device="cuda").manual_seed(sum(n_sets))
    npx = 600000
    score = torch.randn(npx, device="cuda", generator=g) * 4
    perm = torch.randperm(npx, device="cuda", generator=g).int()
    n0, n1, n2 = n_sets
    idx = [perm[:n0].contiguous(), perm[n0:n0 + n1].contiguous(), perm[n0 + n1:n0 + n1 + n2].contiguous()]
    idx = [t if t.numel() else torch.zeros(1, dtype=torch.int32, device="cuda") for t in idx]
    n_out = torch.tensor([n0, n1, n2, 0], dtype=torch.int32, device="cuda")
    n = min(cap, n0, n1, n2)
    sc, (i0, i1, io) = score.cpu().numpy(), (t.cpu().numpy() for t in idx)
    want_d, want_sum = np.zeros(npx, dtype=np.float32), [0.0, 0.0]
    if n:
        i = np.arange(n, dtype=np.uint32)
        p0, p1, po = i0[_feistel_perm(i, n0, seeds[0])], i1[_feistel_perm(i, n1, seeds[1])], io[_feistel_perm(i, n2, seeds[2])]
        v0, v1 = sc[p0] + np.float32(m0) - sc[po], sc[p1] + np.float32(m1) - sc[po]
        assert v0.dtype == v1.dtype == np.float32
        coef = np.float32(wc) / np.float32(n)
        want_d[p0[v0 > 0]] = coef
        want_d[p1[v1 > 0]] = coef
        t = np.where(v0 > 0, -coef, np.float32(0))
        want_d[po] = np.where(v1 > 0, t + -coef, t)
        want_sum = [float(v0[v0 > 0].astype(np.float64).sum()), float(v1[v1 > 0].astype(np.float64).sum())]
    c = torch.zeros(16, dtype=torch.float64, device="cuda")
    d = torch.zeros(npx, device="cuda")
    call("mss_rcl_pairs_device2_f32", ptr(score), ptr(idx[0]), ptr(idx[1]), ptr(idx[2]), ptr(n_out), cap, s0 + 1, s0 + 2, s0 + 7, m0, m1,
         ptr(c), wc, ptr(d))
    assert torch.equal(d.cpu(), torch.from_numpy(want_d))
    c = c.cpu().numpy()
    print(f"hinge sums {c[9:11].tolist()} against {want_sum}: relative {[abs(a - b) / b if b else 0.0 for a, b in zip(c[9:11].tolist(), want_sum)]}")
    np.testing.assert_allclose(c[9:11], want_sum, rtol=2e-6, atol=0)     # CNT_SUM_CORIG, CNT_SUM_CAUG
    assert c[11] == n and not c[:9].any() and not c[12:].any()            # CNT_N_PAIRS; nothing else is touched
    assert (d != 0).sum().item() <= 4 * n and (n == 0 or np.abs(c).sum() > 0)


SELECT_CASES = ["random", "ties", "inf_nan", "k0", "all", "tiny", "one_exponent"]


def _select_case(case):
    """(values, n, ratio, counters) of one selection case: many exact ties at the threshold, +inf / NaN entries (ignored pixels are +inf
    in ce_aug), k = 0, k = n, a single element, and values that share sign and exponent (the first pass sees one digit)."""
    g = torch.Generator(device="cuda").manual_seed(hash(case) % 1000)
    n, ratio = 300007, 0.8
    if case == "random":
        v = torch.randn(n, device="cuda", generator=g).abs() * 3
    elif case == "ties":
        v = (torch.randint(0, 7, (n,), device="cuda", generator=g).float() * 0.25)
    elif case == "inf_nan":
        v = torch.randn(n, device="cuda", generator=g).abs()
        v[::5] = float("inf")
        v[7::1001] = float("nan")
    elif case == "k0":
        v, ratio = torch.rand(n, device="cuda", generator=g), 1e-9
    elif case == "all":
        v, ratio = torch.rand(n, device="cuda", generator=g), 1.0
    elif case == "tiny":
        n = 1
        v = torch.tensor([0.37], device="cuda")
    else:
        v = 1.0 + torch.rand(n, device="cuda", generator=g) * 0.999
    n_in = int(torch.isfinite(v).sum()) if case == "inf_nan" else n
    counters = torch.zeros(16, dtype=torch.float64, device="cuda")
    counters[2] = n_in                                    # CNT_N_IN_AUG
    return v, n, ratio, n_in, counters


def _selection_words(v, ratio, n_in):
    """sel[0..5] from a sort: k = int(float32(ratio) * float32(n_in)), the key (f2key of csrc/loss.hip: order-preserving uint32 image of
    the fp32 bits) of the k-th smallest element by key order, the number of keys below it, k, how many elements equal to the threshold
    are taken, no tie ticket handed out yet, and the rank left inside the last bucket; all zero for k = 0."""
    k = int(np.float32(ratio) * np.float32(n_in))
    if k == 0:
        return [0] * 6
    b = v.cpu().numpy().view(np.uint32)
    keys = np.sort(np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)))
    kth = keys[k - 1]
    less = int(np.searchsorted(keys, kth, side="left"))
    return [int(kth), less, k, k - less, 0, k - less]


def _words(sel):
    return [w & 0xFFFFFFFF for w in sel[:6].tolist()]


@pytest.mark.parametrize("case", SELECT_CASES)
def test_selection_words_equal_the_sorted_keys(case):
    """mss_rcl_select_f32 (each digit's pick in front of the next byte's histogram pass: 5 launches, what the one-call loss runs), on
    dirty and on pre-zeroed scratch, against a sort of the keys (_select_case, _selection_words)."""
    from multishiftseg_amd._lib import call, ptr
    v, n, ratio, n_in, counters = _select_case(case)
    want = _selection_words(v, ratio, n_in)
    for zeroed in (0, 1):
        scratch = torch.full((4 * 256 + 16,), 0 if zeroed else 12345, dtype=torch.int32, device="cuda")
        sel = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        call("mss_rcl_select_f32", ptr(v), n, ptr(counters), ratio, ptr(scratch), zeroed, ptr(sel))
        assert _words(sel) == want, (case, zeroed, sel.tolist(), want)


@pytest.mark.parametrize("case", SELECT_CASES)
def test_stepwise_selection_words_equal_the_sorted_keys(case):
    """The entry points the data-parallel route steps through (init, then histogram and pick of bytes 3, 2, 1, 0), in one process
    without an all-reduce in between: the same words from the same inputs, and a histogram left zeroed for the next pass."""
    from multishiftseg_amd._lib import call, ptr
    v, n, ratio, n_in, counters = _select_case(case)
    want = _selection_words(v, ratio, n_in)
    hist = torch.full((256,), 12345, dtype=torch.int32, device="cuda")
    sel = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    call("mss_rcl_select_init_f32", ptr(counters), ratio, ptr(hist), ptr(sel))
    for shift in (24, 16, 8, 0):
        call("mss_rcl_select_hist_f32", ptr(v), n, ptr(sel), shift, ptr(hist))
        call("mss_rcl_select_pick_f32", ptr(sel), ptr(hist), shift)
        assert not hist.any()
    assert _words(sel) == want, (case, sel.tolist(), want)
