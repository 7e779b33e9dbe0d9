"""GPU: prepare_targets and the two wrappers of csrc/m2f_targets.hip against the numpy restatement of the reference's host-side
target build (tests/ref_m2f_targets.py). Everything is integer-exact: torch.equal, no tolerances. The shapes are the smallest at
which the kernels can go wrong: one pixel, a row narrower than a vector, rows whose width is odd (single-byte stores, unaligned
mask starts), 8- and 4-byte stores (Wp = 8 * odd, 4 * odd), more than one workgroup per image, padded and unpadded sizes."""
import functools

import numpy as np
import pytest
import torch

import poison
import ref_m2f_targets as ref
from multishiftseg_amd import HungarianMatcher, M2FTargets, SetCriterion, prepare_targets
from multishiftseg_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRY = [(5, 37), (32, 64), (33, 65), (1, 1), (7, 300)]
PALETTE = np.array(list(range(19)) + [99, 100, 101, 254, 255], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _batch(B, H, W, seed=0):
    """B label maps that differ in T_b: image b draws from the first 3 + 7 b entries of the palette (the last image from all of it:
    19 classes, 99, 100, 101, 254, 255), so small maps hold few classes and later images more."""
    rng = np.random.default_rng([seed, B, H, W])
    sem = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        n = len(PALETTE) if b == B - 1 else min(len(PALETTE), 3 + 7 * b)
        sem[b] = PALETTE[rng.integers(0, n, (H, W))]
    return sem


def _check(t, sem_np, div, thr=100, ignore=255):
    """An M2FTargets against the restatement on the same maps: every dict entry, and the pack."""
    want = ref.prepare_targets(sem_np, div, ignore, thr)
    B, H, W = sem_np.shape
    Hp, Wp = ref.padded_size(H, W, div)
    assert isinstance(t, M2FTargets) and len(t) == B
    tmask, tstart, labels, counts = t.packed
    assert counts == [len(w["labels"]) for w in want]
    total = sum(counts)
    assert tuple(tmask.shape) == (total, Hp, Wp) and tmask.dtype == torch.uint8
    assert tstart.dtype == torch.int32 and tstart.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert labels.dtype == torch.int32 and labels.tolist() == [int(v) for w in want for v in w["labels"]]
    assert tuple(t.ood.shape) == (B, Hp, Wp) and int(tmask.max() if total else 0) <= 1 and int(t.ood.max()) <= 1
    for b, (got, w) in enumerate(zip(t, want)):
        assert got["labels"].dtype == torch.int64 and got["masks"].dtype == torch.bool and got["ood_mask"].dtype == torch.bool
        assert torch.equal(got["labels"].cpu(), torch.from_numpy(w["labels"])), b
        assert got["masks"].shape == w["masks"].shape and torch.equal(got["masks"].cpu(), torch.from_numpy(w["masks"])), b
        assert torch.equal(got["ood_mask"].cpu(), torch.from_numpy(w["ood_mask"])), b
    return want


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("div", [1, 32])
@pytest.mark.parametrize("hw", GEOMETRY, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_geometry_and_batch(hw, div, B):
    sem = _batch(B, *hw)
    _check(prepare_targets(torch.from_numpy(sem).to(DEV), size_divisibility=div), sem, div)


@pytest.mark.parametrize("div,hw", [(8, (3, 17)), (4, (3, 9)), (2, (3, 5)), (0, (6, 48))], ids=["8-byte", "4-byte", "2-byte", "div0"])
def test_narrower_store_widths(div, hw):
    """Wp = 24, 12 and 6: rows are aligned to 8, 4 and 2 bytes only, so the fill takes its narrower vectors."""
    sem = _batch(3, *hw)
    _check(prepare_targets(torch.from_numpy(sem).to(DEV), size_divisibility=div), sem, div)


def _content(name, H=5, W=37):
    rng = np.random.default_rng(7)
    if name == "all_255":
        return np.full((1, H, W), 255, np.int64)
    if name == "one_class":
        return np.full((1, H, W), 7, np.int64)
    if name == "all_19":
        return (np.arange(H * W, dtype=np.int64) % 19).reshape(1, H, W)
    base = rng.integers(0, 5, (1, H, W)).astype(np.int64)
    if name == "threshold_minus_1":
        base[0, 2, 3:9] = 99
    elif name == "threshold_itself":
        base[0, 1, 4:30] = 100
    elif name == "with_254":
        base[0, 0:3, 10:20] = 254
    elif name == "without_254":
        base[0, 0:3, 10:20] = 255
    elif name == "last_pixel_only":
        base[0, H - 1, W - 1] = 17
    elif name == "batch_without_targets":
        base = np.stack([np.full((H, W), 255, np.int64), np.full((H, W), 100, np.int64), np.full((H, W), 254, np.int64)])
    else:
        raise KeyError(name)
    return base


@pytest.mark.parametrize("div", [1, 32])
@pytest.mark.parametrize("name", ["all_255", "one_class", "all_19", "threshold_minus_1", "threshold_itself", "with_254", "without_254",
                                  "last_pixel_only", "batch_without_targets"])
def test_content(name, div):
    sem = _content(name)
    t = prepare_targets(torch.from_numpy(sem).to(DEV), size_divisibility=div)
    want = _check(t, sem, div)
    counts = [len(w["labels"]) for w in want]
    expect = {"all_255": [0], "one_class": [1], "all_19": [19], "batch_without_targets": [0, 0, 0]}.get(name)
    if expect is not None:
        assert counts == expect
    if name == "batch_without_targets":
        assert t.packed[0].shape[0] == 0 and int(t.ood[2].sum()) == 5 * 37 and int(t.ood[:2].sum()) == 0
    if name == "threshold_minus_1":
        assert want[0]["labels"][-1] == 99
    if name == "threshold_itself":
        assert 100 not in want[0]["labels"].tolist() and not want[0]["ood_mask"].any()
    if name == "with_254":
        assert int(t.ood.sum()) == 30
    if name == "without_254":
        assert int(t.ood.sum()) == 0
    if name == "last_pixel_only":
        assert want[0]["labels"][-1] == 17 and int(t[0]["masks"][-1].sum()) == 1 and bool(t[0]["masks"][-1, 4, 36])


@pytest.mark.parametrize("div", [1, 32])
def test_dtypes_agree_and_negative_values_are_no_class(div):
    sem = _batch(3, 33, 65)
    dev64 = torch.from_numpy(sem).to(DEV)
    runs = [prepare_targets(dev64.to(dt), size_divisibility=div) for dt in (torch.int64, torch.int32, torch.uint8)]
    _check(runs[0], sem, div)
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r.packed[:3], runs[0].packed[:3])) and r.packed[3] == runs[0].packed[3]
        assert torch.equal(r.ood, runs[0].ood)
    # the documented deviation: -1 / -200 / the most negative value are neither a class nor OOD
    neg = sem.copy()
    neg[0, 0, :7] = -1
    neg[1, 5, 5] = -200
    neg[2, 32, 64] = np.iinfo(np.int32).min
    for dt in (torch.int64, torch.int32):
        _check(prepare_targets(torch.from_numpy(neg).to(DEV).to(dt), size_divisibility=div), neg, div)
    big = neg.copy()
    big[2, 32, 64] = np.iinfo(np.int64).min
    big[2, 0, 0] = 2 ** 32 + 3                                  # not class 3: all 64 bits count
    got = prepare_targets(torch.from_numpy(big).to(DEV), size_divisibility=div)
    want = _check(got, big, div)
    assert want[2]["ood_mask"][0, 0] and bool(got[2]["ood_mask"][0, 0])     # above the threshold and not 255: OOD, as in the reference


def test_non_contiguous_input_equals_its_contiguous_copy():
    wide = torch.from_numpy(_batch(3, 33, 80)).to(DEV)
    view = wide[:, 1:, 3:68]
    assert not view.is_contiguous()
    a, b = prepare_targets(view), prepare_targets(view.contiguous())
    _check(a, view.cpu().numpy(), 32)
    assert all(torch.equal(x, y) for x, y in zip(a.packed[:3], b.packed[:3])) and torch.equal(a.ood, b.ood)
    assert a[1]["sem_seg"].data_ptr() == view[1].data_ptr()


@pytest.mark.parametrize("thr", [1, 64, 65, 128])
def test_label_threshold_crosses_the_presence_word(thr):
    rng = np.random.default_rng(thr)
    values = np.array([0, 1, 62, 63, 64, 65, 66, 100, 126, 127, 128, 129, 200, 254, 255], dtype=np.int64)
    sem = values[rng.integers(0, len(values), (2, 9, 70))]
    sem[1][sem[1] == 63] = 64                                   # image 1 lacks 63, image 0 has both sides of the word boundary
    for dt in (torch.int64, torch.uint8):
        t = prepare_targets(torch.from_numpy(sem).to(DEV).to(dt), size_divisibility=1, label_threshold=thr)
        want = _check(t, sem, 1, thr=thr)
    assert want[0]["labels"].tolist() == [int(v) for v in values if v < thr]
    # the set itself: bit v of the image's two words
    _, _, rank, present = K.m2f_targets_count(torch.from_numpy(sem).to(DEV), thr)
    for b in range(2):
        lo, hi = (int(v) & (2 ** 64 - 1) for v in present[b].tolist())
        assert [v for v in range(128) if ((lo >> v) if v < 64 else (hi >> (v - 64))) & 1] == want[b]["labels"].tolist()
        assert rank[b].tolist() == [want[b]["labels"].tolist().index(v) if v in want[b]["labels"] else -1 for v in range(thr)]


@pytest.mark.parametrize("div,hw", [(1, (5, 37)), (32, (5, 37)), (1, (33, 65)), (8, (3, 17))], ids=["bytes", "padded", "odd", "8-byte"])
def test_fill_writes_every_byte(div, hw):
    sem_np = _batch(3, *hw)
    sem = torch.from_numpy(sem_np).to(DEV)
    want = ref.prepare_targets(sem_np, div)
    Hp, Wp = ref.padded_size(*hw, div)
    tstart, labels, rank, _ = K.m2f_targets_count(sem)
    total = int(tstart[-1])
    want_mask = torch.from_numpy(np.concatenate([w["masks"] for w in want]).astype(np.uint8))
    want_ood = torch.from_numpy(np.stack([w["ood_mask"] for w in want]).astype(np.uint8))
    assert total == want_mask.shape[0]
    for fill in (0xAB, 0x00):
        tmask = torch.full((total, Hp, Wp), fill, device=DEV, dtype=torch.uint8)
        ood = torch.full((3, Hp, Wp), fill, device=DEV, dtype=torch.uint8)
        got = K.m2f_targets_fill(sem, tstart, rank, total, (Hp, Wp), tmask=tmask, ood=ood)
        assert got[0] is tmask and got[1] is ood
        assert torch.equal(tmask.cpu(), want_mask) and torch.equal(ood.cpu(), want_ood), hex(fill)
    # buffers that start one byte off a 16-byte boundary: the fill falls back to single-byte stores
    flat_m = torch.full((total * Hp * Wp + 1,), 0xAB, device=DEV, dtype=torch.uint8)
    flat_o = torch.full((3 * Hp * Wp + 1,), 0xAB, device=DEV, dtype=torch.uint8)
    tmask, ood = flat_m[1:].view(total, Hp, Wp), flat_o[1:].view(3, Hp, Wp)
    K.m2f_targets_fill(sem, tstart, rank, total, (Hp, Wp), tmask=tmask, ood=ood)
    assert torch.equal(tmask.cpu(), want_mask) and torch.equal(ood.cpu(), want_ood)
    assert int(flat_m[0]) == 0xAB and int(flat_o[0]) == 0xAB


def test_wrappers_refuse_mismatched_shapes():
    sem = torch.from_numpy(_batch(3, 5, 37)).to(DEV)
    tstart, _, rank, _ = K.m2f_targets_count(sem)
    total = int(tstart[-1])
    with pytest.raises(ValueError):
        K.m2f_targets_fill(sem, tstart, rank, total, (4, 37))
    with pytest.raises(ValueError):
        K.m2f_targets_fill(sem, tstart[:-1], rank, total, (5, 37))
    with pytest.raises(ValueError):
        K.m2f_targets_fill(sem, tstart, rank, total, (5, 37), tmask=torch.zeros((total, 5, 38), device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        K.m2f_targets_count(sem[0])
    with pytest.raises(NotImplementedError):
        K.m2f_targets_count(sem, 129)
    with pytest.raises(RuntimeError):
        K.m2f_targets_count(sem.float())


def test_two_calls_give_equal_bytes_and_no_unlisted_integer_scratch():
    sem_np = _batch(3, 33, 65)
    sem = torch.from_numpy(sem_np).to(DEV)
    a, b = prepare_targets(sem), prepare_targets(sem)
    with poison.poisoned(float("nan")):                          # its exit asserts that no integer buffer came from torch.empty
        c = prepare_targets(sem)
    for other in (b, c):
        assert all(torch.equal(x, y) for x, y in zip(a.packed[:3], other.packed[:3])) and torch.equal(a.ood, other.ood)
        assert a.packed[0].data_ptr() != other.packed[0].data_ptr()
    _check(c, sem_np, 32)


def test_dict_entries_are_views_of_the_pack():
    sem_np = _batch(3, 33, 65)
    sem = torch.from_numpy(sem_np).to(DEV)
    t = prepare_targets(sem)
    tmask, tstart, labels, counts = t.packed
    Hp, Wp = tmask.shape[1:]
    starts = tstart.tolist()
    assert len(set(counts)) > 1                                 # images that differ in T_b
    for b, d in enumerate(t):
        assert set(d) == {"labels", "masks", "ood_mask", "sem_seg"}
        assert d["labels"].dtype == torch.int64 and bool((d["labels"][1:] > d["labels"][:-1]).all())
        assert d["masks"].dtype == torch.bool and d["masks"].data_ptr() == tmask.data_ptr() + starts[b] * Hp * Wp
        assert d["masks"].is_contiguous() and tuple(d["masks"].shape) == (counts[b], Hp, Wp)
        assert d["ood_mask"].data_ptr() == t.ood.data_ptr() + b * Hp * Wp and tuple(d["ood_mask"].shape) == (Hp, Wp)
        assert d["sem_seg"].data_ptr() == sem[b].data_ptr() and torch.equal(d["sem_seg"], sem[b])
    one = prepare_targets(sem[1])                               # [H,W]: a batch of one
    assert len(one) == 1 and torch.equal(one[0]["masks"], t[1]["masks"]) and torch.equal(one[0]["sem_seg"], sem[1])


def test_matcher_passes_the_pack_through():
    sem = torch.from_numpy(_batch(3, 33, 65)).to(DEV)
    t = prepare_targets(sem)
    m = HungarianMatcher()
    for dev in (DEV, torch.device("cuda", torch.cuda.current_device()), sem.device):
        got = m._pack_targets(t, dev)
        assert got is t.packed and all(g is p for g, p in zip(got, t.packed))
    plain = m._pack_targets(list(t), DEV)                       # the same dicts as a plain list: the present code path
    assert plain[0] is not t.packed[0]
    assert all(torch.equal(g, p) for g, p in zip(plain[:3], t.packed[:3])) and plain[3] == t.packed[3]
    assert all(g.dtype == p.dtype for g, p in zip(plain[:3], t.packed[:3]))


def test_criterion_end_to_end_is_bit_identical_to_host_built_targets():
    """B 2, Q 8, 19 classes, 8 x 12 logits, 32 x 48 labels (padded to 32 x 64), S 2 steps, all points injected: the loss table and
    the gradients of every mask and class logit with prepare_targets equal those with targets built on the host by the
    restatement and uploaded, bit for bit."""
    B, Q, C, S, P, Pm = 2, 8, 19, 2, 33, 17
    rng = np.random.default_rng(5)
    sem_np = np.empty((B, 32, 48), dtype=np.int64)
    sem_np[0] = np.array([0, 3, 7, 11, 18, 255, 254])[rng.integers(0, 7, (32, 48))]          # 5 classes
    sem_np[1] = np.array([1, 3, 5, 8, 13, 17, 18, 2, 255])[rng.integers(0, 9, (32, 48))]     # 8 classes = Q
    want = ref.prepare_targets(sem_np, 32)
    total = sum(len(w["labels"]) for w in want)
    assert [len(w["labels"]) for w in want] == [5, 8]
    logits = (rng.standard_normal((S, B, Q, C + 1)) * 2).astype(np.float32)
    masks = (rng.standard_normal((S, B, Q, 8, 12)) * 3).astype(np.float32)
    over, keep = 3.0, 0.75
    n_cand, n_keep = int(P * over), int(keep * P)
    cand = torch.from_numpy(rng.random((S, total, n_cand, 2), dtype=np.float32)).to(DEV)
    rnd = torch.from_numpy(rng.random((S * total, P - n_keep, 2), dtype=np.float32)).to(DEV)
    mpoints = torch.from_numpy(rng.random((S, B, Pm, 2), dtype=np.float32)).to(DEV)

    def run(targets):
        crit = SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=Pm), {}, 0.1, ["labels", "masks"], P, over, keep, None, None, True).to(DEV)
        lg = [torch.from_numpy(logits[s]).to(DEV).requires_grad_(True) for s in range(S)]
        pm = [torch.from_numpy(masks[s]).to(DEV).requires_grad_(True) for s in range(S)]
        steps = [{"pred_logits": a, "pred_masks": b} for a, b in zip(lg, pm)]
        losses = crit(dict(steps[0], aux_outputs=steps[1:]), targets, point_candidates=cand, random_points=rnd, matcher_points=mpoints)
        sum((1.0 + 0.37 * j) * v for j, v in enumerate(losses.values())).backward()
        assert int(crit.matcher.last_status.abs().sum()) == 0
        return list(losses), torch.stack([v.detach() for v in losses.values()]).cpu(), [t.grad.cpu() for t in lg + pm]
    host = [{"labels": torch.from_numpy(w["labels"]).to(DEV), "masks": torch.from_numpy(w["masks"]).to(DEV)} for w in want]
    keys_h, loss_h, grads_h = run(host)
    keys_d, loss_d, grads_d = run(prepare_targets(torch.from_numpy(sem_np).to(DEV), size_divisibility=32))
    assert keys_h == keys_d and len(keys_h) == 3 * S
    assert torch.isfinite(loss_h).all() and torch.equal(loss_h, loss_d)
    assert all(bool(g.abs().sum() > 0) for g in grads_h)
    assert all(torch.equal(a, b) for a, b in zip(grads_h, grads_d))
