"""CPU: the closed-set segmentation metrics (multishiftseg_amd/metric.py: hist_info's table through SegMeter, compute_metric,
compute_score, compute_score_per_class -- lib/utils/metric.py:10-64) against the reference's own outputs in
tests/golden/seg_metrics.npz, exactly; the host side of SegMeter (from_hist, merge, all_reduce over gloo); and the argument checks
of mss_seg_hist, which return before any HIP call and so run without a device."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ref_seg_metric as R
from conftest import golden

CASES = ("all", "absent", "ignore", "lattice")


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.fixture(scope="module")
def g():
    return golden("seg_metrics")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib
    return _lib


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference(g, tag):
    pred, label = g[tag + "_pred"].astype(np.int64), g[tag + "_label"].astype(np.int64)
    assert np.array_equal(pred, np.argmax(g[tag + "_logits"], axis=1))
    hist, labeled, correct = R.hist_info(19, pred, label)
    assert hist.dtype == np.int64 and np.array_equal(hist, g[tag + "_hist"])
    assert (labeled, correct) == (int(g[tag + "_labeled"]), int(g[tag + "_correct"])) == (int(hist.sum()), int(np.trace(hist)))
    assert same(R.metric(hist), g[tag + "_metric"])
    mean_iu, acc, iu, class_acc = R.metric(hist, per_class=True)
    assert same([mean_iu, acc], g[tag + "_metric_per_class"]) and same(iu, g[tag + "_iu_per_class"]) and same(class_acc, g[tag + "_class_acc"])
    assert same(R.score(hist, correct, labeled)[0], g[tag + "_iu"])


@pytest.mark.parametrize("tag", CASES)
def test_host_mirrors_reproduce_the_reference(g, tag):
    from multishiftseg_amd import metric as M
    hist = g[tag + "_hist"]
    labeled, correct = int(g[tag + "_labeled"]), int(g[tag + "_correct"])
    # two partial results, as the reference's sweep appends one per image
    half = hist // 2
    results = [{"hist": half, "labeled": int(half.sum()), "correct": int(np.trace(half))},
               {"hist": hist - half, "labeled": labeled - int(half.sum()), "correct": correct - int(np.trace(half))}]
    assert same(M.compute_metric(results), g[tag + "_metric"])
    mean_iu, acc, iu, class_acc = M.compute_metric(results, per_class=True)
    assert same([mean_iu, acc], g[tag + "_metric_per_class"]) and same(iu, g[tag + "_iu_per_class"]) and same(class_acc, g[tag + "_class_acc"])
    iu, mean_iu, _, acc = M.compute_score(hist.astype(np.float64), correct, labeled)
    assert same(iu, g[tag + "_iu"]) and same([mean_iu, acc], g[tag + "_metric"])
    iu, mean_iu, class_acc, acc = M.compute_score_per_class(hist.astype(np.float64), correct, labeled)
    assert same(iu, g[tag + "_iu_per_class"]) and same(class_acc, g[tag + "_class_acc"]) and same([mean_iu, acc], g[tag + "_metric_per_class"])


def test_the_two_scorers_differ_where_classes_are_absent(g):
    """compute_score leaves a class that occurs in neither map as NaN under the nanmean; compute_score_per_class clamps its union to
    1, so it counts as IoU 0: the fixture's `absent` case must show both."""
    iu, iu_pc = g["absent_iu"], g["absent_iu_per_class"]
    assert int(np.isnan(iu).sum()) == 9 and not np.isnan(iu_pc).any() and np.array_equal(iu_pc[np.isnan(iu)], np.zeros(9))
    assert g["absent_metric"][0] > g["absent_metric_per_class"][0] and g["absent_metric"][1] == g["absent_metric_per_class"][1]
    assert same(g["all_metric"], g["all_metric_per_class"])


@pytest.mark.parametrize("tag", CASES)
def test_segmeter_from_hist_computes_on_a_host_table(g, tag):
    from multishiftseg_amd.metric import SegMeter
    for hist in (g[tag + "_hist"], torch.from_numpy(g[tag + "_hist"]), g[tag + "_hist"].astype(np.float64)):
        m = SegMeter.from_hist(hist)
        assert m.n_cl == 19 and m.hist().dtype == np.int64 and np.array_equal(m.hist(), g[tag + "_hist"])
        assert same(m.compute(), g[tag + "_metric"])
        mean_iu, acc, iu, class_acc = m.compute(per_class=True)
        assert same([mean_iu, acc], g[tag + "_metric_per_class"]) and same(iu, g[tag + "_iu_per_class"]) and same(class_acc, g[tag + "_class_acc"])


def test_segmeter_empty_invalid_merge_and_limits(g):
    from multishiftseg_amd.metric import SegMeter
    assert SegMeter().compute() is None and SegMeter().compute(per_class=True) is None
    assert SegMeter.from_hist(np.zeros((5, 5), np.int64)).compute() is None
    assert np.array_equal(SegMeter(7).hist(), np.zeros((7, 7), np.int64))
    m = SegMeter.from_hist(g["all_hist"])
    m._table[-1] = 3                                               # three labelled pixels with a prediction outside 0..18
    with pytest.raises(ValueError, match="3 labelled pixels"):
        m.compute()
    assert np.array_equal(m.hist(), g["all_hist"])                 # the table of the rest stays readable
    a, b = SegMeter.from_hist(g["all_hist"]), SegMeter.from_hist(g["ignore_hist"])
    assert a.merge(b) is a and np.array_equal(a.hist(), g["all_hist"] + g["ignore_hist"]) and np.array_equal(b.hist(), g["ignore_hist"])
    assert np.array_equal(SegMeter().merge(b).hist(), g["ignore_hist"]) and np.array_equal(b.merge(SegMeter()).hist(), g["ignore_hist"])
    with pytest.raises(ValueError):
        SegMeter(5).merge(b)
    for bad in (1, 33):
        with pytest.raises(ValueError):
            SegMeter(bad)
    with pytest.raises(ValueError):
        SegMeter.from_hist(np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        SegMeter().update(torch.zeros(1, 19, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
    assert SegMeter._CHUNK == 4096 and a.all_reduce() is a          # no process group: nothing to do


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from multishiftseg_amd.metric import SegMeter
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(5 + rank)
    mine = rng.integers(0, 1 << 40, (19, 19))                      # sums beyond 2^32: the table travels as int64
    both = sum(np.random.default_rng(5 + r).integers(0, 1 << 40, (19, 19)) for r in range(world))
    m = SegMeter.from_hist(mine)
    ok = m.all_reduce() is m and np.array_equal(m.hist(), both)
    empty = SegMeter() if rank == 0 else SegMeter.from_hist(mine)   # a rank that saw no batch still takes part
    ok = ok and np.array_equal(empty.all_reduce().hist(), np.random.default_rng(6).integers(0, 1 << 40, (19, 19)))
    out[rank] = bool(ok)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_sums_two_tables_exactly_over_gloo():
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    assert dict(out) == {0: True, 1: True}


def test_seg_hist_validates_arguments_before_any_launch(lib):
    """Raw calls with a NULL stream and a pointer nothing dereferences: every case returns before its launch (include/mss_hip.h
    states the order of the checks). Base case: f32 logits 2 x 19 x 35, dense strides, int64 labels."""
    OK, BAD, UNSUPPORTED = 0, lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    fn = lib.load().mss_seg_hist
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)

    def run(pred=X, kind=0, img=19 * 35, chan=35, label=X, lbytes=8, B=2, HW=35, n_cl=19, hist=X):
        return fn(pred, kind, img, chan, label, lbytes, B, HW, n_cl, hist, None)
    cases = [
        (dict(pred=None), BAD), (dict(label=None), BAD), (dict(hist=None), BAD),
        (dict(kind=2), BAD), (dict(kind=-1), BAD), (dict(kind=4), BAD),
        (dict(lbytes=4), BAD), (dict(lbytes=0), BAD),
        (dict(B=-1), BAD), (dict(HW=-1), BAD),
        (dict(chan=34), BAD),                                       # planes overlap
        (dict(img=19 * 35 - 1), BAD),                               # images overlap
        (dict(chan=-35, img=19 * 35), BAD), (dict(img=-19 * 35), BAD),
        (dict(n_cl=1), UNSUPPORTED), (dict(n_cl=33), UNSUPPORTED),
        (dict(B=1 << 16, HW=1 << 16, chan=1 << 16, img=19 << 16), UNSUPPORTED),      # 2^32 pixels
        (dict(B=1, HW=1 << 32, chan=1 << 32, img=19 << 32), UNSUPPORTED),
        (dict(B=0), OK), (dict(HW=0), OK), (dict(B=0, n_cl=19, chan=0, img=0), OK),
        (dict(B=0, n_cl=40), UNSUPPORTED),                          # the class limit is checked before the empty batch
        (dict(B=0, pred=None), BAD),
        # maps ignore the strides
        (dict(kind=1, B=0, chan=-5, img=-7), OK), (dict(kind=8, HW=0, chan=0, img=0), OK), (dict(kind=1, lbytes=1, B=0), OK),
        (dict(kind=8, n_cl=33), UNSUPPORTED), (dict(kind=1, B=1 << 16, HW=1 << 16), UNSUPPORTED),
    ]
    got = [run(**kw) for kw, _ in cases]
    assert got == [want for _, want in cases], [(kw, g_, w) for (kw, w), g_ in zip(cases, got) if g_ != w]


def test_the_scatter_probe_made_room_for_the_entry_point(lib):
    assert "mss_seg_hist" in lib.SIGNATURES and "mss_peak_scatter_f32" not in lib.SIGNATURES
    assert len(lib.SIGNATURES) == 142
    handle = lib.load()
    assert hasattr(handle, "mss_seg_hist") and not hasattr(handle, "mss_peak_scatter_f32")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mss_hip.h")).read()
    assert "int mss_seg_hist(" in hdr and "int mss_peak_scatter_f32(" not in hdr
