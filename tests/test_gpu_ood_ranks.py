"""GPU: evaluation over ranks -- OODMeter.merge / keys / extend_keys / all_gather and evaluate(group=) of both models
(multishiftseg_amd/metric.py, ddp.shard_batches).

Everything is equality. compute() sorts the keys before it measures, so a union of key multisets gives the three floats of one
meter fed every map, bit for bit: the tuples are compared with ==, never within a tolerance. The one tolerance of the file is that
of tests/test_gpu_metric.py (1e-11, float64 rounding of the final sums and divisions) where the same numbers are held to the
float64 restatement oracle/metric.py. The restatement finds its thresholds with np.diff, which cannot see two equal infinities as
a tie (inf - inf is NaN); the three measures are functions of the order of the scores alone, so it is handed the scores with
+-inf replaced by +-2^100, a strictly increasing map on the values used here.

Maps: scores on the lattice k / 8 (30 values: ties everywhere, within and between the classes) with -0.0, +inf and -inf mixed in
under every label, labels 0 / 1 / 255. Sizes
5 x 4099, 4097, 17 and 4096 pixels: one pixel either side of the compaction chunk (OODMeter._CHUNK = 4096), and a map of six
chunks whose 8 lanes fill unevenly.

Processes: two ranks share GPU 0 over gloo (RCCL needs distinct devices), one mp.spawn per test, so with pytest's own process at
most three have the GPU open. The spawn helper is that of tests/test_gpu_m2f_ddp.py, which documents LIMIT: the parent joins its
workers under LIMIT seconds, then terminates them and fails; after a rank failed in any way or ran into the limit no further test
of this file starts a GPU process."""
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-11                        # tests/test_gpu_metric.py
LIMIT = 105.0                      # tests/test_gpu_m2f_ddp.py
SHAPES = ((5, 4099), (1, 4097), (1, 17), (1, 4096))
_STOPPED = []


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(worker, world, *args):
    """mp.spawn under LIMIT -> {rank: the worker's record}. A worker that raises fails the test with its traceback."""
    if _STOPPED:
        pytest.fail(f"no further GPU process is started: {_STOPPED[0]}")
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(worker, args=(world, _free_port(), out) + args, nprocs=world, join=False)
    deadline = time.monotonic() + LIMIT
    try:
        while not ctx.join(timeout=max(deadline - time.monotonic(), 0.01)):
            if time.monotonic() >= deadline:
                _STOPPED.append(f"the ranks of {worker.__name__} did not finish within {LIMIT:.0f} s")
                pytest.fail(_STOPPED[0])
    except Exception as e:                           # a rank raised (a HIP fault surfaces as a RuntimeError), exited or was killed
        _STOPPED.append(f"a rank of {worker.__name__} failed: {str(e)[-300:]}")
        raise
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
                p.join(10)
    return dict(out)


def _init(rank, world, port, backend="gloo", force=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.environ.pop("MSS_DDP_NO_COMM", None)
    os.environ["MSS_DDP_FORCE"] = "1" if force else "0"
    torch.cuda.set_device(0)
    if backend == "nccl":
        os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        os.environ.pop("MSS_DIST_BACKEND", None)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        os.environ["MSS_DIST_BACKEND"] = "gloo"
        dist.init_process_group("gloo", rank=rank, world_size=world)


# ---- the maps ------------------------------------------------------------------------------------------------------------------
def _host_map(k):
    """(score float32, label int64) of map k, from its seed alone: every rank can build every map."""
    rng = np.random.default_rng(40 + k)
    label = rng.choice(np.array([0, 1, 255], dtype=np.int64), size=SHAPES[k], p=[0.6, 0.25, 0.15])
    score = ((rng.integers(-12, 13, SHAPES[k]) + 5 * (label == 1)) / 8).astype(np.float32)     # id_out scores sit 5 steps higher
    u = rng.random(SHAPES[k])
    score[u < 0.06] = -0.0
    score[(u >= 0.06) & (u < 0.10)] = np.inf
    score[(u >= 0.10) & (u < 0.14)] = -np.inf
    return score, label


def _map(k, keep=None):
    """Map k on the device; keep = 0 / 1: the pixels of the other class become unlabelled."""
    score, label = _host_map(k)
    if keep is not None:
        label = np.where(label == 1 - keep, 255, label)
    return torch.from_numpy(score).to(DEV), torch.from_numpy(label).to(DEV)


def _meter(maps, many=False):
    from multishiftseg_amd.metric import OODMeter
    m = OODMeter()
    if many:
        m.update_many(maps)
    else:
        for s, l in maps:
            m.update(s, l)
    return m


def _float64(ks):
    from oracle import metric as ometric
    score = np.concatenate([_host_map(k)[0].reshape(-1) for k in ks]).astype(np.float64)
    label = np.concatenate([_host_map(k)[1].reshape(-1) for k in ks])
    assert np.isposinf(score).sum() > 1 and np.isneginf(score).sum() > 1 and (np.signbit(score) & (score == 0)).sum() > 1
    big = 2.0 ** 100
    score = np.where(np.isposinf(score), big, np.where(np.isneginf(score), -big, score))
    return ometric.eval_ood_measure(score, label)


def _same_keys(a, b):
    """The two meters hold the same key multisets (sorted on the device with stock torch)."""
    return all(x.dtype == torch.int32 and x.shape == y.shape and torch.equal(torch.sort(x)[0], torch.sort(y)[0]) for x, y in zip(a.keys(), b.keys()))


# ---- 1: in one process ---------------------------------------------------------------------------------------------------------
def test_merge_and_key_round_trip_are_exact_in_process():
    from multishiftseg_amd.metric import OODMeter
    if _STOPPED:
        pytest.fail(f"no further GPU work is started: {_STOPPED[0]}")
    maps = [_map(k) for k in range(4)]
    one = _meter(maps)
    want = one.compute()
    a, b = _meter(maps[:2]), _meter(maps[2:], many=True)
    a_alone, b_alone = a.compute(), b.compute()
    assert want is not None and a_alone is not None and b_alone is not None and len({want, a_alone, b_alone}) == 3
    assert a.merge(b) is a
    got = a.compute()
    print(f"merged {got}, one meter {want}")
    assert got == want
    assert b.compute() == b_alone                                         # the other meter is valid and unchanged
    assert _same_keys(a, one)
    # keys out, keys in: from a meter of lane segments, from a meter of dense chunks, and in two parts
    neg, pos = a.keys()
    labels = np.concatenate([_host_map(k)[1].reshape(-1) for k in range(4)])
    assert (neg.numel(), pos.numel()) == (int((labels == 0).sum()), int((labels == 1).sum()))
    assert neg.dtype == pos.dtype == torch.int32 and neg.is_cuda and pos.is_cuda and neg.is_contiguous() and pos.is_contiguous()
    dense = OODMeter().extend_keys(neg, pos)
    assert dense.compute() == want
    assert OODMeter().extend_keys(*dense.keys()).compute() == want
    parts = OODMeter().extend_keys(*b.keys())
    assert parts.compute() == b_alone
    for s, l in maps[:2]:                                                 # both kinds of chunk in one meter
        parts.update(s, l)
    assert parts.compute() == want
    # an empty meter: two empty tensors, and taking them in changes nothing
    e_neg, e_pos = OODMeter().keys()
    assert e_neg.numel() == e_pos.numel() == 0 and e_neg.dtype == e_pos.dtype == torch.int32
    assert OODMeter().extend_keys(e_neg, e_pos).compute() is None and OODMeter().merge(OODMeter()).compute() is None
    assert OODMeter().merge(b).compute() == b_alone
    # a class that is missing: keys() of a meter for which compute() is None
    only_in = _meter([_map(1, keep=0)])
    n0, p0 = only_in.keys()
    assert only_in.compute() is None and p0.numel() == 0 and n0.numel() == int((_host_map(1)[1] == 0).sum())
    with pytest.raises(ValueError):
        a.merge(OODMeter(train_id_in=2))
    # the float64 restatement, under the tolerance of tests/test_gpu_metric.py
    ref = _float64(range(4))
    print(f"float64 {ref}, max |diff| {max(abs(x - y) for x, y in zip(got, ref)):.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=TOL)
    np.testing.assert_allclose(b_alone, _float64((2, 3)), rtol=0, atol=TOL)


# ---- 2 and 4: two ranks, uneven ------------------------------------------------------------------------------------------------
def _uneven_worker(rank, world, port, out):
    _init(rank, world, port)
    maps = [_map(k) for k in range(4)]
    ref = _meter(maps)
    want = ref.compute()
    m = _meter(maps[:3] if rank == 0 else maps[3:])
    r = dict(want=want, alone=m.compute())
    r["returns_self"] = m.all_gather() is m
    r["got"] = m.compute()
    r["same_keys"] = _same_keys(m, ref)
    r["again"] = m.compute()                                               # compute() leaves the state as it is
    try:
        m.all_gather()
        r["second"] = "no error"
    except RuntimeError as e:                                              # raised before any collective, on every rank alike
        r["second"] = str(e)
    r["after_refusal"] = m.compute()
    m.reset()
    r["reset_gather"] = m.all_gather() is m and m.compute() is None        # every rank empty: the counts travel, no key does
    out[rank] = r
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_uneven_shards_compute_the_single_meter_tuple():
    res = _run(_uneven_worker, 2)
    assert sorted(res) == [0, 1]
    ref = _float64(range(4))
    for rank in (0, 1):
        r = res[rank]
        print(f"rank {rank}: alone {r['alone']}, gathered {r['got']}, one meter {r['want']}")
        assert r["want"] is not None and r["alone"] is not None and r["alone"] != r["want"]
        assert r["returns_self"] and r["got"] == r["want"] and r["again"] == r["want"] and r["same_keys"]
        assert "all_gather" in r["second"] and "reset()" in r["second"]                  # RuntimeError, the state untouched
        assert r["after_refusal"] == r["want"] and r["reset_gather"]
        np.testing.assert_allclose(r["got"], ref, rtol=0, atol=TOL)
    assert res[0]["got"] == res[1]["got"]


# ---- 3: degenerate shards ------------------------------------------------------------------------------------------------------
def _degenerate_worker(rank, world, port, out):
    from multishiftseg_amd.metric import OODMeter
    _init(rank, world, port)
    r = {}
    # a rank that never calls update
    maps = [_map(1), _map(2)]
    m = _meter(maps) if rank == 0 else OODMeter()
    r["silent"] = (m.all_gather().compute(), _meter(maps).compute())
    # each rank holds one class only
    mine = _map(1, keep=0) if rank == 0 else _map(3, keep=1)
    m = _meter([mine])
    r["one_class_alone"] = m.compute()
    r["one_class"] = (m.all_gather().compute(), _meter([_map(1, keep=0), _map(3, keep=1)]).compute())
    n, p = m.keys()
    r["one_class_counts"] = (n.numel(), p.numel())
    # no rank holds an id_out pixel
    m = _meter([_map(0 if rank == 0 else 3, keep=0)])
    r["no_out"] = m.all_gather().compute()
    r["no_out_counts"] = tuple(t.numel() for t in m.keys())
    out[rank] = r
    dist.barrier()
    dist.destroy_process_group()


def test_degenerate_shards_empty_rank_one_class_each_and_a_missing_class():
    res = _run(_degenerate_worker, 2)
    assert sorted(res) == [0, 1]
    labels = [_host_map(k)[1] for k in range(4)]
    for rank in (0, 1):
        r = res[rank]
        got, want = r["silent"]
        assert want is not None and got == want
        assert r["one_class_alone"] is None
        got, want = r["one_class"]
        assert want is not None and got == want
        assert r["one_class_counts"] == (int((labels[1] == 0).sum()), int((labels[3] == 1).sum()))
        assert r["no_out"] is None and r["no_out_counts"] == (int((labels[0] == 0).sum()) + int((labels[3] == 0).sum()), 0)
    np.testing.assert_allclose(res[0]["silent"][0], _float64((1, 2)), rtol=0, atol=TOL)


# ---- 5: the RCCL path ----------------------------------------------------------------------------------------------------------
def _rccl_worker(rank, world, port, out):
    _init(0, 1, port, backend="nccl", force=True)
    assert dist.get_backend() == "nccl"
    maps = [_map(k) for k in range(4)]
    m = _meter(maps)
    before = m.compute()
    os.environ["MSS_DDP_FORCE"] = "0"
    out["idle"] = m.all_gather() is m and not m._gathered and len(m._chunks) == 4     # one rank, not forced: nothing happens
    os.environ["MSS_DDP_FORCE"] = "1"
    m.all_gather()
    out["ran"] = m._gathered and not m._chunks and len(m._dense) == 1                  # the keys came back through the collective
    out["on_device"] = all(t.is_cuda for t in m._dense[0])
    out["before"], out["after"] = before, m.compute()
    out["same_keys"] = _same_keys(m, _meter(maps))
    try:
        m.all_gather()
        out["second"] = "no error"
    except RuntimeError:
        out["second"] = "RuntimeError"
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_backend_one_rank_all_gather():
    """A one-rank nccl group with MSS_DDP_FORCE=1, as test_rccl_backend_one_rank_m2f_steps: both collectives run device to
    device over RCCL, and the union over one rank is the meter's own multiset."""
    o = _run(_rccl_worker, 1)
    assert o.get("idle") is True and o.get("ran") is True and o.get("on_device") is True and o.get("same_keys") is True
    assert o.get("before") is not None and o.get("after") == o.get("before") and o.get("second") == "RuntimeError"


# ---- 6: evaluate(group=) -------------------------------------------------------------------------------------------------------
def _maskformer():
    """The smallest builder of tests/test_gpu_maskformer_train.py."""
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
    m.backbone.freeze(1, norms=True)
    return m


def _maskformer_worker(rank, world, port, out):
    from multishiftseg_amd import ddp
    from multishiftseg_amd.metric import OODMeter, SegMeter
    _init(rank, world, port)
    model = _maskformer()
    g = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(4):
        images = torch.rand((1, 3, 64, 96), generator=g).to(DEV)
        batches.append((images, torch.randint(0, 21, (1, 64, 96), generator=g).to(DEV)))     # 0 / 1: the OOD classes; 19, 20: unlabelled
    ref_seg = SegMeter()
    want = model.evaluate(batches, meter=OODMeter(), seg_meter=ref_seg)
    mine = list(ddp.shard_batches(iter(batches)))                          # rank and world from the default group
    seg = SegMeter()
    got = model.evaluate(iter(mine), meter=OODMeter(), seg_meter=seg, group=True)
    # an empty shard: rank 1 is given nothing and still returns the result of rank 0's four batches
    seg2 = SegMeter()
    got2 = model.evaluate(iter(batches if rank == 0 else []), meter=OODMeter(), seg_meter=seg2, group=dist.group.WORLD)
    out[rank] = dict(shard=len(mine), want_ood=want[0], got_ood=got[0], got2_ood=got2[0],
                     seg_scores=[tuple(float(v) for v in x[1]) for x in (want, got, got2)],
                     table=torch.equal(seg._table.cpu(), ref_seg._table.cpu()), table2=torch.equal(seg2._table.cpu(), ref_seg._table.cpu()),
                     labelled=int(ref_seg._table.sum()))
    dist.barrier()
    dist.destroy_process_group()


def test_maskformer_evaluate_over_two_ranks_returns_the_one_process_result():
    res = _run(_maskformer_worker, 2)
    assert sorted(res) == [0, 1]
    for rank in (0, 1):
        r = res[rank]
        print(f"rank {rank}: {r['got_ood']} against {r['want_ood']}")
        assert r["shard"] == 2 and r["labelled"] > 0
        assert r["want_ood"] is not None and r["got_ood"] == r["want_ood"] and r["got2_ood"] == r["want_ood"]
        assert r["table"] and r["table2"]
        assert r["seg_scores"][1] == r["seg_scores"][0] and r["seg_scores"][2] == r["seg_scores"][0]


def test_deeplab_evaluate_in_a_forced_one_rank_group(deeplab_params, monkeypatch):
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.metric import OODMeter, SegMeter
    if _STOPPED:
        pytest.fail(f"no further GPU work is started: {_STOPPED[0]}")
    m = DeepWV3Plus(19)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
    m = m.cuda().eval()
    rng = np.random.default_rng(12)
    batches = [(torch.from_numpy(synth.synth_image(seed, 1, 64, 64)).cuda(), torch.from_numpy(rng.integers(0, 2, (1, 64, 64))).cuda())
               for seed in (21, 22)]
    want_seg = SegMeter()
    want = m.evaluate(batches, seg_meter=want_seg)
    assert want[0] is not None and want[0] == m.evaluate(batches)
    assert not dist.is_initialized()
    monkeypatch.setenv("MSS_DDP_FORCE", "1")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        meter, seg = OODMeter(), SegMeter()
        got = m.evaluate(batches, meter=meter, seg_meter=seg, group=True)
        assert meter._gathered and not meter._chunks                       # the collectives ran: the keys came back as a dense chunk
        assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]) and torch.equal(seg._table, want_seg._table)
        assert m.evaluate(batches, group=True) == want[0]
        assert m.evaluate(batches, group=dist.group.WORLD) == want[0]
        plain = OODMeter()
        assert m.evaluate(batches, meter=plain) == want[0] and not plain._gathered and len(plain._chunks) == 2      # group=None: as before
    finally:
        dist.destroy_process_group()
