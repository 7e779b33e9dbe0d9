"""GPU: Mask2Former's stage-2 and stage-1 steps over a process group (m2f_trainer.M2FTrainStep / M2FStage1Step with
ddp.GradAllReduce in hook mode). Two ranks on the one GPU over gloo (RCCL needs distinct devices), as tests/test_gpu_ddp.py, on the
smallest full configuration (the builders are those of tests/test_gpu_maskformer_train.py): the R50 with freeze(1, norms=True), one
encoder layer, two decoder layers, 8 queries, 19 classes, one 2 x 3 x 64 x 96 batch per rank seeded by the rank, synthetic targets
with 3 targets in all on rank 0 and 5 on rank 1, and the matcher's and the criterion's point tables passed in, so that nothing
depends on a rank's random stream.

Equality: every rank scales its gradient by 1/2 (exact) and a sum of two terms has no order, so the averaged gradient is
torch.equal to 0.5 * (g0 + g1) of the local gradients, which tensor hooks clone before the sink sees them. The ranks compare among
themselves (the local gradients and the parameters are exchanged over gloo) and hand small records to the parent.

Limits: the parent joins its workers under LIMIT seconds, then terminates them and fails; nothing is tried again. LIMIT = 3 x what
tests/test_gpu_ddp.py takes on the GPU machine (its four tests: 35 s) = 105 s. After a rank failed in any way or ran into the limit no
further test of this file starts a GPU process: it fails at once. Any failure of a rank counts: a HIP fault reaches Python as a
RuntimeError."""
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ref_resnet as RR
import ref_transformer_decoder as RT

pytestmark = pytest.mark.gpu

DEV = "cuda"
Q, LAYERS, C = 8, 2, 19
STEPS = LAYERS                     # prediction steps the criterion sees: the last one and dec_layers - 1 auxiliary ones
BASE_LR = 1e-4
LIMIT = 105.0
COUNTS = {"plain": ((2, 1), (2, 3)), "empty": ((2, 1), (0, 0))}      # targets per image, per rank: 3 + 5 -> 4.0; 3 + 0 -> 1.5
UNUSED = "sem_seg_head.predictor.query_embed.weight"                 # rank 1 keeps this tensor out of its graph
RCL = {"ce_weights": [0.5, 0.25], "conduct_pixel_selection": False, "inoutaug_contras_margins_tri": [0.7, 0.5, 0.2]}
# the reference's fusion_layer of every cross-attention layer: in the state dict, used by nothing, so no rank has a gradient for it
DEAD = sorted(f"sem_seg_head.predictor.transformer_cross_attention_layers.{i}.fusion_layer.{s}" for i in range(LAYERS) for s in ("bias", "weight"))
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


# ---- the builders of tests/test_gpu_maskformer_train.py -----------------------------------------------------------------------
def _model():
    from multishiftseg_amd import MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, build_resnet_backbone
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(3)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=128,
                                       transformer_enc_layers=1, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=C, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=128,
                                                       dec_layers=LAYERS, pre_norm=False, mask_dim=256, enforce_input_project=False)
    predictor.load_state_dict(RT.synth_state_dict(41, num_layers=LAYERS, num_queries=Q, dim_feedforward=128), strict=True)
    m = MaskFormer(backbone, decoder, predictor).cuda().eval()
    m.backbone.freeze(1, norms=True)
    return m


def _criterion():
    from multishiftseg_amd import HungarianMatcher, SetCriterion, m2f_weight_dict
    weight_dict = m2f_weight_dict(2.0, 5.0, 5.0, 1.0, LAYERS + 1, True)
    return SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=33), weight_dict, 0.1, ["labels", "masks"], 65, 3.0, 0.75, None, None,
                        True).to(DEV)


def _batch(rank, counts):
    """(images, targets) of a rank: counts[b] targets in image b, labels distinct within an image."""
    images = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(1 + rank))
    rng = np.random.default_rng(5 + rank)
    targets = [{"labels": torch.tensor([(3 + 4 * t + b) % C for t in range(n)], dtype=torch.int64, device=DEV),
                "masks": torch.from_numpy(rng.random((n, 16, 24)) < 0.5).to(DEV)} for b, n in enumerate(counts)]
    return images.to(DEV), targets


def _tables(crit, rank, total_t):
    """The random numbers of one criterion call, from the rank's own generator: the matcher's points [S,B,P,2], the candidates
    [S, sum T, K, 2] and the random points [S * sum T, P - k, 2] of the uncertainty selection."""
    g = torch.Generator().manual_seed(100 + rank)
    S, B = STEPS, 2
    _, n_cand, n_keep = crit.selection()
    assert n_keep > 0
    return dict(matcher_points=torch.rand((S, B, crit.matcher.num_points, 2), generator=g).to(DEV),
                point_candidates=torch.rand((S, total_t, n_cand, 2), generator=g).to(DEV),
                random_points=torch.rand((S * total_t, crit.num_points - n_keep, 2), generator=g).to(DEV))


# ---- inside a rank -------------------------------------------------------------------------------------------------------------
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


def _gathered(t):
    """The ranks' tensors of one shape, on the host, in rank order."""
    t = t.detach().cpu().contiguous()
    got = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(got, t)
    return got


def _record(named):
    """Tensor hooks run before AccumulateGrad: the local gradient, cloned before the sink sees it."""
    rec = {}
    for n, p in named:
        p.register_hook(lambda g, n=n: rec.__setitem__(n, g.detach().clone()))
    return rec


def _is_view(sink, name, p):
    i, off, _ = sink.where[name]
    return p.grad.data_ptr() == sink.flat[i].data_ptr() + 4 * off


def _same_everywhere(t):
    got = _gathered(t)
    return all(torch.equal(got[0], x) for x in got)


def _average_ok(named, rec):
    """Per name: is p.grad torch.equal to 0.5 * (g0 + g1) of the ranks' recorded local gradients (zeros where a rank had none),
    and None exactly where no rank had one? -> (the names where it is not, the names this rank had no local gradient for, the names
    no rank had one for)."""
    produced = [None] * dist.get_world_size()
    dist.all_gather_object(produced, sorted(rec))
    somewhere = set().union(*produced)
    bad, missing, nowhere = [], [n for n, _ in named if n not in rec], [n for n, _ in named if n not in somewhere]
    for n, p in named:
        if n not in somewhere:
            if p.grad is not None:
                bad.append(n)
            continue
        g0, g1 = _gathered(rec[n] if n in rec else torch.zeros_like(p))
        if p.grad is None or not torch.equal(p.grad.detach().cpu(), 0.5 * (g0 + g1)):
            bad.append(n)
    return sorted(bad), sorted(missing), sorted(nowhere)


def _float64_norm(grads):
    return float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads)))


def _torch_norm(grads):
    """Stock torch in float32 on the CPU, the yardstick of tests/test_gpu_m2f_optim.py: clip_grad_norm_(foreach=False)."""
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return float(torch.nn.utils.clip_grad_norm_(ps, 1e30, foreach=False))


def _stage2_worker(rank, world, port, out, case):
    from multishiftseg_amd import M2FTrainStep, build_m2f_optimizer, weighted_losses
    from multishiftseg_amd.m2f_trainer import target_count
    _init(rank, world, port)
    model = _model().set_trainable()
    if rank == 1:                                    # the replicas start apart: the broadcast at construction has to mend it
        with torch.no_grad():
            model.sem_seg_head.predictor.class_embed.bias.add_(1.0)
    crit = _criterion()
    opt = build_m2f_optimizer(model, base_lr=BASE_LR, weight_decay=0.05, clip_value=0.01)
    step = M2FTrainStep(model, crit, opt, bucket_bytes=16 << 20)
    sink = step.sync
    names = {id(p): n for n, p in model.named_parameters()}
    named = [(names[id(p)], p) for p in opt.params]
    rec = _record(named)
    r = dict(active=sink is not None and sink.active, buckets=len(sink.buckets), handled=len(named),
             order_ok=[n for b in sink.buckets for n in b] == [n for n, _ in reversed(named)])
    images, targets = _batch(rank, COUNTS[case][rank])
    own = target_count(targets)
    inject = _tables(crit, rank, own)
    before = {n: p.detach().clone() for n, p in named}
    r["start_differs"] = [n for n, p in named if not _same_everywhere(p)]

    unused = dict(named)[UNUSED]

    def head(x):
        if rank == 0 or case != "plain":
            return model(x)
        unused.requires_grad_(False)                 # out of this rank's graph; it still requires grad when the gradients are handed out
        try:
            return model(x)
        finally:
            unused.requires_grad_(True)
    step.head = head

    # the single-process call on the same inputs: the losses with the global normaliser, and with the rank's own count
    want_n = {"plain": 4.0, "empty": 1.5}[case]
    ref = {k: v.detach() for k, v in weighted_losses(crit(model(images), targets, num_masks=want_n, **inject), crit.weight_dict).items()}
    own_ref = {k: v.detach() for k, v in weighted_losses(crit(model(images), targets, **inject), crit.weight_dict).items()}

    losses, norm = step(images, targets=targets, **inject)
    torch.cuda.synchronize()
    r["num_masks"] = step.last_num_masks
    r["finite"] = all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(norm))
    r["losses_equal_ref"] = list(losses) == list(ref) and all(torch.equal(losses[k], ref[k]) for k in ref)
    r["mask_losses_differ_from_own"] = [k for k in ref if ("mask" in k or "dice" in k) and not torch.equal(losses[k], own_ref[k])]
    r["ce_equal_own"] = all(torch.equal(losses[k], own_ref[k]) for k in ref if "loss_ce" in k)
    r["loss_keys"] = list(losses)
    r["grads_none"] = sorted(n for n, p in named if p.grad is None)
    r["not_views"] = [n for n, p in named if p.grad is not None and not _is_view(sink, n, p)]
    r["average_bad"], r["missing"], r["nowhere"] = _average_ok(named, rec)
    r["unused_nonzero"] = bool(unused.grad.any())
    grads = [p.grad.detach().cpu() for _, p in named if p.grad is not None]
    r["norm"] = float(norm)
    r["norm_bits_equal"] = _same_everywhere(norm.reshape(1))
    r["norm64"], r["norm_torch"] = _float64_norm(grads), _torch_norm(grads)
    rec.clear()

    images2, targets2 = _batch(rank + 2, COUNTS[case][rank])
    losses2, norm2 = step(images2, targets=targets2, **_tables(crit, rank + 2, own))
    torch.cuda.synchronize()
    r["finite"] = r["finite"] and all(bool(torch.isfinite(v)) for v in losses2.values()) and bool(torch.isfinite(norm2))
    r["params_differ"] = [n for n, p in named if not _same_everywhere(p)]
    r["not_moved"] = sorted(n for n, p in named if torch.equal(p.detach(), before[n]))
    r["not_finite"] = [n for n, p in named if not bool(torch.isfinite(p).all())]
    rate = {id(g["params"][0]): g["lr"] for g in opt.param_groups}
    backbone = [(n, p) for n, p in model.backbone.named_parameters() if p.requires_grad]
    r["backbone"] = len(backbone)
    r["backbone_rate_ok"] = all(rate[id(p)] == pytest.approx(0.1 * BASE_LR) for _, p in backbone)
    r["head_rate_ok"] = all(g["lr"] == pytest.approx(BASE_LR) for g in opt.param_groups if id(g["params"][0]) not in {id(p) for _, p in backbone})
    r["frozen_with_grad"] = [n for n, p in model.named_parameters() if not p.requires_grad and p.grad is not None]
    out[rank] = r
    dist.barrier()
    dist.destroy_process_group()


_ONCE = {}


@pytest.fixture(scope="module")
def two_rank_step():
    """One two-rank run of two stage-2 steps: started once, whatever its outcome, and read by the tests below."""
    if "run" not in _ONCE:
        try:
            _ONCE["run"] = _run(_stage2_worker, 2, "plain")
        except BaseException as e:                   # pytest.fail's outcome included: the run is not started a second time
            _ONCE["run"] = e
    if isinstance(_ONCE["run"], BaseException):
        pytest.fail(f"the two-rank run failed: {_ONCE['run']}")
    return _ONCE["run"]


def test_two_rank_gradients_are_the_exact_average_in_bucket_views(two_rank_step):
    for rank in (0, 1):
        r = two_rank_step[rank]
        assert r["active"] and r["buckets"] >= 3 and r["order_ok"] and r["handled"] > 100
        assert r["start_differs"] == [], r["start_differs"]                 # the construction broadcast rank 0's values
        # the reference's fusion_layer is used by nothing: no rank has a gradient for it and it keeps .grad None, as in one process
        assert r["nowhere"] == DEAD and r["grads_none"] == DEAD and r["average_bad"] == [], (r["grads_none"][:4], r["average_bad"][:4])
        # every other gradient is a view of its bucket; the one tensor rank 1 kept out of its graph got the average as a copy
        assert r["missing"] == sorted(DEAD + ([] if rank == 0 else [UNUSED])) and r["not_views"] == ([] if rank == 0 else [UNUSED])
        assert r["unused_nonzero"]


def test_two_rank_criterion_ran_with_the_global_normaliser(two_rank_step):
    for rank in (0, 1):
        r = two_rank_step[rank]
        assert r["num_masks"] == 4.0
        assert r["finite"] and r["losses_equal_ref"]
        mask_keys = [k for k in r["loss_keys"] if "mask" in k or "dice" in k]
        assert len(mask_keys) == 2 * STEPS and r["mask_losses_differ_from_own"] == mask_keys    # 3 and 5 are not 4
        assert r["ce_equal_own"]                                            # loss_ce has its own normaliser


def test_two_ranks_stay_in_lock_step_and_the_backbone_moves_at_a_tenth_of_the_rate(two_rank_step):
    for rank in (0, 1):
        r = two_rank_step[rank]
        assert r["params_differ"] == [] and r["not_moved"] == DEAD and r["not_finite"] == [], (r["params_differ"][:4], r["not_moved"][:4])
        assert r["backbone"] == 52 and r["backbone_rate_ok"] and r["head_rate_ok"] and r["frozen_with_grad"] == []


def test_two_rank_norm_is_the_norm_of_the_averaged_gradient(two_rank_step):
    a, b = two_rank_step[0], two_rank_step[1]
    assert a["norm_bits_equal"] and b["norm_bits_equal"] and a["norm"] == b["norm"] and a["norm64"] == b["norm64"]
    want = a["norm64"]
    bound = max(8 * abs(a["norm_torch"] - want), float(np.spacing(np.float32(want))))      # tests/test_gpu_m2f_optim.py, norm_out
    print(f"norm {a['norm']:.9g}, float64 {want:.9g}, |hip - float64| {abs(a['norm'] - want):.3e}, bound {bound:.3e}")
    assert want > 0 and abs(a["norm"] - want) <= bound


def test_a_rank_without_any_target_steps_and_the_other_finishes():
    res = _run(_stage2_worker, 2, "empty")
    assert sorted(res) == [0, 1]
    for rank in (0, 1):
        r = res[rank]
        assert r["num_masks"] == 1.5 and r["finite"] and r["losses_equal_ref"]
        assert r["grads_none"] == DEAD and r["average_bad"] == [] and r["missing"] == DEAD and r["not_views"] == []
        assert r["params_differ"] == [] and r["not_moved"] == DEAD and r["not_finite"] == []


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------
def _stage1_inputs(rank):
    images = torch.rand((2, 3, 60, 90), generator=torch.Generator().manual_seed(1 + rank))
    rng = np.random.default_rng(3 + rank)
    t = np.repeat(np.repeat(rng.integers(0, C, (2, 11, 11)), 6, 1), 9, 2)[:, :60, :90].astype(np.int64)
    t[:, :3, :] = 255
    t[1, 20:41, 30:61] = 254                         # an OOD object in the augmented image
    return images.to(DEV), torch.from_numpy(t).to(DEV)


def _stage1_worker(rank, world, port, out):
    from multishiftseg_amd import M2FStage1Step
    from multishiftseg_amd.loss import RelContrastiveLoss
    _init(rank, world, port)
    model = _model()
    if rank == 1:
        with torch.no_grad():
            model.sem_seg_head.predictor.class_embed2.bias.add_(1.0)
    step = M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="reference"), lr=1e-4, weight_decay=1e-4)
    head = model.sem_seg_head.predictor.class_embed2
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    rec = _record(named)
    before = {n: p.detach().clone() for n, p in named}
    r = dict(names=[n for n, _ in named], active=step.sync is not None and step.sync.active, buckets=len(step.sync.buckets),
             start_differs=[n for n, p in named if not _same_everywhere(p)])
    images, target = _stage1_inputs(rank)
    torch.manual_seed(11 + rank)
    loss = step(images, target.clone())
    torch.cuda.synchronize()
    r["with_grad"] = sorted(n for n, p in model.named_parameters() if p.grad is not None)
    r["not_views"] = [n for n, p in named if not _is_view(step.sync, n, p)]
    r["average_bad"], r["missing"], r["nowhere"] = _average_ok(named, rec)
    r["nonzero"] = bool(head.weight.grad.any()) and bool(head.bias.grad.any())
    torch.manual_seed(21 + rank)
    loss2 = step(images, target.clone())
    torch.cuda.synchronize()
    r["finite"] = bool(torch.isfinite(loss)) and bool(torch.isfinite(loss2)) and loss.dim() == 0 and not loss.requires_grad
    r["params_differ"] = [n for n, p in named if not _same_everywhere(p)]
    r["not_moved"] = sorted(n for n, p in named if torch.equal(p.detach(), before[n]))
    r["with_grad_after"] = sorted(n for n, p in model.named_parameters() if p.grad is not None)
    r["losses_differ"] = not torch.equal(*_gathered(loss.reshape(1)))
    out[rank] = r
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_stage1_step_averages_class_embed2_alone():
    res = _run(_stage1_worker, 2)
    want = ["sem_seg_head.predictor.class_embed2.bias", "sem_seg_head.predictor.class_embed2.weight"]
    for rank in (0, 1):
        r = res[rank]
        assert sorted(r["names"]) == want and r["active"] and r["buckets"] == 1 and r["start_differs"] == []
        assert r["with_grad"] == want and r["with_grad_after"] == want
        assert r["not_views"] == [] and r["average_bad"] == [] and r["missing"] == [] and r["nonzero"]
        assert r["finite"] and r["params_differ"] == [] and r["not_moved"] == []
        assert r["losses_differ"]                                           # the returned loss is the rank's own


# ---- the RCCL path ---------------------------------------------------------------------------------------------------------------
def _rccl_worker(rank, world, port, out):
    from multishiftseg_amd import M2FStage1Step, M2FTrainStep, build_m2f_optimizer
    from multishiftseg_amd.loss import RelContrastiveLoss
    _init(0, 1, port, backend="nccl", force=True)
    assert dist.get_backend() == "nccl"
    model = _model()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crit = _criterion()
    images, targets = _batch(0, COUNTS["plain"][0])
    inject = _tables(crit, 0, 3)
    res = {}
    for forced in (True, False):
        os.environ["MSS_DDP_FORCE"] = "1" if forced else "0"
        model.load_state_dict(state)
        model.set_trainable()
        opt = build_m2f_optimizer(model, base_lr=BASE_LR, weight_decay=0.05, clip_value=0.01)
        step = M2FTrainStep(model, crit, opt, bucket_bytes=16 << 20)
        assert (step.sync is not None) == forced
        losses, norm = step(images, targets=targets, **inject)
        torch.cuda.synchronize()
        if forced:
            out["side_streams"] = step.sync.comm_stream is not None
            out["num_masks"] = step.last_num_masks
            out["views"] = all(_is_view(step.sync, n, p) for n, p in step.sync.params.items() if p.grad is not None)
            out["none"] = sorted(n for n, p in step.sync.params.items() if p.grad is None)
            step.sync.detach()
        res[forced] = (losses, norm, [None if p.grad is None else p.grad.detach().clone() for p in opt.params],
                       [p.detach().clone() for p in opt.params])
        model.set_trainable(False)
        for p in model.parameters():
            p.grad = None
    (la, na, ga, pa), (lb, nb, gb, pb) = res[True], res[False]
    out["same"] = list(la) == list(lb) and all(torch.equal(la[k], lb[k]) for k in la) and torch.equal(na, nb) \
        and all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(ga, gb)) \
        and all(torch.equal(x, y) for x, y in zip(pa, pb))
    out["n"] = len(ga)
    # stage 1 over the same one-rank RCCL group
    s1 = {}
    for forced in (True, False):
        os.environ["MSS_DDP_FORCE"] = "1" if forced else "0"
        model.load_state_dict(state)
        step = M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="reference"))
        assert (step.sync is not None) == forced
        imgs, target = _stage1_inputs(0)
        torch.manual_seed(11)
        loss = step(imgs, target.clone())
        torch.cuda.synchronize()
        head = model.sem_seg_head.predictor.class_embed2
        s1[forced] = (loss, head.weight.detach().clone(), head.bias.detach().clone())
        if forced:
            step.sync.detach()
        for p in model.parameters():
            p.grad = None
    out["stage1_same"] = all(torch.equal(x, y) for x, y in zip(s1[True], s1[False]))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_backend_one_rank_m2f_steps():
    """Both steps with their collectives running over RCCL (a one-rank nccl group, MSS_DDP_FORCE=1): the bucket launches from the
    hooks on the side stream, the normaliser's and the flags' collectives on the host group beside it, backward_done, the optimizers -- the mean over one rank
    is the gradient itself, so losses, norm, gradients and parameters are those of the un-synchronised step, bit for bit."""
    o = _run(_rccl_worker, 1)
    assert o.get("same") is True and o.get("n") > 100 and o.get("stage1_same") is True
    assert o.get("side_streams") is True and o.get("views") is True and o.get("num_masks") == 3.0 and o.get("none") == DEAD


# ---- without a process group nothing changes --------------------------------------------------------------------------------------
def _old_train_step(self, *head_args, targets, **criterion_kwargs):
    """M2FTrainStep.__call__ as it was before the step knew about process groups."""
    from multishiftseg_amd import weighted_losses
    self.optimizer.zero_grad(set_to_none=True)
    outputs = self.head(*head_args)
    losses = weighted_losses(self.criterion(outputs, targets, **criterion_kwargs), self.criterion.weight_dict)
    if not losses:
        raise ValueError("M2FTrainStep: no loss of the criterion has a weight in its weight_dict")
    sum(losses.values()).backward()
    norm = self.optimizer.step()
    return {k: v.detach() for k, v in losses.items()}, norm


def _old_stage1_step(self, images, target):
    """M2FStage1Step.__call__ as it was."""
    self.optimizer.zero_grad(set_to_none=True)
    sem_seg, ood_score = self.model.stage1_forward(images)
    loss = self.loss(sem_seg, ood_score, target).mean()
    loss.backward()
    self.optimizer.step()
    return loss.detach()


def test_without_a_process_group_both_steps_are_bit_identical_to_their_former_bodies():
    from multishiftseg_amd import M2FStage1Step, M2FTrainStep, build_m2f_optimizer
    from multishiftseg_amd.loss import RelContrastiveLoss
    if _STOPPED:
        pytest.fail(f"no further GPU work is started: {_STOPPED[0]}")
    assert not dist.is_initialized()
    model = _model()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crit = _criterion()
    images, targets = _batch(0, COUNTS["plain"][0])
    inject = _tables(crit, 0, 3)
    got = {}
    for new in (True, False):
        model.load_state_dict(state)
        model.set_trainable()
        try:
            step = M2FTrainStep(model, crit, build_m2f_optimizer(model, base_lr=BASE_LR, weight_decay=0.05, clip_value=0.01))
            assert step.sync is None and step.counts is None
            losses, norm = step(images, targets=targets, **inject) if new else _old_train_step(step, images, targets=targets, **inject)
        finally:
            model.set_trainable(False)
        got[new] = (losses, norm, {n: p.detach().clone() for n, p in model.named_parameters()})
        for p in model.parameters():
            p.grad = None
    assert list(got[True][0]) == list(got[False][0]) and all(torch.equal(got[True][0][k], got[False][0][k]) for k in got[True][0])
    assert torch.equal(got[True][1], got[False][1])
    moved = [n for n in got[True][2] if not torch.equal(got[True][2][n], state[n])]
    assert len(moved) > 100 and all(torch.equal(got[True][2][n], got[False][2][n]) for n in got[True][2])
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    s1 = {}
    try:
        for new in (True, False):
            model.load_state_dict(state)
            step = M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="reference"))
            assert step.sync is None
            imgs, target = _stage1_inputs(0)
            torch.manual_seed(11)
            loss = step(imgs, target.clone()) if new else _old_stage1_step(step, imgs, target.clone())
            head = model.sem_seg_head.predictor.class_embed2
            s1[new] = (loss, head.weight.detach().clone(), head.bias.detach().clone())
            for p in model.parameters():
                p.grad = None
    finally:
        for n, p in model.named_parameters():
            p.requires_grad = flags[n]
    assert all(torch.equal(x, y) for x, y in zip(s1[True], s1[False]))
    assert not torch.equal(s1[True][1], state["sem_seg_head.predictor.class_embed2.weight"])
