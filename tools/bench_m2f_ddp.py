"""Times the whole-model stage-2 step of Mask2Former under data parallelism (m2f_trainer.M2FTrainStep over a process group) on the
full-size model of tools/bench_m2f_stage1.py -- R50 with freeze(1, norms=True), six encoder layers, nine decoder layers, 100
queries, 19 classes, synthetic weights -- with SetCriterion (labels + masks, deep supervision, 12544 points) and the clipped AdamW,
at 8 x 3 x 384 x 768 and 2 x 3 x 1024 x 2048 per rank.

    python tools/bench_m2f_ddp.py [--ranks 1,2,4,8] [--sizes 8x384x768,2x1024x2048] [--rounds 5] [--iters 10] [--out FILE.json]
    python tools/bench_m2f_ddp.py --count            # bytes per step from the parameter list; host only, no GPU

The tool starts its ranks itself: fresh child processes (at most 8, one per GPU, backend nccl = RCCL), each under --rank-timeout
seconds; rank 0's JSON lines are relayed. A rank count the box has no GPUs for is reported as not run (--backend gloo puts the ranks
on one GPU: a function check, its times say nothing about RCCL).

  1 rank:   the cost of the sink. Three contenders share one model and alternate round by round in one process:
            `plain`   the step as it was before it knew about process groups (its former body, kept below; no hooks attached),
            `ddp`     the step over the one-rank RCCL group with the collectives forced on (MSS_DDP_FORCE=1),
            `no_comm` the same with the collectives skipped (MSS_DDP_NO_COMM=1).
            ddp - plain is what the hooks, the scaled copy into the buckets and the one-rank collectives cost.
  N ranks:  `ddp` and `no_comm` alternate; ddp - no_comm is the EXPOSED communication.

Per contender and round, --iters steps run between two host clock readings, the second after a device synchronise; `enqueue_ms` is
the host time until the last launch of those steps had returned (a step whose enqueue time equals its step time is host-bound).
Medians over --rounds, with min and max. Every shape is warmed first with every contender."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = "8x384x768,2x1024x2048"
DEC_LAYERS, POINTS, TARGETS_PER_IMAGE = 9, 12544, 8


GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=DEC_LAYERS, pre_norm=False, mask_dim=256,
            enforce_input_project=False)


def build(device):
    """(model, criterion) of the timed step: the model of tools/bench_m2f_stage1.py. device None: on the host, for --count."""
    import torch
    import ref_resnet as RR
    import ref_transformer_decoder as RT
    from multishiftseg_amd import HungarianMatcher, MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, SetCriterion, build_resnet_backbone, m2f_weight_dict
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(0)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=1024,
                                       transformer_enc_layers=6, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    predictor.load_state_dict(RT.synth_state_dict(41), strict=True)
    model = MaskFormer(backbone, decoder, predictor).eval()
    weight_dict = m2f_weight_dict(2.0, 5.0, 5.0, 1.0, DEC_LAYERS + 1, True)
    crit = SetCriterion(19, HungarianMatcher(2.0, 5.0, 5.0, num_points=POINTS), weight_dict, 0.1, ["labels", "masks"], POINTS, 3.0, 0.75, None, None,
                        True)
    if device is not None:
        model, crit = model.to(device), crit.to(device)
    model.backbone.freeze(1, norms=True)
    return model, crit


def count():
    """Bytes one step's gradient all-reduces move per rank, from the parameter list (what GradAllReduce.bytes_per_step reports)."""
    from multishiftseg_amd import build_m2f_param_groups
    model, _ = build(None)
    groups = build_m2f_param_groups(model, 1e-4, 0.05)
    by = {}
    for n, p in model.named_parameters():
        if p.requires_grad:
            part = "backbone" if n.startswith("backbone.") else n.split(".")[1]
            by[part] = by.get(part, 0) + p.numel() * 4
    total = sum(g["params"][0].numel() * 4 for g in groups)
    buckets, cur = 0, 0
    for g in reversed(groups):                                       # ddp.GradAllReduce's rule at 64 MB, no tensor reaches 16 MB
        nbytes = g["params"][0].numel() * 4
        if cur and cur + nbytes > 64 << 20:
            buckets, cur = buckets + 1, 0
        cur += nbytes
    print(json.dumps(dict(tensors=len(groups), bytes_per_step=total, MB=total / 2 ** 20, by_part_bytes=by, buckets_at_64MB=buckets + (cur > 0),
                          largest_tensor_bytes=max(g["params"][0].numel() * 4 for g in groups))))


def _plain_step(step, *head_args, targets, **criterion_kwargs):
    """M2FTrainStep.__call__ before the step knew about process groups: the yardstick of the one-rank comparison."""
    from multishiftseg_amd import weighted_losses
    step.optimizer.zero_grad(set_to_none=True)
    outputs = step.head(*head_args)
    losses = weighted_losses(step.criterion(outputs, targets, **criterion_kwargs), step.criterion.weight_dict)
    sum(losses.values()).backward()
    norm = step.optimizer.step()
    return {k: v.detach() for k, v in losses.items()}, norm


def child(args):
    import torch
    import torch.distributed as dist
    from multishiftseg_amd import M2FTrainStep, build_m2f_optimizer
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    ndev = torch.cuda.device_count()
    if ndev < 1 or (args.backend == "nccl" and ndev < world):
        print(json.dumps(dict(ranks=world, not_run=f"{world} RCCL ranks need {world} GPUs, this box shows {ndev}")), flush=True)
        return 3
    dev = torch.device("cuda", rank % ndev)
    torch.cuda.set_device(dev)
    if args.backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    os.environ["MSS_DDP_FORCE"] = "1"
    model, crit = build(dev)
    model.set_trainable()

    def make(no_comm):
        os.environ["MSS_DDP_NO_COMM"] = "1" if no_comm else "0"
        try:
            step = M2FTrainStep(model, crit, build_m2f_optimizer(model, base_lr=1e-5, weight_decay=0.05, clip_value=0.01))
        finally:
            os.environ.pop("MSS_DDP_NO_COMM")
        step.sync.detach()                                           # one contender's hooks at a time (they share the parameters)
        return step
    steps = {"ddp": make(False), "no_comm": make(True)}
    if world == 1:
        os.environ["MSS_DDP_FORCE"] = "0"
        steps = {"plain": M2FTrainStep(model, crit, build_m2f_optimizer(model, base_lr=1e-5, weight_decay=0.05, clip_value=0.01)), **steps}
        assert steps["plain"].sync is None
    sink = steps["ddp"].sync
    head = dict(ranks=world, backend=args.backend, device=torch.cuda.get_device_name(dev), tensors=len(sink.where), buckets=len(sink.buckets),
                bytes_per_step=sink.bytes_per_step, rounds=args.rounds, iters=args.iters)
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        g = torch.Generator().manual_seed(10 + rank)
        images = torch.rand((B, 3, H, W), generator=g).to(dev)
        targets = [{"labels": torch.randperm(19, generator=g)[:TARGETS_PER_IMAGE].to(dev),
                    "masks": (torch.rand((TARGETS_PER_IMAGE, H // 8, W // 8), generator=g) < 0.5).repeat_interleave(8, 1).repeat_interleave(8, 2).to(dev)}
                   for _ in range(B)]

        def run(name, n):
            step = steps[name]
            if step.sync is not None:
                step.sync.attach()
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    _plain_step(step, images, targets=targets) if name == "plain" else step(images, targets=targets)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
            finally:
                if step.sync is not None:
                    step.sync.detach()
            return (t2 - t0) * 1e3 / n, (t1 - t0) * 1e3 / n
        for name in steps:
            run(name, 2)
        ms = {name: ([], []) for name in steps}
        for _ in range(args.rounds):
            for name in steps:
                total, enqueue = run(name, args.iters)
                ms[name][0].append(total)
                ms[name][1].append(enqueue)
        entry = dict(head, shape=[B, 3, H, W], peak_GB=torch.cuda.max_memory_allocated(dev) / 2 ** 30)
        for name, (total, enqueue) in ms.items():
            entry[name] = dict(step_ms=statistics.median(total), min_ms=min(total), max_ms=max(total), enqueue_ms=statistics.median(enqueue))
        entry["exposed_comm_ms"] = entry["ddp"]["step_ms"] - entry["no_comm"]["step_ms"]
        if world == 1:
            entry["sink_cost_ms"] = entry["ddp"]["step_ms"] - entry["plain"]["step_ms"]
            entry["sink_cost_without_collectives_ms"] = entry["no_comm"]["step_ms"] - entry["plain"]["step_ms"]
        if rank == 0:
            print(json.dumps(entry), flush=True)
        del images, targets
        torch.cuda.empty_cache()
    dist.barrier()
    dist.destroy_process_group()
    return 0


def launch(world, args):
    """`world` fresh rank processes, each under its own limit -> rank 0's JSON lines."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--backend", args.backend, "--sizes", args.sizes, "--rounds", str(args.rounds),
               "--iters", str(args.iters)]
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, text=True))
    deadline = time.monotonic() + args.rank_timeout
    failed = None
    try:
        while failed is None and any(p.poll() is None for p in procs):
            for rank, p in enumerate(procs):
                if p.poll() not in (None, 0, 3):         # the first bad status ends the run: its peers wait in a collective
                    failed = f"rank {rank} of {world} ended with status {p.returncode}"
                    break
            else:
                if time.monotonic() >= deadline:
                    failed = f"a rank of {world} ran past {args.rank_timeout} s"
                time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    if failed is None:
        bad = [(rank, p.returncode) for rank, p in enumerate(procs) if p.returncode not in (0, 3)]
        failed = f"rank {bad[0][0]} of {world} ended with status {bad[0][1]}" if bad else None
    out = procs[0].stdout.read()
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    if failed:
        raise SystemExit(f"bench_m2f_ddp.py: {failed}; nothing further is started")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1", help="rank counts to run one after the other, each at most 8 (e.g. 1,2,4,8)")
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="steps per contender and round: a window of about a second")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--rank-timeout", type=float, default=900.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.count:
        return count()
    if args.child:
        sys.exit(child(args))
    worlds = [int(v) for v in args.ranks.split(",")]
    if any(w < 1 or w > 8 for w in worlds):
        raise SystemExit("--ranks: between 1 and 8 ranks")
    results = []
    for world in worlds:
        for line in launch(world, args):
            print(json.dumps(line), flush=True)
            results.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
