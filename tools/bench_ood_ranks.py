"""Times the exchange at the end of a validation sweep that is split over ranks (OODMeter.all_gather): per rank 16
synthetic 1024 x 2048 score and label maps (3 % id_out, 5 % unlabelled, the rest id_in; seeded by the rank), no model.

    python tools/bench_ood_ranks.py [--ranks 1,2,4,8] [--maps 16] [--size 1024x2048] [--rounds 5] [--backend nccl|gloo] [--out FILE.json]

The tool starts its ranks itself: fresh child processes (at most 8, one per GPU, backend nccl = RCCL), each under --rank-timeout
seconds; rank 0's JSON lines are relayed. A rank count the box has no GPUs for is reported as not run (--backend gloo puts the ranks
on one GPU and stages the keys through the host: a function check of that path, its times say nothing about RCCL). With one rank the
collectives are forced on (MSS_DDP_FORCE=1): the one-rank RCCL group.

Per round, between host clock readings with a device synchronise before each:
  `update_ms`          update_many over the rank's own maps (what the sweep costs without a forward),
  `gather_compute_ms`  all_gather + compute() after it: the exchange, the sort of the union and the measures,
  `sweep_ms`           the two together, the forward-free sweep of a rank,
  `single_ms`          the yardstick: ONE process -- rank 0, its peers waiting at a barrier -- runs update_many + compute() over the
                       maps of all ranks on a meter that never meets a collective (OODMeter as it was before it could combine).
Every rank's gathered tuple must equal the single meter's with ==; the tool fails otherwise. Medians over --rounds with min and
max; one warm-up round first."""
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


def _maps(rank, n, H, W, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(10 + rank)
    maps = []
    for _ in range(n):
        u = torch.rand((1, H, W), device=dev, generator=g)
        label = (u < 0.03).long()
        label[u > 0.95] = 255
        maps.append((torch.randn((1, H, W), device=dev, generator=g) + 1.2 * (label == 1), label))
    return maps


def child(args):
    import torch
    import torch.distributed as dist
    from multishiftseg_amd.metric import OODMeter
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
    H, W = (int(v) for v in args.size.split("x"))
    mine = _maps(rank, args.maps, H, W, dev)
    everyone = [m for r in range(world) for m in (mine if r == rank else _maps(r, args.maps, H, W, dev))] if rank == 0 else None

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    ms = dict(update_ms=[], gather_compute_ms=[], sweep_ms=[], single_ms=[])
    keys = None
    for rnd in range(args.rounds + 1):                                    # round 0 warms every path
        dist.barrier()
        meter = OODMeter()
        t0 = clock()
        meter.update_many(mine)
        t1 = clock()
        got = meter.all_gather().compute()
        t2 = clock()
        keys = sum(t.numel() for t in meter.keys())
        del meter
        dist.barrier()
        want, t3, t4 = None, 0.0, 0.0
        if rank == 0:
            single = OODMeter()
            t3 = clock()
            single.update_many(everyone)
            want = single.compute()
            t4 = clock()
            del single
        box = [want]
        dist.broadcast_object_list(box, src=0)
        if got != box[0]:
            raise SystemExit(f"bench_ood_ranks.py: rank {rank} computed {got} after all_gather, one meter over every map {box[0]}")
        if rnd:
            for k, v in (("update_ms", t1 - t0), ("gather_compute_ms", t2 - t1), ("sweep_ms", t2 - t0), ("single_ms", t4 - t3)):
                ms[k].append(v * 1e3)
    if rank == 0:
        entry = dict(ranks=world, backend=args.backend, device=torch.cuda.get_device_name(dev), maps_per_rank=args.maps, map=[H, W],
                     rounds=args.rounds, union_keys=keys, key_MB_per_rank=keys * 4 / world / 2 ** 20, measures=list(got),
                     peak_GB=torch.cuda.max_memory_allocated(dev) / 2 ** 30)
        for k, v in ms.items():
            entry[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(json.dumps(entry), flush=True)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--backend", args.backend, "--size", args.size, "--maps", str(args.maps),
               "--rounds", str(args.rounds)]
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
        raise SystemExit(f"bench_ood_ranks.py: {failed}; nothing further is started")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="1", help="rank counts to run one after the other, each at most 8 (e.g. 1,2,4,8)")
    ap.add_argument("--maps", type=int, default=16, help="maps per rank")
    ap.add_argument("--size", default="1024x2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--rank-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
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
