"""Data parallelism for the training loop: one process per GPU, gradients of the *trainable subset*
averaged with bucketed all-reduces (RCCL over xGMI; backend "nccl" is RCCL on ROCm) launched from
inside the backward as soon as each gradient exists, on a side stream, so they overlap with the
remaining dgrad/wgrad kernels.

The reference only has single-process ``nn.DataParallel`` (train_deeplab.py:91): replicate +
scatter + gather of the full-resolution logits to device 0 every step. Here every rank keeps its own
(original, augmented) pairs -- local batch layout [orig...; aug...] so the loss's ``i <-> i + B/2``
pairing stays rank-local -- and only gradients travel: 19 KB in stage 1, 123 MB in
stage 2. xGMI is point-to-point (7 links x ~153 GB/s per GPU), so buckets are few and large.
"""
import torch
import torch.distributed as dist


class GradAllReduce:
    """Bucketed, overlapped gradient averaging. Use as ``model.grad_sink``.

    ``named_params``: (name, parameter) in the order the backward produces the gradients (heads first, ASPP last);
    consecutive names are grouped into buckets of at most ``bucket_bytes``. Every bucket owns ONE persistent flat buffer:
    a gradient is scaled by 1/world straight into its slice the moment it exists (one pass), the bucket is all-reduced IN
    PLACE on a side stream as soon as it is complete, and what autograd receives is the slice itself -- no concatenation,
    no division pass, no copy back (round 2 made three passes over the 123 MB of stage 2).

    The sequence of collectives never depends on which gradients a rank produced: buckets are launched strictly in index
    order (a complete bucket waits for its incomplete predecessors until ``backward_done``), every bucket is launched
    every step, and a gradient that did not arrive travels as zeros and still receives the average (it is assigned to
    ``param.grad`` of a parameter that requires grad) -- ranks can therefore never pair collectives of different sizes.

    Contract: every handled parameter's ``.grad`` must be None when its gradient arrives (``zero_grad(set_to_none=True)``,
    what TrainStep does): ``param.grad`` aliases the bucket buffer between steps. Violations raise.

    Two ways in: the call style above (DeepWV3Plus's own backward calls ``model.grad_sink(name, grad)``), and ``attach()``,
    which takes the gradients from the parameters themselves with post-accumulate-grad hooks (Mask2Former: dozens of nodes
    plus stock autograd). Layout, launch order and everything after the backward are the same in both.
    """

    def __init__(self, named_params, bucket_bytes=64 << 20, group=None, force=False, close_after_bytes=16 << 20):
        """close_after_bytes: a gradient at least this large closes its bucket, i.e. its all-reduce starts the moment it exists
        instead of waiting for the small gradients behind it (stage 2: the three 37.7 MB ASPP weight gradients each end a bucket
        and travel beside the next branch's GEMMs; the last bucket is the 8 MB of the two small branches).
        force: run the collectives even in a one-rank group (exercises the RCCL path on a single GPU; tests).
        MSS_DDP_NO_COMM=1 (bench / tests only): everything but the collective itself -- the exposed-communication probe."""
        import os
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())
        self.no_comm = os.environ.get("MSS_DDP_NO_COMM") == "1"
        self.buckets = []       # list of lists of names (fixed at construction: every rank reduces the same layout)
        self.where = {}         # name -> (bucket index, offset, numel)
        self.params = {}        # name -> parameter
        cur, cur_bytes = [], 0
        for name, p in named_params:
            self.params[name] = p
            nbytes = p.numel() * p.element_size()
            if cur and cur_bytes + nbytes > bucket_bytes:
                self.buckets.append(cur)
                cur, cur_bytes = [], 0
            cur.append(name)
            cur_bytes += nbytes
            if close_after_bytes and nbytes >= close_after_bytes:
                self.buckets.append(cur)
                cur, cur_bytes = [], 0
        if cur:
            self.buckets.append(cur)
        self.sizes = []
        for i, b in enumerate(self.buckets):
            off = 0
            for n in b:
                self.where[n] = (i, off, self.params[n].numel())
                off += self.params[n].numel()
            self.sizes.append(off)
        self.flat = [None] * len(self.buckets)          # persistent, allocated on first use
        self.comm_stream = None
        self.bytes_per_step = sum(self.sizes) * 4
        self._handles = []      # attach(): the hooks' handles
        self._hooked = []       # attach(): the parameters that carry them (each is marked with this sink: one sink a tensor)
        self._flag_group = None # attach(): where the per-tensor "some rank produced it" flags travel (host tensors, gloo)
        self._held = {}         # hook mode: name -> what this sink last left in param.grad (kept alive: its address identifies it)
        self._reset()

    def _reset(self):
        self.arrived = [set() for _ in self.buckets]
        self.next_bucket = 0
        self.inflight = []      # (bucket index, work)

    def _buffer(self, i):
        if self.flat[i] is None:
            p = self.params[self.buckets[i][0]]
            self.flat[i] = torch.zeros(self.sizes[i], dtype=p.dtype, device=p.device)
        return self.flat[i]

    def __call__(self, name, grad):
        """Returns the tensor to hand to autograd in place of `grad` (a view of the bucket's flat buffer, holding the
        average once backward_done() has returned), or None when this sink does not handle `name`."""
        if not self.active or name not in self.where:
            return None
        if self.params[name].grad is not None:
            # autograd steals the returned view as param.grad, so a gradient still defined from an earlier backward IS this
            # buffer: writing the new one would overwrite it and AccumulateGrad would then add the buffer to itself (silently
            # doubled gradients), and an accumulated sum would be all-reduced a second time. Accumulation over several
            # backwards is not what the reference loop does (train_deeplab.py:198-204: zero_grad / backward / step).
            raise RuntimeError(self._contract(name))
        return self._take(name, grad)

    def _contract(self, name):
        return (f"GradAllReduce: {name}.grad is still defined at backward time; call "
                "optimizer.zero_grad(set_to_none=True) before every backward (gradient accumulation and "
                "zero_grad(set_to_none=False) are not supported with the in-place bucket buffers)")

    def _take(self, name, grad):
        """grad / world into the slice of `name`, then every bucket that has become complete, in index order -> the slice."""
        i, off, n = self.where[name]
        view = self._buffer(i)[off:off + n].view(grad.shape)
        torch.mul(grad, 1.0 / self.world, out=view)
        self.arrived[i].add(name)
        while self.next_bucket < len(self.buckets) and len(self.arrived[self.next_bucket]) == len(self.buckets[self.next_bucket]):
            self._launch(self.next_bucket)
            self.next_bucket += 1
        return view

    def attach(self):
        """Hook mode, for a model made of many autograd nodes and stock autograd between them: instead of one hand-written
        backward calling the sink, every handled parameter that requires grad gets a post-accumulate-grad hook that does what
        __call__ does -- the local gradient, scaled by 1/world, goes into the parameter's slice of its bucket, `param.grad` is
        rebound to that slice and the complete buckets are launched. backward_done / flush / abort are used as before, with one
        addition (_produced_somewhere): a tensor that NO rank produced a gradient for keeps .grad None. Nothing is attached to
        an inactive sink (one rank, not forced). The flags travel over host_group(group). A tensor carries the hook of ONE sink:
        attach() raises where another sink still holds a parameter (detach() that one first). Returns self; detach() removes
        the hooks.

        The contract check of hook mode is narrower than the call style's: by the time the hook runs AccumulateGrad has already
        accumulated, so it recognises what THIS sink left in .grad at the previous step (the bucket slice, or the copy of the
        average) by its address. A .grad that somebody else assigned between the steps is accumulated into and averaged without
        an error, and so is an out-of-place accumulation (create_graph=True), which replaces the tensor."""
        if self.active and not self._handles:
            for name, p in self.params.items():
                other = getattr(p, "_mss_grad_sink", None)
                if p.requires_grad and other is not None and other is not self:
                    # two hooks on one tensor would each scale by 1/world, and the older sink's buckets are never finished
                    raise RuntimeError(f"GradAllReduce.attach: {name} already hands its gradient to another sink; detach() that one "
                                       "first (M2FStage1Step.close() / M2FTrainStep.close() at the stage switch)")
            self._flag_group = host_group(self.group)
            for name, p in self.params.items():
                if p.requires_grad:
                    p._mss_grad_sink = self
                    self._hooked.append(p)
                    self._handles.append(p.register_post_accumulate_grad_hook(lambda p, name=name: self._hook(name, p)))
        return self

    def detach(self):
        """Remove the hooks: the parameters are free for another sink (the stage switch), this one can attach() again."""
        for h in self._handles:
            h.remove()
        for p in self._hooked:
            if getattr(p, "_mss_grad_sink", None) is self:
                del p._mss_grad_sink
        self._handles, self._hooked = [], []

    @torch.no_grad()
    def _hook(self, name, p):
        g = p.grad
        held = self._held.get(name)
        if held is not None and g.data_ptr() == held.data_ptr():
            # AccumulateGrad found what the previous step handed over (the bucket slice, or the average given to a parameter
            # without a local gradient) still in place and added to it: the live gradient is gone and the sum would travel again
            raise RuntimeError(self._contract(name))
        p.grad = self._held[name] = self._take(name, g)

    def _launch(self, i):
        flat = self._buffer(i)
        for n in self.buckets[i]:                     # a gradient that is absent this step travels as zeros
            if n not in self.arrived[i]:
                _, off, cnt = self.where[n]
                flat[off:off + cnt].zero_()
        if self.no_comm:
            self.inflight.append((i, None))
            return
        if flat.is_cuda:
            if self.comm_stream is None:
                self.comm_stream = torch.cuda.Stream()
            self.comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                work = dist.all_reduce(flat, group=self.group, async_op=True)
        else:
            work = dist.all_reduce(flat, group=self.group, async_op=True)
        self.inflight.append((i, work))

    def flush(self):
        """Launch, in index order, every bucket that has not been launched yet (some gradient of it, or of a predecessor,
        did not arrive this step)."""
        while self.next_bucket < len(self.buckets):
            self._launch(self.next_bucket)
            self.next_bucket += 1

    def _produced_somewhere(self):
        """Hook mode: the names some rank produced a gradient for this step -- one all-reduce over a flag per tensor, issued by
        every rank after its last bucket. A tensor NO rank produced one for (a parameter the forward never uses) keeps .grad None
        as in a one-process step, so the optimizer skips it instead of decaying it with a zero gradient. The flags are host
        tensors on host_group(group): the host decides what the optimizer sees, and reading the answer from the device would
        make it wait for the whole backward every step. The all-reduce blocks the host until every rank's host has enqueued its
        backward (the hosts meet once per step; the devices are not waited for)."""
        names = [n for b in self.buckets for n in b]
        here = [any(n in a for a in self.arrived) for n in names]
        if self.no_comm:
            return {n for n, f in zip(names, here) if f}
        flags = torch.tensor([float(f) for f in here], dtype=torch.float32)
        dist.all_reduce(flags, group=self._flag_group)
        return {n for n, f in zip(names, flags.tolist()) if f > 0}

    def backward_done(self):
        if not self.active:
            return
        self.flush()
        produced = self._produced_somewhere() if self._handles else None
        for i, work in self.inflight:
            if work is not None:
                work.wait()      # CUDA: makes the current stream wait for the collective, no host block
            for n in self.buckets[i]:
                if n not in self.arrived[i]:
                    p = self.params[n]
                    # no local gradient this step, but the other ranks' average is this rank's too
                    if p.requires_grad and (produced is None or n in produced):
                        _, off, cnt = self.where[n]
                        p.grad = self.flat[i][off:off + cnt].view(p.shape).clone()
                        if self._handles:
                            self._held[n] = p.grad
        self._reset()

    def abort(self):
        """The backward is unwinding from an exception: start no further collective (the other ranks may never reach
        theirs), wait for the ones already in flight and forget this step's gradients."""
        for _, work in self.inflight:
            try:
                if work is not None:
                    work.wait()
            except Exception:
                pass
        self._reset()


def is_active(group=None):
    """The switch of every data-parallel step (trainer.TrainStep, m2f_trainer): torch.distributed is initialised and the group
    has more than one rank, or MSS_DDP_FORCE=1 asks for the collectives in a one-rank group too (the RCCL path on one GPU)."""
    import os
    return dist.is_initialized() and (dist.get_world_size(group) > 1 or os.environ.get("MSS_DDP_FORCE") == "1")


def broadcast_params(params, group=None):
    """Rank 0's values of `params` to every rank of the group, in place, once (construction time: one collective a tensor)."""
    src = dist.get_global_rank(group, 0) if group is not None else 0
    for p in params:
        dist.broadcast(p.detach(), src=src, group=group)     # in place on the shared storage: bumps the parameter's version


_HOST_GROUPS = {}


def host_group(group=None):
    """The group over which host tensors of `group`'s ranks travel: `group` itself where its backend has gloo, else ONE gloo
    group of the same ranks, created at the first call and shared by every sink and step of the process (a collective call: all
    ranks of `group` make it, in the same order; with a sub-group only its members do)."""
    if "gloo" in str(dist.get_backend(group)):
        return group
    key = (dist.group.WORLD, group)
    if key not in _HOST_GROUPS:
        if group is None:
            _HOST_GROUPS[key] = dist.new_group(backend="gloo")
        else:
            _HOST_GROUPS[key] = dist.new_group(ranks=dist.get_process_group_ranks(group), backend="gloo", use_local_synchronization=True)
    return _HOST_GROUPS[key]


def global_num_masks(sums, world=None):
    """The normaliser of Mask2Former's criterion over several processes (reference criterion.py:447-453): the ranks' target
    counts sum_b T_b are summed, divided by the world size and clamped at 1. `sums`: one count per rank (or, with `world`,
    any split of their total, as after an all-reduce) -> float."""
    return max(float(sum(sums)) / (len(sums) if world is None else world), 1.0)


class CountAllReduce:
    """global_num_masks as one tiny collective per step that no device stream is involved in: start(count) before the forward,
    result() before the criterion; a one-element host tensor over host_group(group). MSS_DDP_NO_COMM=1 skips the collective (the
    probe then normalises by its own count)."""

    def __init__(self, group=None):
        import os
        self.world = dist.get_world_size(group)
        self.group = host_group(group)
        self.no_comm = os.environ.get("MSS_DDP_NO_COMM") == "1"
        self._pending = None

    def drop(self):
        """The step is unwinding from an exception: forget a collective that was started, without waiting for it (a peer that
        failed earlier may never have started its own)."""
        self._pending = None

    def start(self, count):
        t = torch.tensor([float(count) * (self.world if self.no_comm else 1)], dtype=torch.float64)
        self._pending = (t, None if self.no_comm else dist.all_reduce(t, group=self.group, async_op=True))

    def result(self):
        t, work = self._pending
        self._pending = None
        if work is not None:
            work.wait()
        return global_num_masks((float(t.item()),), self.world)       # the ranks' sum is what travelled


def init_from_env():
    """(rank, world, local_rank, device) from the torchrun environment; initialises the default
    process group when WORLD_SIZE > 1 (backend nccl = RCCL on a GPU box, gloo otherwise)."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        ndev = torch.cuda.device_count()
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
        if local_world > ndev and os.environ.get("MSS_DIST_BACKEND") != "gloo":
            # a mis-sized launch: ranks would silently share GPUs (local_rank % ndev below) and the "per-GPU" numbers mean nothing
            import warnings
            warnings.warn(f"multishiftseg_amd.ddp: {local_world} local ranks on {ndev} visible GPU(s): ranks share devices "
                          f"(rank {rank} -> cuda:{local_rank % ndev}); launch with --nproc-per-node <= {ndev}", RuntimeWarning, stacklevel=2)
        torch.cuda.set_device(local_rank % ndev)
        device = torch.device("cuda", local_rank % ndev)
        backend = "nccl"
    else:
        device = torch.device("cpu")
        backend = "gloo"
    backend = os.environ.get("MSS_DIST_BACKEND", backend)   # tests: gloo with several ranks on one GPU
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend == "nccl":
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, local_rank, device


def shard_pairs(num_pairs, rank, world):
    """Pairs owned by `rank`: {k : k mod world == rank}."""
    return list(range(rank, num_pairs, world))


def shard_batches(batches, rank=None, world=None, group=None):
    """A rank's share of a validation sweep: the items k of any iterable with k mod world == rank (shard_pairs' rule), as a
    generator -- the iterable is walked once and never asked for its length. `rank` / `world` default to the group's, and to 0 / 1
    without an initialised process group. A rank beyond the item count gets nothing and still takes part in the collectives of
    evaluate(group=)."""
    up = dist.is_available() and dist.is_initialized()
    if world is None:
        world = dist.get_world_size(group) if up else 1
    if rank is None:
        rank = dist.get_rank(group) if up else 0
    for k, item in enumerate(batches):
        if k % world == rank:
            yield item


def gather_meters(group, meter, seg_meter=None):
    """The end of a sharded sweep (DeepWV3Plus.evaluate / MaskFormer.evaluate with group=): every rank of the group calls this
    once, a rank whose shard was empty too. `group` True stands for the default group. The OOD keys are gathered
    (OODMeter.all_gather), the confusion matrix is summed (SegMeter.all_reduce). A rank that raised inside its sweep never gets
    here: its peers wait in the collective until the process group's timeout ends them. There is no protocol for that."""
    group = None if group is True else group
    meter.all_gather(group)
    if seg_meter is not None:
        if seg_meter._table is None and torch.cuda.is_available() and is_active(group):
            seg_meter._counters(torch.device("cuda", torch.cuda.current_device()))      # an empty shard: a table where the peers' are
        seg_meter.all_reduce(group)
