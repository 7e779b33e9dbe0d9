"""CPU (gloo, spawned ranks, stock nn modules): the hook mode of ddp.GradAllReduce -- gradients taken from the parameters by
post-accumulate-grad hooks instead of from one hand-written backward -- the normaliser of Mask2Former's criterion over ranks,
and the data-parallel wiring of m2f_trainer.M2FTrainStep around a stand-in criterion and optimizer (the real ones are GPU only:
tests/test_gpu_m2f_ddp.py).

Equality: every rank scales its gradient by 1/2 (exact) and the sum of two terms does not depend on their order, so the averaged
gradient is torch.equal to 0.5 * (g0 + g1) of the recorded local gradients.

No test waits for a hang to fail: the parent joins its workers under LIMIT seconds (a worker takes about 3 s, most of it the
import of torch), terminates them when it expires and fails. Nothing is tried twice."""
import os
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

LIMIT = 120.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(worker, world, *args):
    """mp.spawn under a limit -> {rank: what the worker stored}. A worker that raises fails the test with its traceback."""
    mgr = mp.Manager()
    out = mgr.dict()
    ctx = mp.spawn(worker, args=(world, _free_port(), out) + args, nprocs=world, join=False)
    deadline = time.monotonic() + LIMIT
    try:
        while not ctx.join(timeout=max(deadline - time.monotonic(), 0.01)):
            if time.monotonic() >= deadline:
                pytest.fail(f"the ranks did not finish within {LIMIT:.0f} s (finished: {sorted(dict(out))})")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
                p.join(10)
    return dict(out)


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.environ.pop("MSS_DDP_FORCE", None)
    os.environ.pop("MSS_DDP_NO_COMM", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3), torch.nn.LayerNorm(3))


def _record(named):
    """Tensor hooks run before AccumulateGrad: the local gradient, cloned before the sink sees it."""
    rec, order = {}, []
    for n, p in named:
        def hook(g, n=n):
            rec[n] = g.detach().clone()
            order.append(n)
        p.register_hook(hook)
    return rec, order


def _averaging_worker(rank, world, port, out):
    from multishiftseg_amd import ddp
    _init(rank, world, port)
    net = _net()
    named = list(net.named_parameters())
    sink = ddp.GradAllReduce(list(reversed(named)), bucket_bytes=100).attach()          # 100 bytes: several buckets
    assert sink.active and len(sink.buckets) >= 3 and len(sink._handles) == len(named)
    assert [n for b in sink.buckets for n in b] == [n for n, _ in reversed(named)]
    rec, _ = _record(named)
    res = {}
    for step in range(2):                                                               # the second step reuses the buffers
        for _, p in named:
            p.grad = None
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * step + rank))
        net(x).square().sum().backward()
        sink.backward_done()
        views = all(p.grad.data_ptr() == sink.flat[sink.where[n][0]].data_ptr() + 4 * sink.where[n][1] for n, p in named)
        res[step] = dict(local={n: g.clone() for n, g in rec.items()}, grad={n: p.grad.clone() for n, p in named}, views=views)
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_hook_mode_delivers_the_exact_average_as_a_view_of_the_bucket():
    res = _run(_averaging_worker, 2)
    assert sorted(res) == [0, 1]
    for step in range(2):
        a, b = res[0][step], res[1][step]
        assert a["views"] and b["views"]
        assert len(a["local"]) == 6
        for n in a["local"]:
            assert not torch.equal(a["local"][n], b["local"][n]), n                     # the ranks had different batches
            want = 0.5 * (a["local"][n] + b["local"][n])
            assert torch.equal(a["grad"][n], want) and torch.equal(b["grad"][n], want), (step, n)


def _deadlock_worker(rank, world, port, out):
    from multishiftseg_amd import ddp
    _init(rank, world, port)
    torch.manual_seed(1)
    a, b, c = (torch.nn.Parameter(torch.randn(5)) for _ in range(3))
    named = [("a", a), ("b", b), ("c", c)]
    sink = ddp.GradAllReduce(list(reversed(named)), bucket_bytes=4).attach()            # one bucket a tensor: c, b, a
    assert sink.buckets == [["c"], ["b"], ["a"]]
    rec, order = _record(named)
    x = torch.arange(1.0, 6.0) * (rank + 1)
    if rank == 0:
        y = ((x * a) * b) * c                                                           # gradients arrive c, b, a: bucket order
    else:
        y = (x * b) * a                                                                 # a first, then b; c never
    y.sum().backward()
    sink.backward_done()
    out[rank] = dict(order=list(order), local=dict(rec), grad={n: p.grad.clone() for n, p in named},
                     c_is_view=c.grad.data_ptr() == sink.flat[0].data_ptr())
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_that_produce_gradients_in_other_orders_or_not_at_all_still_finish():
    res = _run(_deadlock_worker, 2)
    assert sorted(res) == [0, 1]                                                        # both ranks finished
    assert res[0]["order"] == ["c", "b", "a"] and res[1]["order"] == ["a", "b"]         # what the test set out to provoke
    for n in ("a", "b"):
        want = 0.5 * (res[0]["local"][n] + res[1]["local"][n])
        assert torch.equal(res[0]["grad"][n], want) and torch.equal(res[1]["grad"][n], want), n
    half = 0.5 * res[0]["local"]["c"]                                                   # the missing one travelled as zeros
    assert bool(half.any()) and torch.equal(res[0]["grad"]["c"], half) and torch.equal(res[1]["grad"]["c"], half)
    assert res[0]["c_is_view"] and not res[1]["c_is_view"]


def _contract_worker(rank, world, port, out):
    from multishiftseg_amd import ddp
    _init(rank, world, port)
    net = _net()
    named = list(net.named_parameters())
    sink = ddp.GradAllReduce(list(reversed(named))).attach()
    x = torch.randn(4, 6, generator=torch.Generator().manual_seed(rank))
    net(x).sum().backward()
    sink.backward_done()
    first = {n: p.grad.clone() for n, p in named}
    raised = ""
    try:
        net(x).sum().backward()                                                         # no zero_grad in between
    except RuntimeError as e:
        raised = str(e)
    sink.abort()
    for _, p in named:
        p.grad = None                                                                   # zero_grad(set_to_none=True)
    net(x).sum().backward()
    sink.backward_done()
    again = all(torch.equal(p.grad, first[n]) for n, p in named)
    # the average handed to a parameter WITHOUT a local gradient is under the same contract; a tensor that NO rank produced a
    # gradient for keeps .grad None, as in a one-process step
    w, u, v = (torch.nn.Parameter(torch.ones(3)) for _ in range(3))
    sink2 = ddp.GradAllReduce([("w", w), ("u", u), ("v", v)]).attach()
    ((w * 2.0 + u * 3.0) if rank == 0 else (w * 2.0)).sum().backward()
    sink2.backward_done()
    got_u = u.grad is not None and torch.equal(u.grad, torch.full((3,), 1.5)) and v.grad is None
    w.grad = None
    raised_u = ""
    try:
        (w * 2.0 + u).sum().backward()                                                  # u.grad was never set to None
    except RuntimeError as e:
        raised_u = str(e)
    sink2.abort()
    # detach(): no hooks, stock autograd again
    sink2.detach()
    w.grad = u.grad = None
    (w * 3.0).sum().backward()
    plain = torch.equal(w.grad, torch.full((3,), 3.0)) and w.grad.data_ptr() != sink2.flat[0].data_ptr()
    out[rank] = dict(raised=raised, again=again, got_u=got_u, raised_u=raised_u, plain=plain)
    dist.barrier()
    dist.destroy_process_group()


def test_a_second_backward_without_zero_grad_raises_the_contract_error():
    res = _run(_contract_worker, 2)
    for rank in (0, 1):
        r = res[rank]
        assert "zero_grad(set_to_none=True)" in r["raised"] and "is still defined at backward time" in r["raised"], r["raised"]
        assert r["again"] and r["got_u"] and r["plain"]
        assert "u.grad is still defined" in r["raised_u"], r["raised_u"]


def test_normaliser_rule():
    from multishiftseg_amd import ddp
    assert ddp.global_num_masks((3, 5)) == 4.0
    assert ddp.global_num_masks((0, 0)) == 1.0
    assert ddp.global_num_masks((0, 1)) == 1.0
    assert ddp.global_num_masks((7,)) == 7.0 and ddp.global_num_masks((1, 2, 2, 2)) == 1.75
    assert ddp.global_num_masks((8,), 2) == 4.0 and ddp.global_num_masks((1,), 2) == 1.0        # the all-reduced total, as the step passes it


class _Criterion:
    """Stand-in for SetCriterion: one loss normalised by num_masks, which it records."""
    weight_dict = {"loss_mask": 2.0}

    def __init__(self):
        self.seen = []

    def __call__(self, outputs, targets, *, num_masks=None):
        own = max(sum(int(t["labels"].shape[0]) for t in targets), 1)
        self.seen.append(num_masks)
        return {"loss_mask": outputs.square().sum() / (own if num_masks is None else num_masks), "loss_unweighted": outputs.sum()}


class _SGD:
    """Stand-in for optim.AdamW: .params, zero_grad, step() -> the norm of what it finds in .grad."""

    def __init__(self, params):
        self.params = list(params)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self):
        gs = [p.grad for p in self.params if p.grad is not None]
        for p in self.params:
            if p.grad is not None:
                p.sub_(0.1 * p.grad)
        return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs]))


def _targets(count):
    return [{"labels": torch.zeros(count - count // 2, dtype=torch.int64)}, {"labels": torch.zeros(count // 2, dtype=torch.int64)}]


def _step_worker(rank, world, port, out, counts):
    from multishiftseg_amd import M2FTrainStep, target_count
    _init(rank, world, port)
    net = _net(seed=rank)                                                               # different initial values: the broadcast must fix it
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    crit = _Criterion()
    step = M2FTrainStep(net, crit, _SGD(net.parameters()), bucket_bytes=100)
    assert step.sync is not None and step.sync.active and len(step.sync.buckets) >= 3
    assert [n for b in step.sync.buckets for n in b] == [n for n, _ in reversed(list(net.named_parameters()))]
    synced = {n: p.detach().clone() for n, p in net.named_parameters()}
    targets = _targets(counts[rank])
    assert target_count(targets) == counts[rank]
    res = dict(start=start, synced=synced, losses=[], norms=[])
    for k in range(2):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * k + rank))
        if k == 0:
            with torch.no_grad():
                res["own_loss"] = float(2.0 * net(x).square().sum() / max(counts[rank], 1))
        losses, norm = step(x, targets=targets)
        res["losses"].append({n: float(v) for n, v in losses.items()})
        res["norms"].append(norm.clone())
    res["num_masks"] = list(crit.seen)
    res["last"] = step.last_num_masks
    # a caller's num_masks wins; an exception in the head leaves the step usable
    step(x, targets=targets, num_masks=2.5)
    res["given"] = crit.seen[-1]

    def broken(x):
        raise KeyError("head")
    good, step.head = step.head, broken
    try:
        step(x, targets=targets)
        res["raised"] = False
    except KeyError:
        res["raised"] = True
    step.head = good
    step(x, targets=targets)
    res["params"] = {n: p.detach().clone() for n, p in net.named_parameters()}
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("counts,want", [((3, 5), 4.0), ((0, 1), 1.0)])
def test_train_step_wiring_over_two_ranks(counts, want):
    res = _run(_step_worker, 2, counts)
    a, b = res[0], res[1]
    for n in a["start"]:
        assert not torch.equal(a["start"][n], b["start"][n]) or n.startswith("3.")     # (the LayerNorm starts at 1 / 0 everywhere)
        assert torch.equal(a["synced"][n], a["start"][n]) and torch.equal(b["synced"][n], a["start"][n]), n   # rank 0's values
        assert torch.equal(a["params"][n], b["params"][n]) and not torch.equal(a["params"][n], a["start"][n]), n
    for r in (a, b):
        assert r["num_masks"][:2] == [want, want] and r["given"] == 2.5 and r["raised"] and r["last"] == want
        assert list(r["losses"][0]) == ["loss_mask"]
    assert torch.equal(a["norms"][0], b["norms"][0]) and torch.equal(a["norms"][1], b["norms"][1])
    assert a["losses"][0] != b["losses"][0]                                             # the returned losses stay rank-local
    if counts == (3, 5):
        assert a["losses"][0]["loss_mask"] != pytest.approx(a["own_loss"], rel=1e-3)    # normalised by 4, not by this rank's 3
        assert a["losses"][0]["loss_mask"] == pytest.approx(a["own_loss"] * 3 / 4, rel=1e-5)


def test_without_a_process_group_the_steps_attach_nothing():
    from multishiftseg_amd import M2FTrainStep, attach_grad_sync
    assert not dist.is_initialized()
    net = _net()
    crit = _Criterion()
    step = M2FTrainStep(net, crit, _SGD(net.parameters()))
    assert step.sync is None and step.counts is None and attach_grad_sync(net.parameters(), net) is None
    step(torch.randn(4, 6), targets=_targets(3))
    assert crit.seen == [None] and step.last_num_masks is None
    assert all(not getattr(p, "_post_accumulate_grad_hooks", None) for p in net.parameters())


class _Tiny(torch.nn.Module):
    """A body and a class_embed2 head: what the stage switch needs of a model."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.body, self.class_embed2 = torch.nn.Linear(6, 5), torch.nn.Linear(5, 3)

    def forward(self, x):
        return self.class_embed2(torch.tanh(self.body(x)))


def _switch_worker(rank, world, port, out):
    from multishiftseg_amd import M2FStage1Step, M2FTrainStep
    _init(rank, world, port)
    model = _Tiny()
    stage1 = M2FStage1Step(model, loss=None)                                            # its optimizer is built on the host; it is not stepped here
    r = dict(stage1_hooks=len(stage1.sync._handles), frozen=[n for n, p in model.named_parameters() if not p.requires_grad])
    for p in model.parameters():                                                        # update_trainable_params: stage 2 trains everything
        p.requires_grad_(True)
    try:
        M2FTrainStep(model, _Criterion(), _SGD(model.parameters()))
        r["refused"] = ""
    except RuntimeError as e:
        r["refused"] = str(e)
    stage1.close()
    try:
        stage1(torch.zeros(2, 6), None)
        r["closed_raises"] = False
    except RuntimeError as e:
        r["closed_raises"] = "closed" in str(e)
    step = M2FTrainStep(model, _Criterion(), _SGD(model.parameters()), bucket_bytes=100)
    named = list(model.named_parameters())
    rec, _ = _record(named)
    r["bad"] = []
    for k in range(2):
        x = torch.randn(4, 6, generator=torch.Generator().manual_seed(10 * k + rank))
        step(x, targets=_targets(3))
        for n, p in named:
            both = [torch.empty_like(rec[n]) for _ in range(world)]
            dist.all_gather(both, rec[n])
            if not torch.equal(p.grad, 0.5 * (both[0] + both[1])) or torch.equal(both[0], both[1]):
                r["bad"].append((k, n))
    out[rank] = r
    dist.barrier()
    dist.destroy_process_group()


def test_stage_switch_on_one_model_needs_close_and_then_averages_exactly():
    """Stage 1, then stage 2 on the same model (train_m2f.py's order): a second sink on class_embed2 would scale its gradient by
    1/world twice, so building stage 2 raises until stage 1 is closed; after close() every gradient, class_embed2's included, is
    the exact average on both steps."""
    res = _run(_switch_worker, 2)
    for rank in (0, 1):
        r = res[rank]
        assert r["stage1_hooks"] == 2 and r["frozen"] == ["body.weight", "body.bias"]
        assert "already hands its gradient to another sink" in r["refused"] and "class_embed2" in r["refused"], r["refused"]
        assert r["closed_raises"] and r["bad"] == []

