"""CPU: what of the sharded validation sweep needs no GPU -- ddp.shard_batches' partition rule, OODMeter.merge's refusal (the ids
are compared before any tensor is touched), OODMeter.all_gather without a process group, and the signatures of both evaluate()
methods. The exchange itself is tests/test_gpu_ood_ranks.py."""
import inspect

import pytest
import torch.distributed as dist


class _NoLen:
    """An iterable that can only be walked: len() raises TypeError (no __len__), indexing too."""

    def __init__(self, n):
        self.n = n
        self.walks = 0

    def __iter__(self):
        self.walks += 1
        return (f"item{k}" for k in range(self.n))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_batches_partitions_a_generator_in_order(world):
    from multishiftseg_amd import ddp
    items = [f"item{k}" for k in range(7)]
    shards = []
    for rank in range(world):
        src = _NoLen(7)
        got = ddp.shard_batches(src, rank, world)
        assert inspect.isgenerator(got) and src.walks == 0               # lazy: nothing is consumed before the sweep asks
        shards.append(list(got))
        assert src.walks == 1
    assert shards == [items[r::world] for r in range(world)]              # shard_pairs' rule, k mod world == rank, order kept
    assert sorted(sum(shards, []), key=items.index) == items              # a partition: every item once
    assert all(shards[r] == [] for r in range(7, world))                  # ranks beyond the item count get nothing
    assert [[int(s[4:]) for s in sh] for sh in shards] == [ddp.shard_pairs(7, r, world) for r in range(world)]


def test_shard_batches_defaults_to_one_rank_without_a_process_group():
    import multishiftseg_amd as pkg
    from multishiftseg_amd import ddp
    assert not dist.is_initialized()
    assert list(ddp.shard_batches(k for k in range(5))) == [0, 1, 2, 3, 4]
    assert list(ddp.shard_batches(iter(range(5)), world=2)) == [0, 2, 4] and list(ddp.shard_batches(iter(range(5)), rank=1, world=2)) == [1, 3]
    assert "shard_batches" in pkg.__all__ and pkg.shard_batches is ddp.shard_batches


def test_merge_refuses_another_question_without_a_gpu():
    from multishiftseg_amd.metric import OODMeter
    for other in (OODMeter(train_id_in=2), OODMeter(train_id_out=3), OODMeter(recall_level=0.9)):
        with pytest.raises(ValueError, match="OODMeter.merge"):
            OODMeter().merge(other)
    a, b = OODMeter(), OODMeter()
    assert a.merge(b) is a and a.compute() is None and b.compute() is None            # two empty meters: nothing to touch


def test_all_gather_without_a_process_group_returns_the_meter():
    from multishiftseg_amd.metric import OODMeter
    assert not dist.is_initialized()
    m = OODMeter()
    assert m.all_gather() is m and m.all_gather() is m                    # nothing ran: nothing to count twice
    assert m.compute() is None


def test_both_evaluates_take_group_none_by_signature():
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.maskformer import MaskFormer
    for cls in (DeepWV3Plus, MaskFormer):
        params = inspect.signature(cls.evaluate).parameters
        assert list(params) == ["self", "batches", "meter", "seg_meter", "group"]
        assert all(params[k].default is None for k in ("meter", "seg_meter", "group"))
