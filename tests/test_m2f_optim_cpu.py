"""CPU: what the stage-2 optimizer rests on, without a GPU. The float64 restatement of tests/ref_adamw.py against stock torch, the
launch planner of csrc/m2f_optim.hip (host queries of the built library) on adversarial size lists, the parameter groups of
m2f_trainer.build_m2f_param_groups on a toy module tree, and the two dict helpers."""
import numpy as np
import pytest
import torch
from torch import nn

import ref_adamw as R


@pytest.fixture(scope="module")
def geometry():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib
    return (_lib.value("mss_adamw_chunk_elems"), _lib.value("mss_adamw_tensors_per_launch"), _lib.value("mss_adamw_blocks_per_launch"))


def test_restatement_matches_stock_torch_over_six_steps():
    """Pins the oracle, not the kernel: float64 restatement vs torch.optim.AdamW(foreach=False) + clip_grad_norm_(foreach=False) in
    float32, rtol 1e-5 on parameter deltas and both moments; steps clip and do not clip, one tensor misses two gradients."""
    sizes = [1, 3, 5, 257, 1000]
    case = R.parity_case(sizes, seed=3)
    assert any(c < 0.5 for c in case["coefs"]) and any(c == 1.0 and n > 0 for c, n in zip(case["coefs"], case["norms"]))
    out = R.torch_cpu_run(case["p0"], case["lrs"], case["wds"], case["grads"], max_norm=case["max_norm"])
    ref = R.RefAdamW(case["p0"], case["lrs"], case["wds"], max_norm=case["max_norm"])
    for k, row in enumerate(case["grads"]):
        norm = ref.step(row)
        ps, ms, vs, tnorm = out[k]
        np.testing.assert_allclose(float(tnorm), norm, rtol=1e-5)
        for i in range(len(sizes)):
            d_ref = ref.p[i] - case["p0"][i].astype(np.float64)
            d_got = ps[i].astype(np.float64) - case["p0"][i].astype(np.float64)
            # rtol 1e-5, plus what float32 storage itself adds where a value is small beside its tensor's operands (a delta beside
            # its parameter, a moment that cancelled): a spacing of the tensor's largest magnitude per step taken
            np.testing.assert_allclose(d_got, d_ref, rtol=1e-5, atol=(k + 1) * float(np.spacing(np.abs(ps[i]).max())))
            np.testing.assert_allclose(ms[i], ref.m[i], rtol=1e-5, atol=(k + 1) * float(np.spacing(np.abs(ms[i]).max())))
            np.testing.assert_allclose(vs[i], ref.v[i], rtol=1e-5, atol=(k + 1) * float(np.spacing(np.abs(vs[i]).max())))
    assert ref.t == [R.STEPS - len(R.NONE_STEPS) if i == case["none_tensor"] else R.STEPS for i in range(len(sizes))]


def test_restatement_skips_missing_gradients():
    ref = R.RefAdamW([np.ones(3), np.ones(2)], [1e-3, 1e-3], [0.1, 0.1], max_norm=1.0)
    norm = ref.step([None, np.array([3.0, 4.0])])
    assert norm == 5.0 and ref.t == [0, 1]
    assert np.array_equal(ref.p[0], np.ones(3)) and np.array_equal(ref.m[0], np.zeros(3))
    assert (ref.p[1] < 1).all()


def _adversarial_lists(chunk, tensors, blocks):
    return {
        "size_1": [1],
        "chunk_edges": [chunk - 1, chunk, chunk + 1, 1, 2 * chunk + 5],
        "empty_between": [5, 0, 7, 0],
        "more_tensors_than_a_launch": [7] * (tensors + 3),
        "exactly_one_launch_of_tensors": [3] * tensors,
        "two_full_tables": [2] * (2 * tensors),
        "more_chunks_than_a_launch": [chunk * 10 + 1] * (blocks // 10 + 2),
        "one_tensor_over_a_launch": [blocks * chunk + 2 * chunk + 3],
        "exactly_one_launch_of_blocks": [blocks * chunk],
        "cut_then_small": [5, blocks * chunk + 1, 9, chunk + 1] + [1] * (tensors + 1),
        "table_fills_on_a_cut_tensor": [1] * (tensors - 1) + [(blocks + 5) * chunk, 3],
        "empty": [],
    }


def test_planner_covers_every_element_exactly_once(geometry):
    from multishiftseg_amd import _lib
    from multishiftseg_amd.optim import adamw_launches, adamw_plan
    import ctypes
    chunk, tensors, blocks = geometry
    assert chunk % 4 == 0 and chunk >= 1024 and tensors >= 2 and blocks >= 2
    for name, sizes in _adversarial_lists(chunk, tensors, blocks).items():
        plan = adamw_plan(sizes)
        want_chunks = [-(-s // chunk) for s in sizes]
        assert len(plan) == sum(want_chunks), name
        arr = (ctypes.c_longlong * max(len(sizes), 1))(*sizes)
        assert _lib.value("mss_adamw_scratch_floats", len(sizes), arr) == sum(want_chunks), name
        seen, slots = set(), []
        per_launch = {}
        for launch, block, tensor, ck, slot in plan:
            assert 0 <= tensor < len(sizes) and 0 <= ck < want_chunks[tensor], (name, tensor, ck)
            assert (tensor, ck) not in seen, (name, tensor, ck)            # chunks partition a tensor: one workgroup per chunk
            seen.add((tensor, ck))
            slots.append(slot)
            per_launch.setdefault(launch, []).append((block, tensor))
        assert seen == {(t, c) for t, n in enumerate(want_chunks) for c in range(n)}, name
        assert sorted(slots) == list(range(len(plan))), name              # scratch slots: unique and dense
        assert sorted(per_launch) == list(range(len(per_launch))), name
        for launch, entries in per_launch.items():
            assert [b for b, _ in entries] == list(range(len(entries))), (name, launch)
            assert len(entries) <= blocks and len({t for _, t in entries}) <= tensors, (name, launch)
        n_launch = len(per_launch)
        assert adamw_launches(sizes, clip=False) == n_launch and adamw_launches(sizes, clip=True) == (2 * n_launch + 1 if n_launch else 0)
    assert len({l for l, *_ in adamw_plan([7] * (tensors + 3))}) == 2
    assert len({l for l, *_ in adamw_plan([blocks * chunk + 1])}) == 2


def test_step_entry_point_checks_its_arguments(geometry):
    """include/mss_hip.h's convention, on the host side of the call only (nothing is launched)."""
    import ctypes
    from multishiftseg_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_void_p * 1)(64)
    n1, lr, wd = (ctypes.c_longlong * 1)(8), (ctypes.c_double * 1)(1e-3), (ctypes.c_double * 1)(0.0)
    launches = ctypes.c_int(-1)

    def step(count, params, steps, clip=0, scratch=None):
        return lib.mss_adamw_clip_step_f32(count, params, one, one, one, n1, lr, wd, (ctypes.c_int * 1)(steps), 0.9, 0.999, 1e-8, clip, 1.0,
                                           scratch, 0, None, ctypes.byref(launches), None)
    assert step(0, None, 1) == 0 and launches.value == 0                    # the empty list
    assert step(1, None, 1) == _lib.MSS_ERR_BAD_ARG
    assert step(1, (ctypes.c_void_p * 1)(None), 1) == _lib.MSS_ERR_BAD_ARG  # a null tensor pointer
    assert step(1, one, 0) == _lib.MSS_ERR_BAD_ARG                          # step < 1
    assert step(1, one, 1, clip=1) == _lib.MSS_ERR_BAD_ARG                  # clipping without scratch / norm_out
    assert step(-1, one, 1) == _lib.MSS_ERR_BAD_ARG


class _Backbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        self.bn = nn.BatchNorm2d(4)
        self.absolute_pos_embed = nn.Parameter(torch.zeros(1, 4))


class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = _Backbone()
        self.ln = nn.LayerNorm(4)
        self.gn = nn.GroupNorm(2, 4)
        self.query_embed = nn.Embedding(5, 4)
        self.proj = nn.Linear(4, 4)
        self.proj_again = self.proj                       # the same Linear under a second name
        self.frozen = nn.Linear(4, 2, bias=False)
        self.frozen.weight.requires_grad_(False)
        self.relative_position_bias_table = nn.Parameter(torch.zeros(3, 2))


def test_param_groups_of_a_toy_tree():
    from multishiftseg_amd import build_m2f_optimizer, build_m2f_param_groups
    from multishiftseg_amd.optim import AdamW
    model = _Toy()
    groups = build_m2f_param_groups(model, 1e-5, 0.05, weight_decay_norm=0.0, weight_decay_embed=0.01, backbone_multiplier=0.1)
    names = {id(p): n for n, p in model.named_parameters()}                 # named_parameters() dedups: the first name of a shared tensor
    got = {names[id(g["params"][0])]: (g["lr"], g["weight_decay"]) for g in groups}
    assert all(len(g["params"]) == 1 for g in groups) and len(got) == len(groups)
    assert got == {
        "relative_position_bias_table": (1e-5, 0.0),
        "backbone.absolute_pos_embed": (1e-5 * 0.1, 0.0),
        "backbone.conv.weight": (1e-5 * 0.1, 0.05),
        "backbone.conv.bias": (1e-5 * 0.1, 0.05),
        "backbone.bn.weight": (1e-5 * 0.1, 0.0),
        "backbone.bn.bias": (1e-5 * 0.1, 0.0),
        "ln.weight": (1e-5, 0.0),
        "ln.bias": (1e-5, 0.0),
        "gn.weight": (1e-5, 0.0),
        "gn.bias": (1e-5, 0.0),
        "query_embed.weight": (1e-5, 0.01),
        "proj.weight": (1e-5, 0.05),
        "proj.bias": (1e-5, 0.05),
    }
    # a later rule overrides an earlier one: norm decay differs from 0 here, and reaches the norm layers only
    g2 = build_m2f_param_groups(model, 1e-5, 0.05, weight_decay_norm=0.3, weight_decay_embed=0.0)
    got2 = {names[id(g["params"][0])]: g["weight_decay"] for g in g2}
    assert got2["ln.weight"] == 0.3 and got2["backbone.bn.bias"] == 0.3 and got2["query_embed.weight"] == 0.0 and got2["proj.weight"] == 0.05
    opt = build_m2f_optimizer(model, base_lr=1e-5, weight_decay=0.05)
    assert isinstance(opt, AdamW) and opt.max_norm == 0.01 and len(opt.param_groups) == 13
    assert build_m2f_optimizer(model, clip_value=0.0).max_norm is None
    with pytest.raises(NotImplementedError):
        build_m2f_optimizer(model, optimizer="SGD")


def test_adamw_constructor_forms():
    from multishiftseg_amd.optim import AdamW
    a, b = nn.Parameter(torch.zeros(2)), nn.Parameter(torch.zeros(3))
    flat = AdamW([a, b], lr=2e-3, weight_decay=0.5)
    assert len(flat.param_groups) == 1 and flat.param_groups[0]["lr"] == 2e-3 and flat.param_groups[0]["weight_decay"] == 0.5
    grouped = AdamW([{"params": [a], "lr": 1.0}, {"params": [b], "weight_decay": 0.0}], lr=3.0, weight_decay=4.0)
    assert [(g["lr"], g["weight_decay"]) for g in grouped.param_groups] == [(1.0, 4.0), (3.0, 0.0)]
    assert grouped.params[0] is a and grouped.params[1] is b and grouped.step() is None      # no gradient anywhere: nothing to do
    with pytest.raises(ValueError):
        AdamW([{"params": [a]}, {"params": [a]}])
    a.grad = torch.ones(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        grouped.step()


def test_weight_dict_and_weighted_losses():
    from multishiftseg_amd import m2f_weight_dict, weighted_losses
    assert m2f_weight_dict(2.0, 5.0, 5.0, 1.5, 3, False) == {
        "loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "loss_ood": 1.5, "loss_original_mask": 5.0, "loss_original_dice": 5.0,
        "loss_aug_mask": 5.0, "loss_aug_dice": 5.0}
    deep = m2f_weight_dict(2.0, 5.0, 4.0, 1.5, 3, True)
    assert len(deep) == 24 and list(deep)[8] == "loss_ce_0"
    assert deep["loss_ce_1"] == 2.0 and deep["loss_dice_0"] == 4.0 and deep["loss_ood_1"] == 1.5 and "loss_ce_2" not in deep
    assert m2f_weight_dict(1, 1, 1, 1, 1, True) == m2f_weight_dict(1, 1, 1, 1, 1, False)
    table = torch.tensor([1.0, 2.0, 3.0])
    losses = {"loss_ce": table[0], "loss_unknown": table[1], "loss_dice": table[2]}
    keep = dict(losses)
    out = weighted_losses(losses, {"loss_dice": 5.0, "loss_ce": 2.0, "loss_mask": 7.0})
    assert list(out) == ["loss_ce", "loss_dice"] and float(out["loss_ce"]) == 2.0 and float(out["loss_dice"]) == 15.0
    assert losses.keys() == keep.keys() and all(losses[k] is keep[k] for k in keep)          # the input dict is not mutated
    assert table.tolist() == [1.0, 2.0, 3.0]                                               # nor the table its entries view
