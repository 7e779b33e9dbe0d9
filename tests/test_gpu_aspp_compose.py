"""The composed ASPP route as a whole (deepv3.DeepWV3Plus._aspp_composed: mod7's two 2048 -> 4096 output convolutions folded into the
ASPP weights) against the present path (MSS_ASPP_COMPOSE=0), at 2 x 3 x 592 x 600: the smallest fixture size at which the tile policy
gives F(4x4) on all three ASPP rates, so that the route is taken. Inputs, Dropout2d masks and loss permutations are those of the
reference-generated stage-2 fixture; the bars between the two routes are the ones test_three_routes_agree_at_bench_size holds."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

LOSS_PARAMS = {"ce_weights": [50, 10], "conduct_pixel_selection": True, "selection_ratio": 0.8,
               "inoutaug_contras_margins_tri": [10, 5, 5]}
FIXTURE = "deepwv3plus_train_step_2x592x600"


def _new_model(deeplab_params, state=None):
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    m = DeepWV3Plus(19)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
    m = m.cuda()
    m.uncertainty_func_init()
    if state is not None:
        m.load_state_dict(state)
    return m


@pytest.fixture(scope="module")
def inputs():
    from multishiftseg_amd import kernels as K, synth
    g = golden(FIXTURE)
    pairs, h, w = (int(v) for v in g["shape"])
    assert (pairs, h, w) == (1, 592, 600)
    assert [K.wino_tile(-(-h // 8), -(-w // 8), r) for r in (12, 24, 36)] == [4, 4, 4]
    return dict(img=torch.from_numpy(synth.synth_image(int(g["image_seed"]), 2 * pairs, h, w)).cuda(),
                target=torch.from_numpy(g["target"].astype(np.int64)).cuda(),
                masks={"mod6": torch.from_numpy(g["stage2_drop_mod6"]), "mod7": torch.from_numpy(g["stage2_drop_mod7"])},
                perms=[torch.from_numpy(g[f"stage2_perm{i}"].astype(np.int64)) for i in range(3)],
                sens={k[len("stage2_gradsens_"):]: float(g[k]) for k in g.files if k.startswith("stage2_gradsens_")})


def _train_steps(m, inputs, stage, steps):
    """`steps` TrainStep calls -> per call (score, logit, loss, {name: grad}, profile rows)."""
    from multishiftseg_amd import kernels as K
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import TrainStep
    step = TrainStep(m, RelContrastiveLoss(LOSS_PARAMS), stage=stage)
    step.keep_outputs = True
    m.dropout_masks = inputs["masks"]
    out = []
    for _ in range(steps):
        prof = K.ConvProfile()
        K.set_conv_profile(prof)
        try:
            loss = step(inputs["img"], inputs["target"].clone(), perms=inputs["perms"])
            rows = prof.per_launch()
        finally:
            K.set_conv_profile(None)
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
        out.append(step.last_outputs + (float(loss), grads, rows))
    return out


def _composes(rows, what=None):
    return [r for r in rows if r[0] == "aspp_compose" and (what is None or r[1][0] == what)]


def _trunk_output_products(rows):
    """The launches of a 2048 -> 4096 product over every pixel of the 74 x 75 map (mod7's proj_conv / conv3)."""
    return [r for r in rows if r[1] is not None and len(r[1]) == 8 and tuple(r[1][1:3]) == (74, 75) and r[1][4] == 4096]


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_composed_route_agrees_with_the_present_path(deeplab_params, inputs, monkeypatch):
    out, stats = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MSS_ASPP_COMPOSE", mode)
        m = _new_model(deeplab_params)
        out[mode] = _train_steps(m, inputs, 2, 1)[0]
        stats[mode] = {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k}
        del m
    # the route is really taken: one compose and one projection, and neither 2048 -> 4096 product over the map
    rows1, rows0 = out["1"][4], out["0"][4]
    assert len(_composes(rows1, "compose")) == 1 and len(_composes(rows1, "project")) == 1, _composes(rows1)
    assert not _composes(rows0)
    assert not _trunk_output_products(rows1) and len(_trunk_output_products(rows0)) >= 2
    assert sum(1 for r in rows1 if r[0] == "wino_transform" and r[1][0] == "input_aspp3") == 1
    (s1, l1, loss1, g1, _), (s0, l0, loss0, g0, _) = out["1"], out["0"]
    e_s, e_l = float((s1 - s0).abs().max()), float((l1 - l0).abs().max())
    print(f"composed vs present: max|dscore| {e_s:.3e} max|dlogit| {e_l:.3e} loss {loss1:.8g} / {loss0:.8g}")
    assert e_s < 5e-4 and e_l < 5e-4, (e_s, e_l)
    assert abs(loss1 / loss0 - 1) < 1e-4, (loss1, loss0)
    assert set(g1) == set(g0) and len(g1) == 18
    bad = []
    for k in g1:
        rel = _rel_l2(g1[k], g0[k])
        # aspp.img_conv at two images: BatchNorm over 2 samples is sign(x0 - x1), its input gradient O(eps) rounding noise in any
        # implementation -- the allowance test_three_routes_agree_at_bench_size makes
        bound = 0.5 if k.startswith("aspp.img_conv") else max(6e-3, 3 * inputs["sens"].get(k, 0.0))
        print(f"  grad {k}: rel-L2 {rel:.3e} (bound {bound:.3e})")
        if not rel <= bound:
            bad.append((k, rel, bound))
    assert not bad, bad
    assert set(stats["1"]) == set(stats["0"]) and stats["1"]
    for k, v in stats["1"].items():
        scale = float(stats["0"][k].abs().max())
        err = float((v - stats["0"][k]).abs().max())
        assert err <= 1e-6 * scale, (k, err, scale)


def test_composed_weights_follow_the_parameter_version(deeplab_params, inputs):
    """Two consecutive optimizer steps on one model == one step of a fresh model loaded with the once-updated weights: the cache of
    composed weights is keyed on the ASPP parameters' (version, data_ptr), so the second step composes again."""
    m = _new_model(deeplab_params)
    first = _train_steps(m, inputs, 2, 1)[0]
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    second = _train_steps(m, inputs, 2, 1)[0]
    assert len(_composes(first[4], "compose")) == 1 and len(_composes(second[4], "compose")) == 1
    assert not torch.equal(first[1], second[1])                          # the step moved the weights
    fresh = _train_steps(_new_model(deeplab_params, state), inputs, 2, 1)[0]
    assert torch.equal(second[0], fresh[0]) and torch.equal(second[1], fresh[1]) and second[2] == fresh[2]
    for k in second[3]:
        assert torch.equal(second[3][k], fresh[3][k]), k


def test_frozen_aspp_composes_once(deeplab_params, inputs):
    """Eval and stage 1 (only ood_head trains): the composed weights are made by the first forward and by no later one."""
    from multishiftseg_amd import kernels as K
    m = _new_model(deeplab_params).eval()
    counts = []
    for _ in range(2):
        prof = K.ConvProfile()
        K.set_conv_profile(prof)
        try:
            with torch.no_grad():
                m(inputs["img"][:1])
            counts.append(len(_composes(prof.per_launch())))
        finally:
            K.set_conv_profile(None)
    assert counts == [1, 0], counts
    m2 = _new_model(deeplab_params)
    steps = _train_steps(m2, inputs, 1, 3)
    assert [len(_composes(s[4])) for s in steps] == [1, 0, 0]
    assert all(not _trunk_output_products(s[4]) for s in steps)
