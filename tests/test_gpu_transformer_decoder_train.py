"""GPU: the opt-in trainable path of the GMA transformer decoder (transformer_decoder.set_trainable): gradients of every parameter, of
the feature levels and of the mask features against torch autograd through the stock-torch helper (tests/ref_transformer_decoder.py)
under the module's own mask bits, in float64 and in float32.

Bound, per tensor: relative L2 error against float64 <= 4 x the float32 helper's relative L2 error against float64, measured here."""
import pytest
import torch

import ref_transformer_decoder as R

pytestmark = pytest.mark.gpu

B, SIZES, FSIZE, Q, LAYERS, SEED = 2, [(4, 6), (8, 12), (16, 24)], (32, 48), 37, 3, 41
GEOM = dict(num_classes=19, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=128, dec_layers=LAYERS, pre_norm=False, mask_dim=256)
SD_GEOM = dict(num_layers=LAYERS, num_queries=Q, dim_feedforward=128)


def unpack(bits, n):
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(-1) >> sh) & 1).flatten(-2)[..., :n].bool()


def build_module(project):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, enforce_input_project=project, **GEOM)
    m.load_state_dict(R.synth_state_dict(SEED, enforce_input_project=project, **SD_GEOM), strict=True)
    return m.cuda().eval()


def steps_of(out):
    """The distinct returned tensors of every step: (class logits of steps 0 .. L, OOD class logits of steps 1 .. L, masks of steps
    0 .. L); every pred_masks_ood is one of those masks."""
    aux = out["aux_outputs"]
    return ([a["pred_logits"] for a in aux] + [out["pred_logits"]], [a["pred_logits_ood"] for a in aux] + [out["pred_logits_ood"]],
            [a["pred_masks"] for a in aux] + [out["pred_masks"]])


def cotangents(out):
    g = torch.Generator().manual_seed(77)
    return [[torch.randn(t.shape, generator=g, dtype=torch.float64) * scale for t in group] for group, scale in zip(steps_of(out), (1.0, 1.0, 0.05))]


def pull(out, cots):
    loss = 0
    for group, cg in zip(steps_of(out), cots):
        for t, c in zip(group, cg):
            loss = loss + (t * c.to(device=t.device, dtype=t.dtype)).sum()
    loss.backward()


def helper_run(dtype, project, x, feat, forced, cots):
    sd = R.synth_state_dict(SEED, dtype=dtype, enforce_input_project=project, **SD_GEOM)
    for t in sd.values():
        t.requires_grad_(True)
    xs = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in x]
    ft = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    out = R.decoder_forward(sd, xs, ft, LAYERS, forced_bits=forced)
    pull(out, cots)
    grads = {k: t.grad for k, t in sd.items()}
    for i, t in enumerate(xs):
        grads[f"x[{i}]"] = t.grad
    grads["mask_features"] = ft.grad
    return out, grads


@pytest.mark.parametrize("project", [True, False])
def test_trainable_decoder_gradients(project):
    x, feat = R.synth_inputs(411, B, SIZES, FSIZE)
    m = build_module(project).set_trainable()

    def module_run():
        m.zero_grad(set_to_none=True)
        xs = [torch.from_numpy(v).cuda().requires_grad_(True) for v in x]
        ft = torch.from_numpy(feat).cuda().requires_grad_(True)
        out = m(xs, ft, return_attn_bits=True)
        return out, xs, ft
    out, xs, ft = module_run()
    assert out["pred_masks_ood"] is out["pred_masks"] and len(out["aux_outputs"]) == LAYERS - 1
    cots = cotangents(out)
    pull(out, cots)
    got = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    for i, t in enumerate(xs):
        got[f"x[{i}]"] = t.grad.clone()
    got["mask_features"] = ft.grad.clone()
    # a second pass: the same bits
    out_b, xs_b, ft_b = module_run()
    pull(out_b, cots)
    for k, p in m.named_parameters():
        assert (p.grad is None) == (got[k] is None) and (p.grad is None or torch.equal(p.grad, got[k])), k
    assert all(torch.equal(a.grad, got[f"x[{i}]"]) for i, a in enumerate(xs_b)) and torch.equal(ft_b.grad, got["mask_features"])

    forced = []
    for words in out["attn_bits"]:
        mk = unpack(words, Q).transpose(2, 3).cpu()
        forced.append((mk[:, 0].contiguous(), mk[:, 1].contiguous()))
    o64, g64 = helper_run(torch.float64, project, x, feat, forced, cots)
    o32, g32 = helper_run(torch.float32, project, x, feat, forced, cots)

    # forward: the trainable path against the frozen path of the same module, within 4 x the helper's own float32 distance
    with torch.no_grad():
        frozen = m(xs, ft, return_attn_bits=True)
    for a, b in zip(out["attn_bits"], frozen["attn_bits"]):
        assert torch.equal(a, b)
    for kind, tr, fr, h32, h64 in zip(("logits", "logits_ood", "masks"), steps_of(out), steps_of(frozen), steps_of(o32), steps_of(o64)):
        noise = max(float((p.double() - q).abs().max()) for p, q in zip(h32, h64))
        err = max(float((p.detach() - q).abs().max()) for p, q in zip(tr, fr))
        far = max(float((p.detach().double().cpu() - q.detach()).abs().max()) for p, q in zip(tr, h64))
        rms = max(float(q.detach().pow(2).mean().sqrt()) for q in h64)
        print(f"forward {kind}: trainable vs frozen {err:.3g}, vs float64 {far:.3g}, helper float32 noise {noise:.3g}")
        assert err <= 4.0 * noise, (kind, err, noise)
        assert far <= max(1e-5 * rms, 4.0 * noise), (kind, far, noise)        # the forward protocol of test_gpu_transformer_decoder.py

    worst = []
    for name, w64 in g64.items():
        if "fusion_layer" in name:
            assert got[name] is None and w64 is None, name
            continue
        assert got[name] is not None, f"{name} received no gradient"
        nrm = float(w64.norm())
        e32 = float((g32[name].double() - w64).norm()) / nrm
        err = float((got[name].double().cpu() - w64).norm()) / nrm
        print(f"{name}: rel L2 {err:.3g} float32 helper {e32:.3g}")
        assert torch.isfinite(got[name]).all(), name
        if err > 4.0 * e32:
            worst.append((name, err, e32))
    assert not worst, worst


def test_switch_off_keeps_the_forward_only_behaviour():
    x, feat = R.synth_inputs(411, B, SIZES, FSIZE)
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    plain, toggled = build_module(True), build_module(True)
    toggled.set_trainable(True)
    toggled.set_trainable(False)
    with pytest.raises(NotImplementedError):
        toggled(xs, ft)                                                # every parameter trainable, switch off: still not a supported mode
    with torch.no_grad():                                              # under no_grad the switch makes no difference
        a = plain(xs, ft)
        b = toggled.set_trainable(True)(xs, ft)
        toggled.set_trainable(False)
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_masks"], b["pred_masks"])
    grads = []
    cot = torch.randn(a["pred_logits_ood"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for m in (plain, toggled):                                         # stage 1: only class_embed2 trainable
        for p in m.parameters():
            p.requires_grad_(False)
        m.class_embed2.weight.requires_grad_(True)
        m.class_embed2.bias.requires_grad_(True)
        out = m(xs, ft)
        assert not out["pred_logits"].requires_grad and not out["pred_masks"].requires_grad
        (out["pred_logits_ood"] * cot).sum().backward()
        grads.append((m.class_embed2.weight.grad, m.class_embed2.bias.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
