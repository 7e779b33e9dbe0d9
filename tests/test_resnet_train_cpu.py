"""CPU: the bookkeeping of the trainable backbone -- set_trainable / freeze, the parameter groups of a MaskFormer, what the
differentiable path refuses -- and the norm-gradient identity the backward rests on, on stock torch in float64. No kernels run."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import ref_resnet as R

STAGES = ("res2", "res3", "res4", "res5")


def _backbone():
    from multishiftseg_amd import build_resnet_backbone
    return build_resnet_backbone().eval()


def _is_norm(name):
    return ".norm." in name


def test_set_trainable_returns_self_and_is_off_by_default():
    m = _backbone()
    assert m._trainable is False
    assert m.set_trainable() is m and m._trainable is True
    assert m.set_trainable(False) is m and m._trainable is False


@pytest.mark.parametrize("freeze_at", [0, 1, 2, 3, 5, 6])
def test_freeze_has_detectron2s_meaning(freeze_at):
    """The stem for freeze_at >= 1, then res2 ... by index; convolution weights AND norm parameters of the frozen parts."""
    m = _backbone()
    assert m.freeze(freeze_at) is m
    frozen = (("stem",) + STAGES)[:freeze_at]
    for n, p in m.named_parameters():
        assert p.requires_grad == (n.split(".")[0] not in frozen), n
    assert all(p.requires_grad for p in m.parameters()) == (freeze_at == 0)
    if freeze_at >= 5:
        assert not any(p.requires_grad for p in m.parameters())


def test_the_faithful_stage2_pattern():
    """freeze(1, norms=True): every norm parameter and the stem frozen, the 52 res2..res5 convolution weights trainable."""
    m = _backbone().freeze(1, norms=True)
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert len(trainable) == 52 and all(n.endswith(".weight") and not _is_norm(n) and not n.startswith("stem.") for n in trainable)
    assert sum(1 for n, p in m.named_parameters() if _is_norm(n)) == 2 * 53
    assert "FREEZE_AT" in type(m).freeze.__doc__ and "FrozenBatchNorm2d" in type(m).freeze.__doc__


def test_refusal_messages_name_the_thing():
    m = _backbone().set_trainable()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="trainable stem.*stem.conv1.weight"):
        m(x)                                               # everything trainable: the stem is the first thing in the way
    m.freeze(1)
    m.stem.conv1.norm.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="trainable stem.*stem.conv1.norm.bias"):
        m(x)
    m.freeze(1)
    with pytest.raises(NotImplementedError, match="gradient for the image"):
        m(x.clone().requires_grad_(True))
    m.train()
    with pytest.raises(NotImplementedError, match="train-mode"):
        m(x)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x)                                               # past every refusal: the differentiable path would run, on a GPU
    m.freeze(5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x)                                               # nothing asks for a gradient: the frozen path
    m.set_trainable(False)
    m.res5[2].conv3.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="no backward"):
        m(x)                                               # without the switch, as before


def test_maskformer_switch_and_param_groups():
    """set_trainable switches the backbone and the predictor; build_m2f_param_groups gives the backbone's tensors 0.1 x lr, norm
    parameters weight_decay_norm, everything else the base values; frozen tensors are in no group."""
    from multishiftseg_amd import MaskFormer, build_m2f_param_groups

    class _Predictor(nn.Linear):
        def set_trainable(self, flag=True):
            self.flag = flag
            return self

    predictor = _Predictor(3, 3)
    shell = MaskFormer(_backbone(), nn.Sequential(nn.Linear(2, 2), nn.LayerNorm(2)), predictor)
    assert shell._trainable is False
    assert shell.set_trainable() is shell and shell.backbone._trainable and predictor.flag is True and shell._trainable
    shell.set_trainable(False)
    assert not shell.backbone._trainable and predictor.flag is False and not shell._trainable

    shell.backbone.freeze(1)                               # res2..res5 with their norms trainable
    groups = build_m2f_param_groups(shell, 1e-4, 0.05, weight_decay_norm=0.0)
    by_id = {id(g["params"][0]): g for g in groups}
    assert len(by_id) == len(groups) == 52 * 3 + 4 + 2
    for n, p in shell.named_parameters():
        if n.startswith("backbone.stem."):
            assert id(p) not in by_id, n
            continue
        g = by_id[id(p)]
        assert g["lr"] == pytest.approx(1e-5 if n.startswith("backbone.") else 1e-4), n
        norm = _is_norm(n) or n.startswith("sem_seg_head.pixel_decoder.1.")
        assert g["weight_decay"] == (0.0 if norm else 0.05), n
    shell.backbone.freeze(1, norms=True)
    faithful = build_m2f_param_groups(shell, 1e-4, 0.05)
    assert sum(1 for g in faithful if g["lr"] == pytest.approx(1e-5)) == 52
    assert all(g["weight_decay"] == 0.05 for g in faithful if g["lr"] == pytest.approx(1e-5))


@pytest.mark.parametrize("stride,k,pad", [(1, 1, 0), (2, 3, 1), (2, 1, 0)])
def test_norm_gradient_identity(stride, k, pad):
    """y = norm(conv(x, W)) with running statistics: for G = d<dz, conv(x, W)>/dW (the plain weight gradient at dz),
    dW = s * G, dbeta = sum dz, dgamma = rstd * (<W, G> - running_mean * dbeta) with s = gamma * rstd -- autograd's, in float64.
    The pre-norm output is linear in W, so <W_k, G_k> = sum_pixels dz_k * conv(x, W)_k: nothing is stored or divided by gamma."""
    g = torch.Generator().manual_seed(11 * k + stride)
    x = torch.randn((2, 6, 9, 13), generator=g, dtype=torch.float64)
    w = torch.randn((8, 6, k, k), generator=g, dtype=torch.float64).requires_grad_(True)
    gamma = (torch.rand(8, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(8, generator=g, dtype=torch.float64).requires_grad_(True)
    mean, var = torch.randn(8, generator=g, dtype=torch.float64), torch.rand(8, generator=g, dtype=torch.float64) + 0.5
    y = F.batch_norm(F.conv2d(x, w, None, stride, pad), mean, var, gamma, beta, training=False, eps=R.EPS)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dw, dgamma, dbeta = torch.autograd.grad((y * dz).sum(), [w, gamma, beta])
    wd = w.detach().clone().requires_grad_(True)
    G, = torch.autograd.grad((F.conv2d(x, wd, None, stride, pad) * dz).sum(), [wd])
    rstd = (var + R.EPS).rsqrt()
    s = gamma.detach() * rstd
    db = dz.sum((0, 2, 3))
    torch.testing.assert_close(s.view(-1, 1, 1, 1) * G, dw, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, dbeta, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rstd * ((w.detach() * G).sum((1, 2, 3)) - mean * db), dgamma, rtol=1e-11, atol=1e-11)


def test_what_is_new_is_exported():
    import multishiftseg_amd as pkg
    from multishiftseg_amd import _lib, kernels
    assert "conv2d_dgrad_s2" in pkg.__all__ and pkg.conv2d_dgrad_s2 is kernels.conv2d_dgrad_s2
    assert callable(pkg.ResNet.set_trainable) and callable(pkg.ResNet.freeze) and callable(pkg.MaskFormer.set_trainable)
    assert _lib.MSS_ABI_VERSION == 26
