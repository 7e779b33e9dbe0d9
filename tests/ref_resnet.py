"""Stock-torch restatement of the ResNet-50 backbone the Mask2Former config loads (detectron2 build_resnet_backbone: depth 50,
STRIDE_IN_1X1 False, eval-mode norms), on a plain state dict in any float dtype. The yardstick of tests/test_gpu_stem7.py,
tests/test_gpu_resnet.py and tools/bench_m2f_backbone.py; nothing here imports the package."""
import torch
import torch.nn.functional as F

STAGES = (("res2", 3, 1), ("res3", 4, 2), ("res4", 6, 2), ("res5", 3, 2))      # name, blocks, stride of the first block
EPS = 1e-5


def cast(sd, dtype, device=None):
    return {k: v.to(dtype=dtype, device=device) for k, v in sd.items() if v.is_floating_point()}


def conv_norm(x, sd, name, stride=1, padding=0):
    """norm(conv(x)) of the layer `name` (weight without bias, then its `.norm` with running statistics)."""
    y = F.conv2d(x, sd[name + ".weight"], None, stride=stride, padding=padding)
    n = name + ".norm."
    return F.batch_norm(y, sd[n + "running_mean"], sd[n + "running_var"], sd[n + "weight"], sd[n + "bias"], training=False, eps=EPS)


def stem_conv(x, sd):
    """The stem before its max-pool: relu(norm(conv7x7 stride 2 padding 3))."""
    return F.relu(conv_norm(x, sd, "stem.conv1", stride=2, padding=3))


def block(x, sd, prefix, stride):
    """relu(norm3(conv3(relu(norm2(conv2(relu(norm1(conv1(x)))))))) + shortcut(x)); the 3x3 layer carries the stride."""
    sc = conv_norm(x, sd, prefix + ".shortcut", stride=stride) if prefix + ".shortcut.weight" in sd else x
    y = F.relu(conv_norm(x, sd, prefix + ".conv1"))
    y = F.relu(conv_norm(y, sd, prefix + ".conv2", stride=stride, padding=1))
    return F.relu(conv_norm(y, sd, prefix + ".conv3") + sc)


def resnet50(x, sd):
    """x [N,3,H,W] -> {"res2": ..., "res5": ...}; x and sd share dtype and device."""
    y = F.max_pool2d(stem_conv(x, sd), kernel_size=3, stride=2, padding=1)
    out = {}
    for name, nblocks, stride in STAGES:
        for i in range(nblocks):
            y = block(y, sd, f"{name}.{i}", stride if i == 0 else 1)
        out[name] = y
    return out


def randomize_(module, seed, conv3_scale=0.25):
    """kaiming_normal_ convolutions; norm weight in [0.5, 1.5], bias and running mean in [-0.2, 0.2], running variance in [0.5, 1.5];
    every conv3.norm.weight scaled by conv3_scale so that the residual trunk does not grow over 16 blocks."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if t.dim() == 4:
                fan_out = t.shape[0] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / fan_out) ** 0.5)          # kaiming_normal_(fan_out, relu)
            elif name.endswith("running_mean") or name.endswith("norm.bias"):
                t.copy_(torch.rand(t.shape, generator=g) * 0.4 - 0.2)
            else:                                                                          # norm.weight, running_var
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
                if name.endswith("conv3.norm.weight"):
                    t.mul_(conv3_scale)
    return module


def rel_max_err(a, ref):
    """max|a - ref| / max|ref| in float64."""
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())
