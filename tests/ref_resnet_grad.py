"""tests/ref_resnet.py under stock-torch autograd: the gradients of sum_maps <map, g_map> with respect to the block / backbone
parameters (and the block's input), in any float dtype on the CPU, together with the `> 0` pattern of the pre-activation of EVERY
ReLU. The yardstick of tests/test_gpu_resnet_backward.py, tests/test_gpu_maskformer_train.py and tools/bench_m2f_backbone.py;
nothing here imports the package.

The sign patterns are a condition of the comparison, not a tolerance: a ReLU whose pre-activation changes sign between two
precisions changes a gradient by a finite amount, so a test first asserts that the patterns agree and then compares every element."""
import torch
import torch.nn.functional as F

import ref_resnet as R


def _relu(t, gates):
    gates.append(t.detach() > 0)
    return F.relu(t)


def block(x, sd, prefix, stride, gates):
    """ref_resnet.block with the three ReLUs' patterns appended to `gates` (conv1, conv2, output)."""
    sc = R.conv_norm(x, sd, prefix + ".shortcut", stride=stride) if prefix + ".shortcut.weight" in sd else x
    y = _relu(R.conv_norm(x, sd, prefix + ".conv1"), gates)
    y = _relu(R.conv_norm(y, sd, prefix + ".conv2", stride=stride, padding=1), gates)
    return _relu(R.conv_norm(y, sd, prefix + ".conv3") + sc, gates)


def resnet50(x, sd, gates):
    y = F.max_pool2d(_relu(R.conv_norm(x, sd, "stem.conv1", stride=2, padding=3), gates), kernel_size=3, stride=2, padding=1)
    out = {}
    for name, nblocks, stride in R.STAGES:
        for i in range(nblocks):
            y = block(y, sd, f"{name}.{i}", stride if i == 0 else 1, gates)
        out[name] = y
    return out


def leaves(sd, dtype):
    """The state dict in `dtype` with every convolution weight and norm weight / bias a leaf that requires a gradient."""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            continue
        t = v.detach().cpu().to(dtype).clone()
        out[k] = t.requires_grad_(True) if k.endswith((".weight", ".bias")) else t
    return out


def block_grads(x, sd, prefix, stride, g_out, dtype):
    """(out, {"x": dx, <key>: grad}, gates) of one block at output gradient g_out."""
    p, gates = leaves(sd, dtype), []
    xin = x.to(dtype).clone().requires_grad_(True)
    out = block(xin, p, prefix, stride, gates)
    (out * g_out.to(dtype)).sum().backward()
    grads = {k: t.grad for k, t in p.items() if t.requires_grad and t.grad is not None}
    grads["x"] = xin.grad
    return out.detach(), grads, gates


def resnet50_grads(img, sd, g_maps, dtype):
    """(maps, {<key>: grad}, gates) of the backbone at output gradients g_maps {name: tensor}; no gradient for the image."""
    p, gates = leaves(sd, dtype), []
    out = resnet50(img.to(dtype), p, gates)
    sum((out[n] * g.to(dtype)).sum() for n, g in g_maps.items()).backward()
    return {n: t.detach() for n, t in out.items()}, {k: t.grad for k, t in p.items() if t.requires_grad and t.grad is not None}, gates


def same_gates(a, b):
    """The number of ReLU inputs whose `> 0` pattern differs between two runs."""
    assert len(a) == len(b)
    return sum(int((x != y).sum()) for x, y in zip(a, b))
