"""Test helper: the masked attention of the GMA transformer decoder in stock torch (the formula of attention_reference in
test_gpu_transformer_decoder.py, without the in-place writes, so that torch autograd can differentiate it), and the packing of
bool masks into the attention kernel's words."""
import torch


def pack(mask):
    """bool [..., Q] -> int32 words [..., ceil(Q/32)]."""
    Q = mask.shape[-1]
    W = (Q + 31) // 32
    m = torch.zeros(mask.shape[:-1] + (W * 32,), dtype=torch.int64, device=mask.device)
    m[..., :Q] = mask
    words = (m.view(mask.shape[:-1] + (W, 32)) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def attention(q, k, v, mask, B, Q, NK, A):
    """softmax(q k^T / sqrt(32) + mask) v per (image, attention, head) in the dtype of q; q [B*Q, A*256], k / v [B*NK, A*256],
    mask bool [B, A, Q, NK] (True = not allowed) or None."""
    outs = []
    for a in range(A):
        sl = slice(a * 256, (a + 1) * 256)
        qq = q[:, sl].view(B, Q, 8, 32).transpose(1, 2)
        kk = k[:, sl].view(B, NK, 8, 32).transpose(1, 2)
        vv = v[:, sl].view(B, NK, 8, 32).transpose(1, 2)
        s = torch.matmul(qq * (32 ** -0.5), kk.transpose(2, 3))
        if mask is not None:
            s = s.masked_fill(mask[:, a].unsqueeze(1), float("-inf"))
        outs.append(torch.matmul(torch.softmax(s, -1), vv).transpose(1, 2).reshape(B * Q, 256))
    return torch.cat(outs, 1)


def attention_grads(q, k, v, mask, cot, B, Q, NK, A, dtype):
    """(out, dq, dk, dv) of `attention` by torch autograd in `dtype` for the cotangent `cot`."""
    q, k, v = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out = attention(q, k, v, mask, B, Q, NK, A)
    out.backward(cot.to(dtype))
    return out.detach(), q.grad, k.grad, v.grad
