"""GPU: the differentiable mask-logit product (kernels.mask_logits: einsum("bqc,bchw->bqhw") written pixel-major) -- the forward's
bits and both gradients against float64 einsum autograd. Bound, the project's convention: max-abs error <= 4 x the error of the
float32 torch evaluation against float64, measured here."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Q,ldq", [(37, 40), (100, 100)])
def test_mask_logits_forward_bits_and_gradients(Q, ldq, gemm_route):
    from multishiftseg_amd import kernels as K
    B, C, h, w = 2, 256, 8, 12
    g = torch.Generator(device="cuda").manual_seed(300 + Q)
    me = torch.randn((B, Q, C), device="cuda", generator=g)
    feat = torch.randn((B, C, h, w), device="cuda", generator=g)
    cot = torch.randn((B, h, w, ldq), device="cuda", generator=g)           # padded columns Q .. ldq-1 hold plain noise here
    act = K.nchw_to_act(feat)
    want_fwd = K.m2f_mask_logits_act(me, act, ldq)

    def run(cotangent):
        m = me.clone().requires_grad_(True)
        buf = act.buf.clone().requires_grad_(True)
        out = K.mask_logits(m, K.Act(buf, C=C), ldq)
        out.backward(cotangent)
        return out.detach(), m.grad, buf.grad
    out, dme, dfeat = run(cot)
    assert torch.equal(out, want_fwd)
    if ldq > Q:                                                              # garbage in the padded columns changes nothing
        dirty = cot.clone()
        dirty[..., Q:] = float("nan")
        _, dme2, dfeat2 = run(dirty)
        dirty[..., Q:] = 1e30
        _, dme3, dfeat3 = run(dirty)
        assert torch.equal(dme, dme2) and torch.equal(dfeat, dfeat2) and torch.equal(dme, dme3) and torch.equal(dfeat, dfeat3)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        m = me.to(dtype).requires_grad_(True)
        f = feat.to(dtype).requires_grad_(True)
        torch.einsum("bqc,bchw->bqhw", m, f).backward(cot[..., :Q].permute(0, 3, 1, 2).to(dtype))
        refs[dtype] = (m.grad, f.grad.permute(0, 2, 3, 1))
    for name, got, w64, w32 in zip(("d mask_embed", "d feat"), (dme, dfeat), refs[torch.float64], refs[torch.float32]):
        e32 = float((w32.double() - w64).abs().max())
        err = float((got.double() - w64).abs().max())
        print(f"Q {Q} ldq {ldq} {name}: kernel {err:.3g} torch-fp32 {e32:.3g}")
        assert torch.isfinite(got).all()
        assert err <= 4.0 * e32, (name, err, e32)
