"""GPU: the masked attention's training forward and backward alone (csrc/m2f_attn.hip: mss_m2f_masked_attention_lse_f32,
mss_m2f_masked_attention_bwd_f32; kernels.m2f_masked_attention_lse / m2f_masked_attention_backward / masked_attention).

Reference: tests/ref_attention.py (the formula of attention_reference in test_gpu_transformer_decoder.py) differentiated by torch
autograd in float64 and in float32 on the same inputs. Bound for each of dq, dk, dv: max-abs error against float64 <= 4 x the
error of the float32 torch evaluation against float64, measured in the same test."""
import pytest
import torch

import ref_attention as RA

pytestmark = pytest.mark.gpu

# (B, Q, NK, A, chunks): NK below a key tile and not a multiple of 8 | one wave, partial mask word | ragged last chunk | all 128
# queries, two words per wave | few queries | the second wave holds a single query | the second word holds one query, a second dK/dV
# workgroup with one key | the fourth word holds one query, three dK/dV workgroups, chunks of 56 keys | one full wave, one full
# dK/dV workgroup | one query, a second step of one key (plain mask: make_mask) | 64 chunks asked, 16 launched, the last dK/dV lane idle
CASES = [(1, 100, 15, 2, 1), (2, 37, 100, 1, 1), (1, 100, 100, 1, 4), (1, 128, 200, 2, 3), (2, 5, 70, 2, 2), (1, 65, 193, 1, None),
         (1, 33, 129, 1, 2), (1, 97, 257, 2, 5), (2, 64, 128, 1, 1), (1, 1, 9, 1, 1), (1, 128, 127, 1, 64)]
DEAD_KEY = 1        # masked for every query


def make_inputs(B, Q, NK, A, seed=0):
    g = torch.Generator(device="cuda").manual_seed(2000 + NK + Q + seed)
    q = torch.randn((B * Q, A * 256), device="cuda", generator=g)
    k = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    v = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    cot = torch.randn((B * Q, A * 256), device="cuda", generator=g)
    return q, k, v, cot, g


def make_mask(B, Q, NK, A, g, rescue):
    """-> (bits, allowed, effective bool mask [B, A, Q, NK]). Rows: random at 50 %; query 1 sees only the last 3 keys; query 2 fully
    masked and rescued through its `allowed` bit (rescue=True; else a random row like the others); query 3 has exactly one allowed
    key (key 0); key DEAD_KEY is masked for every query. Fewer than 4 queries: only the random rows, each with key 0 allowed, and
    the dead key (no rescued row)."""
    mask = torch.rand((B, A, Q, NK), device="cuda", generator=g) < 0.5
    if Q < 4:
        mask[..., 0] = False
        mask[..., DEAD_KEY] = True
        return RA.pack(mask.transpose(2, 3).contiguous()), RA.pack(torch.ones((B, A, Q), dtype=torch.bool, device="cuda")), mask
    mask[:, :, 1, :] = True
    mask[:, :, 1, max(0, NK - 3):] = False
    mask[:, :, 0, 0] = False                                         # every row keeps at least one key
    mask[:, :, 3:, 0] = False
    mask[:, :, 3, 1:] = True
    if rescue:
        mask[:, :, 2, :] = True
    else:
        mask[:, :, 2, 0] = False
    mask[:, :, :, DEAD_KEY] = True
    bits = RA.pack(mask.transpose(2, 3).contiguous())                # [B, A, NK, W]
    ok = torch.ones((B, A, Q), dtype=torch.bool, device="cuda")
    if rescue:
        ok[:, :, 2] = False
    allowed = RA.pack(ok)
    eff = mask.clone()
    if rescue:
        eff[:, :, 2, :] = False                                      # what the rescue rule makes of row 2
    return bits, allowed, eff


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,Q,NK,A,chunks", CASES)
def test_attention_backward_kernels(B, Q, NK, A, chunks, masked):
    """Forward bits, lse, the three gradients against float64 under the 4 x float32-torch bound, reproducibility (the third run on a
    NaN-filled workspace and NaN-prefilled outputs). The rescued query 2 ignores its mask and so attends to DEAD_KEY as well: the
    exact zeros of that key's dk / dv rows are asserted on a second mask set of the same kind whose row 2 is a plain row (no rescue)."""
    from multishiftseg_amd import _lib, kernels as K
    q, k, v, cot, g = make_inputs(B, Q, NK, A)
    bits = allowed = eff = None
    if masked:
        bits, allowed, eff = make_mask(B, Q, NK, A, g, rescue=True)
    n_chunks = chunks if chunks is not None else K.m2f_attn_chunks(B, A, NK)
    kw = dict(A=A, bits=bits, allowed=allowed, chunks=chunks)
    out_inf = K.m2f_masked_attention(q, k, v, B, Q, NK, **kw)
    out, lse = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, **kw)
    assert torch.equal(out, out_inf)
    assert tuple(lse.shape) == (B, A, 8, Q) and torch.isfinite(lse).all()
    g1 = K.m2f_masked_attention_backward(q, k, v, out, lse, cot, B, Q, NK, **kw)
    g2 = K.m2f_masked_attention_backward(q, k, v, out, lse, cot, B, Q, NK, **kw)
    nan = float("nan")
    ws = torch.full((_lib.value("mss_m2f_attn_bwd_workspace_bytes", B, Q, A, n_chunks) // 4,), nan, device="cuda")
    pre = tuple(torch.full_like(t, nan) for t in g1)
    g3 = K.m2f_masked_attention_backward(q, k, v, out, lse, cot, B, Q, NK, ws=ws, grads=pre, **kw)
    torch.cuda.synchronize()
    for a, b, c in zip(g1, g2, g3):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)
    r64 = RA.attention_grads(q, k, v, eff, cot, B, Q, NK, A, torch.float64)
    r32 = RA.attention_grads(q, k, v, eff, cot, B, Q, NK, A, torch.float32)
    # lse: log2 domain
    for a in range(A):
        s = torch.matmul(q[:, a * 256:(a + 1) * 256].double().view(B, Q, 8, 32).transpose(1, 2) * (32 ** -0.5),
                         k[:, a * 256:(a + 1) * 256].double().view(B, NK, 8, 32).transpose(1, 2).transpose(2, 3))
        if eff is not None:
            s = s.masked_fill(eff[:, a].unsqueeze(1), float("-inf"))
        want = torch.logsumexp(s, -1) * 1.4426950408889634
        assert float((lse[:, a].double() - want).abs().max()) <= 1e-4
    for name, got, w64, w32 in zip(("dq", "dk", "dv"), g1, r64[1:], r32[1:]):
        e32 = float((w32.double() - w64).abs().max())
        err = float((got.double() - w64).abs().max())
        print(f"B {B} Q {Q} NK {NK} A {A} chunks {n_chunks} masked {masked} {name}: kernel {err:.3g} torch-fp32 {e32:.3g}")
        assert err <= 4.0 * e32, (name, err, e32)
    if masked:
        # query 3 has one allowed key: P = 1, dS = 0, its dq row is 0 to rounding (|dout| |v| |k| ~ 32 x 2^-22 per element)
        if Q >= 4:
            dq = g1[0].view(B, Q, A * 256)
            assert float(dq[:, 3].abs().max()) <= 1e-4, float(dq[:, 3].abs().max())
        bits2, allowed2, _ = make_mask(B, Q, NK, A, g, rescue=False)
        kw2 = dict(A=A, bits=bits2, allowed=allowed2, chunks=chunks)
        out2, lse2 = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, **kw2)
        _, dk2, dv2 = K.m2f_masked_attention_backward(q, k, v, out2, lse2, cot, B, Q, NK, **kw2)
        assert torch.isfinite(dk2).all() and torch.isfinite(dv2).all()
        assert int((dk2.view(B, NK, -1)[:, DEAD_KEY] != 0).sum()) == 0 and int((dv2.view(B, NK, -1)[:, DEAD_KEY] != 0).sum()) == 0
        assert float(dk2.view(B, NK, -1)[:, 0].abs().max()) > 0


@pytest.mark.parametrize("B,Q,NK,chunks", [(2, 37, 100, 1), (1, 100, 100, 4)])
def test_autograd_op_on_column_slices(B, Q, NK, chunks):
    """multishiftseg_amd.masked_attention on q / k that are column slices of a [rows, 512] tensor (the self-attention's stacked
    projection) gives the bits of contiguous copies, forward and backward; the gradients arrive in the wide tensor's columns."""
    import multishiftseg_amd
    q, k, v, cot, g = make_inputs(B, Q, NK, 1, seed=7)
    wide_q = torch.randn((B * Q, 512), device="cuda", generator=g)
    wide_k = torch.randn((B * NK, 512), device="cuda", generator=g)
    wide_q[:, 256:] = q
    wide_k[:, :256] = k
    wide_q.requires_grad_(True)
    wide_k.requires_grad_(True)
    vv = v.clone().requires_grad_(True)
    out = multishiftseg_amd.masked_attention(wide_q[:, 256:], wide_k[:, :256], vv, B, Q, NK, chunks=chunks)
    out.backward(cot)
    qc, kc, vc = (t.clone().requires_grad_(True) for t in (q, k, v))
    out_c = multishiftseg_amd.masked_attention(qc, kc, vc, B, Q, NK, chunks=chunks)
    out_c.backward(cot)
    assert torch.equal(out, out_c)
    assert torch.equal(wide_q.grad[:, 256:], qc.grad) and int((wide_q.grad[:, :256] != 0).sum()) == 0
    assert torch.equal(wide_k.grad[:, :256], kc.grad) and int((wide_k.grad[:, 256:] != 0).sum()) == 0
    assert torch.equal(vv.grad, vc.grad)


def test_needs_input_grad_subsets():
    import multishiftseg_amd
    B, Q, NK, A = 2, 37, 100, 2
    q, k, v, cot, g = make_inputs(B, Q, NK, A, seed=3)
    bits, allowed, _ = make_mask(B, Q, NK, A, g, rescue=True)
    full = [t.clone().requires_grad_(True) for t in (q, k, v)]
    multishiftseg_amd.masked_attention(*full, B, Q, NK, A=A, bits=bits, allowed=allowed).backward(cot)
    for which in ((2,), (0,)):                                       # only v, only q
        ins = [t.clone().requires_grad_(i in which) for i, t in enumerate((q, k, v))]
        multishiftseg_amd.masked_attention(*ins, B, Q, NK, A=A, bits=bits, allowed=allowed).backward(cot)
        for i, t in enumerate(ins):
            if i in which:
                assert torch.equal(t.grad, full[i].grad)
            else:
                assert t.grad is None
