"""GPU: the masked attention (csrc/m2f_attn.hip) on constructions whose expected result is exact in fp32, at every query-word,
key-step and chunk boundary. No tolerance enters the exact tests; why equality is owed:

1. Argmax attention (tests/ref_attention.py argmax_case). Per head q_i = +-G e_d(i) with G = 1024, and component d of the keys is a
   permutation of NK distinct integers. q is 0 in the other components, so the kernel's 32-term fma chain adds exact zeros to ONE
   product, rounded once: score(i, j) = fl(fl(+-G * scale * log2 e) * k_j[d(i)]). One integer step of k is G * scale * log2(e) ~ 261
   units of that log2-domain score (products stay below 2^16, their rounding below 2^-8), so relative to the best allowed key every
   other key sits at <= -160 and exp2f gives exactly 0 (2^-160 is below half the smallest denormal); the best has exp2f(0) = 1.
   Hence l = 1, 1 / l = 1, log2f(1) = 0, a rescale by alpha = exp2f(<= -160) = 0 wipes what was accumulated, and
     out[i] = v[win(i)] (win: the best allowed key -- argmax for +G, argmin for -G), lse[i] = score(i, win(i)), finite, equal on
     the direct and the chunked route (a chunk whose keys all lose, or which has no allowed key, enters the merge with weight
     exp2f(<= -160) = 0, resp. the literal 0 of a chunk with maximum -inf; the winner's chunk has weight exp2f(0) = 1, den = 1);
     dv[j] = the sum of dout[i] over the queries j wins (dout: small integers, P = exp2f(score - lse) = 1 resp. 0), exact zeros in
     the dv rows of every other key; dq = dk = 0, because D = <dout, out> and <dout, v_win> are the same 32-term fma chain over
     the same values, so dS = 1 * (x - x) = 0 for the winner and 0 * (finite) for the rest.
   Keys ascending with their index move the running maximum of a +G query at every 8-key step, descending never; both run, and a
   shuffled order.
2. Uniform attention (uniform_case): scale = 0.0 makes every score 0 and every allowed key p = exp2f(0) = 1; with integer v and
   allowed sets of 1, 2, 4 ... 128 keys, out is an integer sum times the exact reciprocal of a power of two (direct route), resp. an
   integer numerator over an integer power-of-two denominator merged with weights exp2f(0) = 1 (chunked route): exact. dq and dk
   are products with scale = 0 resp. with q * 0: they compare equal to 0. dv is NOT exact by argument: P = exp2f(0 - lse) with
   lse = log2f(2^n), and neither log2f(2^n) = n nor exp2f(-n) = 2^-n is promised exact -- it is held to 4 ulp of the float64 value
   (dout >= 0 there, so the sum has no cancellation and an ulp of the value is the right unit).
3. Mask-bits kernel -> attention in one chain: logits on the 1/8 grid and dyadic size ratios make every bilinear blend exact
   (zeros are exact zeros), so the bit rows are the sign pattern of the float64 interpolation, and the argmax attention run on the
   KERNEL's bits must pick the winners computed on the CPU from that sign pattern.

The scale / peaked-score test is by tolerance, under a bound derived from the arithmetic (its docstring), never measured."""
import numpy as np
import pytest
import torch

import ref_attention as RA

pytestmark = pytest.mark.gpu

SEED = 17
S32 = 32 ** -0.5
NAN = float("nan")

# (B, Q, NK, A, chunks, key order, masked, the edge the case is there for)
ARGMAX_CASES = [
    (1, 1, 1, 1, 1, "asc", False, "the smallest launch: one query, one key"),
    (1, 1, 9, 1, 1, "asc", False, "Q = 1; NK = 8 + 1: a second step of one key"),
    (2, 1, 129, 2, 5, "shuffle", True, "Q = 1 with a rescued row; chunks of 32 keys, the last chunk one key"),
    (1, 32, 8, 1, 1, "desc", True, "exactly one mask word, exactly one 8-key step"),
    (1, 33, 7, 1, 1, "asc", True, "the second word holds one query; NK < 8"),
    (1, 33, 1, 1, 1, "asc", True, "NK = 1: every row sees key 0 or is rescued"),
    (2, 64, 1, 2, 64, "asc", False, "NK = 1, 64 chunks asked: the plan shrinks to one"),
    (1, 64, 9, 2, 1, "shuffle", True, "a full wave, both words; NK = 8 + 1"),
    (1, 65, 127, 1, 1, "asc", True, "the second wave holds one query (its second word is clamped); NK = 128 - 1"),
    (1, 65, 8, 1, 2, "shuffle", False, "2 chunks asked of 8 keys: one chunk"),
    (1, 65, 7, 2, 5, "shuffle", True, "5 chunks asked of 7 keys: one chunk, one ragged step"),
    (1, 96, 128, 1, 2, "shuffle", True, "three words: the second wave's second word is clamped; 2 x 64 keys"),
    (1, 96, 9, 1, 2, "desc", True, "2 chunks of 8 keys, the last one key"),
    (1, 96, 127, 2, 64, "shuffle", True, "16 chunks of 8 keys, the last 7; chunk 1 has no allowed key"),
    (1, 97, 129, 2, 2, "asc", True, "the fourth word holds one query; chunks of 72 and 57 keys"),
    (1, 97, 7, 1, 64, "desc", True, "64 chunks asked of 7 keys"),
    (2, 97, 8, 1, 5, "asc", True, "5 chunks asked of 8 keys; B = 2"),
    (1, 97, 257, 1, 64, "shuffle", True, "33 chunks of 8 keys (64 asked), the last one key"),
    (1, 97, 129, 1, 5, "asc", False, "no mask, chunked, the last chunk one key, the maximum moves at every step"),
    (1, 128, 257, 1, 5, "shuffle", True, "all four words; chunks of 56 keys, the last 33"),
    (2, 128, 129, 2, 5, "asc", True, "both words of the second wave, B = A = 2, the last chunk one key"),
    (1, 128, 9, 1, 64, "asc", True, "64 asked -> 2 chunks, the last one key"),
    (1, 128, 257, 2, 1, "asc", True, "direct, 33 steps, the running maximum moves at every one"),
    (1, 128, 257, 1, 1, "desc", False, "direct, the running maximum never moves after the first step"),
    (1, 128, 128, 1, 1, "shuffle", False, "no mask, 128 x 128, one dK/dV workgroup exactly"),
    (1, 128, 127, 2, 2, "desc", True, "NK = 127: the last dK/dV lane idle"),
    (1, 33, 127, 1, 5, "shuffle", True, "5 chunks asked, 4 launched (32 keys each, the last 31)"),
    (1, 33, 128, 1, 64, "desc", True, "16 full chunks of 8 keys"),
    (1, 64, 128, 1, 5, "asc", True, "5 chunks asked, 4 launched, all full"),
    (1, 64, 129, 1, 64, "asc", True, "17 chunks, the last one key; two dK/dV workgroups, the second with one key"),
    (2, 32, 129, 1, 2, "shuffle", True, "one word; chunks of 72 and 57 keys (57 = 7 steps + 1 key)"),
    (1, 32, 257, 2, 2, "asc", True, "chunks of 136 and 121 keys; three dK/dV workgroups, the third with one key"),
    (2, 65, 257, 1, 5, "desc", True, "B = 2 at 257 keys, second wave with one query"),
    (1, 64, 257, 1, 64, "desc", False, "no mask, 33 chunks"),
]

# (B, Q, NK, A, chunks, masked, the edge)
UNIFORM_CASES = [
    (1, 128, 257, 1, 1, True, "direct, sets up to 128 keys, the tail set is key 256 alone"),
    (1, 128, 257, 1, 5, True, "chunks of 56 keys: sets across chunk boundaries"),
    (1, 128, 257, 2, 64, True, "33 chunks of 8 keys: a set of 128 spans 17 chunks"),
    (1, 97, 129, 2, 5, True, "the fourth word holds one query; the last chunk is one key"),
    (2, 65, 127, 1, 2, True, "sets inside the ragged last step of 7 keys; B = 2"),
    (1, 33, 9, 1, 64, True, "2 chunks, the second is key 8 alone"),
    (2, 64, 128, 1, 64, True, "16 full chunks"),
    (1, 32, 8, 1, 1, True, "one step"),
    (1, 1, 129, 1, 5, True, "Q = 1"),
    (1, 96, 7, 1, 1, True, "NK < 8: sets of 1, 2, 4 inside one ragged step"),
    (1, 64, 1, 1, 1, True, "NK = 1"),
    (1, 33, 8, 1, 1, False, "no mask, NK = 8"),
    (1, 128, 128, 2, 2, False, "no mask, NK = 128, two chunks"),
    (2, 65, 1, 1, 1, False, "no mask, NK = 1"),
]

# the scale / peaked-score test: shapes, and (scale, t) with q, k = randn * t over the grid {0.05, 32^-0.5, 1.0} x {1, 3, 6}. Condition
# (b) of the derived bound needs about scale * t^2 <= 5; the three pairs of the grid that break it have their t lowered until it holds
# (32^-0.5: 6 -> 5, where t = 6 gives a bound of 9.2e-3 against 2e-3 * 4.3; 1.0: 3 -> 1.5 and 6 -> 2), the constant is untouched.
# 32^-0.5 at t = 5 puts scores at about +-100 natural units.
TOL_SHAPES = [(1, 97, 129, 2, 1), (2, 33, 257, 1, 5)]
TOL_INPUTS = [(0.05, 1), (0.05, 3), (0.05, 6), (S32, 1), (S32, 3), (S32, 5), (1.0, 1), (1.0, 1.5), (1.0, 2)]


def case_id(case):
    return "-".join(str(x) for x in case[:-1])


def cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def nonzero(t):
    """elements that do not compare equal to 0 (a NaN counts)"""
    return int((t != 0).sum())


def build_argmax(B, Q, NK, A, chunks, order, masked):
    """-> (argmax_case dict, bits, allowed, eff) on the CPU"""
    bits = allowed = eff = None
    if masked:
        mask, ok, eff = RA.edge_mask(B, A, Q, NK, chunks, torch.Generator().manual_seed(SEED + Q + NK))
        bits, allowed = RA.pack(mask.transpose(2, 3).contiguous()), RA.pack(ok)
    return RA.argmax_case(B, Q, NK, A, order, SEED + 7 * Q + NK, eff), bits, allowed, eff


def forward_routes(K, _lib, q, k, v, B, Q, NK, A, bits, allowed, chunks, scale):
    """The inference and the training forward at `chunks` (NaN-filled workspace) and the training forward on the direct route:
    -> (out, lse, out_direct, lse_direct) after asserting that the inference forward has the training forward's bits."""
    kw = dict(A=A, bits=bits, allowed=allowed, scale=scale)
    ws = None
    if chunks > 1:
        ws = torch.full((_lib.value("mss_m2f_attn_workspace_bytes", B, Q, A, chunks) // 4,), NAN, device="cuda")
    out_inf = K.m2f_masked_attention(q, k, v, B, Q, NK, chunks=chunks, ws=ws, **kw)
    out, lse = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, chunks=chunks, ws=None if ws is None else torch.full_like(ws, NAN), **kw)
    out_d, lse_d = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, chunks=1, **kw)
    assert torch.equal(out_inf, out)
    assert tuple(lse.shape) == (B, A, 8, Q) and torch.isfinite(lse).all() and torch.isfinite(lse_d).all()
    return out, lse, out_d, lse_d


def backward_all(K, _lib, q, k, v, out, lse, dout, B, Q, NK, A, bits, allowed, chunks, scale):
    """(dq, dk, dv) on a NaN-filled workspace into NaN-prefilled buffers, after asserting that the need=(False, True, True) and
    need=(True, False, False) calls give the same bits."""
    kw = dict(A=A, bits=bits, allowed=allowed, chunks=chunks, scale=scale)
    n_ws = _lib.value("mss_m2f_attn_bwd_workspace_bytes", B, Q, A, chunks) // 4
    shapes = ((B * Q, A * 256), (B * NK, A * 256), (B * NK, A * 256))

    def run(need):
        pre = tuple(torch.full(s, NAN, device="cuda") if n else None for s, n in zip(shapes, need))
        return K.m2f_masked_attention_backward(q, k, v, out, lse, dout, B, Q, NK, ws=torch.full((n_ws,), NAN, device="cuda"), grads=pre,
                                               need=need, **kw)
    full = run((True, True, True))
    kv = run((False, True, True))
    qq = run((True, False, False))
    assert kv[0] is None and torch.equal(kv[1], full[1]) and torch.equal(kv[2], full[2])
    assert qq[1] is None and qq[2] is None and torch.equal(qq[0], full[0])
    return full


def check_argmax(c, bits, allowed, B, Q, NK, A, chunks):
    from multishiftseg_amd import _lib, kernels as K
    q, k, v, dout, bits, allowed = cuda(c["q"], c["k"], c["v"], c["dout"], bits, allowed)
    out, lse, out_d, lse_d = forward_routes(K, _lib, q, k, v, B, Q, NK, A, bits, allowed, chunks, None)
    dq, dk, dv = backward_all(K, _lib, q, k, v, out, lse, dout, B, Q, NK, A, bits, allowed, chunks, None)
    torch.cuda.synchronize()
    assert torch.equal(out, out_d) and torch.equal(lse, lse_d)
    wrong = (out.cpu() != c["out"]).any(1).nonzero().flatten().tolist()
    assert not wrong, f"out differs from v[win] in rows {wrong[:8]}"
    assert torch.equal(lse.cpu(), c["lse"])
    assert nonzero(dq) == 0 and nonzero(dk) == 0
    assert torch.equal(dv.cpu(), c["dv"])
    loses = torch.ones((B, A, 8, NK), dtype=torch.bool).scatter_(3, c["win"], False)      # keys that win no query of their head
    assert nonzero(dv.cpu().view(B, NK, A, 8, 32).permute(0, 2, 3, 1, 4)[loses]) == 0


@pytest.mark.parametrize("case", ARGMAX_CASES, ids=case_id)
def test_argmax_attention_is_exact(case):
    """Construction 1 of the module docstring: out = v[win], lse = the winner's score, dv = the winners' dout sums, dq = dk = 0,
    all bit for bit, equal between the inference and the training forward and between the direct and the chunked route."""
    B, Q, NK, A, chunks, order, masked, _ = case
    c, bits, allowed, _ = build_argmax(B, Q, NK, A, chunks, order, masked)
    check_argmax(c, bits, allowed, B, Q, NK, A, chunks)


@pytest.mark.parametrize("case", UNIFORM_CASES, ids=case_id)
def test_uniform_attention_is_exact(case):
    """Construction 2: scale = 0.0, power-of-two allowed sets, integer v: out is exact on both routes, dq = dk = 0. dv is held to
    4 ulp of the float64 value, not to equality: log2f(2^n) and exp2f(-n) are not promised exact."""
    from multishiftseg_amd import _lib, kernels as K
    B, Q, NK, A, chunks, masked, _ = case
    c = RA.uniform_case(B, Q, NK, A, chunks, SEED, masked)
    bits = allowed = None
    if masked:
        bits, allowed = cuda(RA.pack(c["mask"].transpose(2, 3).contiguous()), RA.pack(c["ok"]))
    q, k, v, dout = cuda(c["q"], c["k"], c["v"], c["dout"])
    out, lse, out_d, lse_d = forward_routes(K, _lib, q, k, v, B, Q, NK, A, bits, allowed, chunks, 0.0)
    dq, dk, dv = backward_all(K, _lib, q, k, v, out, lse, dout, B, Q, NK, A, bits, allowed, chunks, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(out, out_d)
    assert torch.equal(out.cpu(), c["out"])
    want_lse = torch.log2(c["size"].double()).unsqueeze(2)                                 # [B, A, 1, Q]
    assert float((lse.cpu().double() - want_lse).abs().max()) <= 2e-6 and float((lse_d.cpu().double() - want_lse).abs().max()) <= 2e-6
    assert nonzero(dq) == 0 and nonzero(dk) == 0
    ulp = torch.from_numpy(np.spacing(c["dv"].abs().float().numpy())).double()
    err = (dv.cpu().double() - c["dv"]).abs()
    print(f"{case_id(case)}: dv worst {float((err / ulp).max()):.3g} ulp")
    assert bool((err <= 4.0 * ulp).all())


# ---- the mask-bits kernel -------------------------------------------------------------------------------------------------------
BITS_Q = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128]
# (source size, level size): up-sampling | down-sampling | identity | a 1-pixel source | a level of one key | a one-row source
BITS_GEOMS = [((3, 5), (24, 40)), ((12, 20), (6, 10)), ((7, 9), (7, 9)), ((1, 1), (4, 4)), ((4, 4), (1, 1)), ((1, 8), (2, 16))]


def grid_logits(src, B, Q, seed, neg=None):
    """[B, Q, hm, wm] float32 on the CPU, the protocol of bits_case_logits (test_gpu_transformer_decoder.py) with grid=True for any Q
    and source size: N(0, 5) rounded to the 1/8 grid, every 7th value exactly 0, query `neg` (default: the last, so that one rescue
    flag sits in the last bit in use) negative everywhere and (Q >= 2) query 0 positive everywhere: the two rescue flags."""
    neg = Q - 1 if neg is None else neg
    g = torch.Generator().manual_seed(seed)
    x = torch.round(5.0 * torch.randn((B, Q, src[0], src[1]), generator=g) * 8) / 8
    x.view(-1)[::7] = 0.0
    x[:, neg] = -x[:, neg].abs() - 0.125
    if Q >= 2:
        x[:, 0] = x[:, 0].abs() + 0.125
    return x


def sign_rows(x, dst):
    """(neg / pos rows bool [B, 2, hw, Q], allowed bool [B, 2, Q]) from the float64 interpolation, which holds no value at rounding
    level (asserted): on the 1/8 grid with dyadic ratios every fp32 blend is exact."""
    import ref_transformer_decoder as R
    it64 = R.interp_logits(x.double(), dst).flatten(2)                                     # [B, Q, hw]
    near = (it64.abs() < 1e-5 * it64.abs().max()) & (it64 != 0)
    assert int(near.sum()) == 0, "the committed inputs must hold no value at rounding level"
    want = torch.stack((it64 < 0, it64 > 0), 1).transpose(2, 3).contiguous()
    return want, (~want).any(2)


def nhwc_nan(x, ldq):
    """[B, Q, hm, wm] -> pixel-major [B, hm, wm, ldq] on the GPU, NaN in the padding columns"""
    B, Q, hm, wm = x.shape
    nhwc = torch.full((B, hm, wm, ldq), NAN, device="cuda")
    nhwc[..., :Q] = x.permute(0, 2, 3, 1).cuda()
    return nhwc


@pytest.mark.parametrize("Q", BITS_Q)
def test_mask_bits_are_exact_at_every_word_boundary(Q):
    """Every geometry at this Q (B = 3 on the first; ldq = Q rounded up to 4, and 8 more columns on the down-sampling one), NaN in the
    padding columns, which the kernel never reads. The bit rows -- whole words, so the padding bits of the last word are clear --
    and `allowed` equal the sign pattern of the float64 interpolation; a second call on the same buffers leaves the same words
    (`allowed` is OR-ed into, so this checks the memset). The buffers start from a junk pattern: every word is written."""
    from multishiftseg_amd import _lib, kernels as K
    W = (Q + 31) // 32
    for gi, (src, dst) in enumerate(BITS_GEOMS):
        for extra in ((0, 8) if gi == 1 else (0,)):
            B = 3 if gi == 0 else 1
            ldq = (Q + 3) // 4 * 4 + extra
            x = grid_logits(src, B, Q, 100 * Q + gi)
            want, want_allowed = sign_rows(x, dst)
            assert not want_allowed[:, 0, Q - 1].any() and want_allowed[:, 1, Q - 1].all()
            if Q >= 2:
                assert not want_allowed[:, 1, 0].any() and want_allowed[:, 0, 0].all()
            nhwc = nhwc_nan(x, ldq)
            hw = dst[0] * dst[1]
            words = torch.full((B * 2 * (hw + 1) * W,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            bits, allowed = words[:B * 2 * hw * W].view(B, 2, hw, W), words[B * 2 * hw * W:].view(B, 2, W)
            args = (_lib.ptr(nhwc), B, Q, ldq, src[0], src[1], dst[0], dst[1], _lib.ptr(bits), _lib.ptr(allowed))
            _lib.call("mss_m2f_attn_mask_bits_f32", *args)
            first = words.clone()
            _lib.call("mss_m2f_attn_mask_bits_f32", *args)
            bits_w, allowed_w = K.m2f_attn_mask_bits(nhwc, Q, dst)
            torch.cuda.synchronize()
            where = f"Q {Q} {src} -> {dst} B {B} ldq {ldq}"
            got = first[:B * 2 * hw * W].view(B, 2, hw, W).cpu()
            diff = RA.unpack(got, Q) != want
            assert int(diff.sum()) == 0, f"{where}: {int(diff.sum())} differing bits, first at {diff.nonzero()[0].tolist()}"
            assert torch.equal(got, RA.pack(want)), f"{where}: padding bits"
            # the bits of `allowed` past Q are unspecified (the kernel ORs ~neg of its idle lanes into them; no reader looks at them)
            assert torch.equal(RA.unpack(first[B * 2 * hw * W:].view(B, 2, W).cpu(), Q), want_allowed), f"{where}: allowed"
            assert torch.equal(words, first), f"{where}: the second call on the same buffers"
            assert torch.equal(bits_w, bits) and torch.equal(allowed_w, allowed), where


@pytest.mark.parametrize("B,Q,src,dst,chunks", [(2, 97, (3, 5), (12, 20), 5), (1, 128, (3, 5), (12, 20), 1), (1, 33, (4, 4), (1, 1), 1),
                                                (1, 65, (12, 20), (6, 10), 64)])
def test_mask_bits_feed_the_argmax_attention(B, Q, src, dst, chunks):
    """Construction 3: the bits and flags of m2f_attn_mask_bits (foreground and background: A = 2) go into the argmax attention as
    they are; the winners are those of the sign pattern of the float64 interpolation under the rescue rule, computed on the CPU."""
    from multishiftseg_amd import kernels as K
    x = grid_logits(src, B, Q, 7 * Q + chunks, neg=Q - 2)          # the last query is a plain one: its word, too, decides winners
    want, ok = sign_rows(x, dst)
    mask = want.transpose(2, 3)                                                            # [B, 2, Q, hw], True = not allowed
    eff = mask & ok.unsqueeze(-1)
    assert not ok[:, 0, Q - 2].any() and not ok[:, 1, 0].any()                              # both rescue flags are in play
    NK = dst[0] * dst[1]
    bits, allowed = K.m2f_attn_mask_bits(nhwc_nan(x, (Q + 3) // 4 * 4), Q, dst)
    assert torch.equal(bits.cpu(), RA.pack(want)) and torch.equal(RA.unpack(allowed.cpu(), Q), ok)
    c = RA.argmax_case(B, Q, NK, 2, "shuffle", SEED + Q, eff)
    check_argmax(c, bits, allowed, B, Q, NK, 2, chunks)


# ---- strides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Q,NK,A,ld,chunks", [(2, 37, 100, 1, 512, 1), (1, 100, 129, 2, 768, 3)])
def test_forward_on_column_slices(B, Q, NK, A, ld, chunks):
    """q, k, v as column slices of wider row-major tensors (offsets 256, 0, 256) and out= a slice of a wider buffer: the bits of the
    contiguous call, on both forwards; the columns of the wide `out` outside the slice keep their poison value."""
    from multishiftseg_amd import kernels as K
    g = torch.Generator().manual_seed(SEED + ld)
    cols = A * 256
    q, k, v = torch.randn((B * Q, cols), generator=g), torch.randn((B * NK, cols), generator=g), torch.randn((B * NK, cols), generator=g)
    mask, ok, _ = RA.edge_mask(B, A, Q, NK, chunks, g)
    q, k, v, bits, allowed = cuda(q, k, v, RA.pack(mask.transpose(2, 3).contiguous()), RA.pack(ok))
    kw = dict(A=A, bits=bits, allowed=allowed, chunks=chunks)
    want, want_lse = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, **kw)
    wide = []
    for t, off in ((q, 256), (k, 0), (v, 256)):
        w = torch.full((t.shape[0], ld), NAN, device="cuda")
        w[:, off:off + cols] = t
        wide.append(w[:, off:off + cols])
    POISON = -12345.0
    for off in (0, ld - cols):
        for lse_too in (False, True):
            buf = torch.full((B * Q, ld), POISON, device="cuda")
            dst = buf[:, off:off + cols]
            if lse_too:
                got, lse = K.m2f_masked_attention_lse(*wide, B, Q, NK, out=dst, **kw)
                assert torch.equal(lse, want_lse)
            else:
                got = K.m2f_masked_attention(*wide, B, Q, NK, out=dst, **kw)
            assert got.data_ptr() == dst.data_ptr() and torch.equal(dst, want)
            keep = torch.ones(ld, dtype=torch.bool, device="cuda")
            keep[off:off + cols] = False
            assert bool((buf[:, keep] == POISON).all())


# ---- scale and peaked scores, by tolerance --------------------------------------------------------------------------------------
def build_tolerance(B, Q, NK, A, chunks, masked, scale, t):
    """CPU: the inputs of one case, the float64 reference and the derived bound, after asserting its two conditions:
    (a) the float32 torch evaluation of the same inputs is inside the bound; (b) the bound is nowhere above 2e-3 max|ref|."""
    g = torch.Generator().manual_seed(4000 + 10 * Q + NK + int(1000 * scale) + int(10 * t))
    q, k = t * torch.randn((B * Q, A * 256), generator=g), t * torch.randn((B * NK, A * 256), generator=g)
    v = torch.randn((B * NK, A * 256), generator=g)
    bits = allowed = eff = None
    if masked:
        mask, ok, eff = RA.edge_mask(B, A, Q, NK, chunks, g)
        bits, allowed = RA.pack(mask.transpose(2, 3).contiguous()), RA.pack(ok)
    ref, bound = RA.derived_bound(q, k, v, eff, B, Q, NK, A, scale)
    e32 = (RA.attention(q, k, v, eff, B, Q, NK, A, scale).double() - ref).abs()
    assert bool((e32 <= bound).all()), ("(a)", float((e32 / bound).max()))
    assert float(bound.max()) <= 2e-3 * float(ref.abs().max()), ("(b)", float(bound.max()), float(ref.abs().max()))
    return q, k, v, bits, allowed, ref, bound


@pytest.mark.parametrize("B,Q,NK,A,chunks", TOL_SHAPES)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("scale,t", TOL_INPUTS)
def test_scale_and_peaked_scores(B, Q, NK, A, chunks, masked, scale, t):
    """softmax(scale q k^T + mask) v for q, k = randn * t against float64 under a derived bound. With p the float64 softmax and
    delta_i = 36 * 2^-24 * scale * max_k sum_d |q_id| |k_kd|:
        |out_id - ref_id| <= 2 * [expm1(2 delta_i) + (NK + 16) * 2^-24] * sum_k p_ik |v_kd|.
    expm1(2 delta_i) covers the rounding of the 32-term score chain (32 products and sums + the fold of scale * log2 e into q + the
    subtraction of the maximum: 36 roundings of terms bounded by the absolute sum), in numerator and normaliser; (NK + 16) * 2^-24
    covers the exponential, the NK-term accumulation, the reciprocal and the product; the whole is doubled. Conditions (a) and (b)
    are asserted on the CPU before the first GPU call (build_tolerance)."""
    from multishiftseg_amd import kernels as K
    q, k, v, bits, allowed, ref, bound = build_tolerance(B, Q, NK, A, chunks, masked, scale, t)
    q, k, v, bits, allowed = cuda(q, k, v, bits, allowed)
    for ch in sorted({1, chunks}):
        out = K.m2f_masked_attention(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed, chunks=ch, scale=scale).cpu()
        assert torch.isfinite(out).all()
        err = (out.double() - ref).abs()
        print(f"B {B} Q {Q} NK {NK} A {A} chunks {ch} masked {masked} scale {scale:.4g} t {t}: worst error {float(err.max()):.3g}, "
              f"worst error / bound {float((err / bound).max()):.3g}")
        assert bool((err <= bound).all())
