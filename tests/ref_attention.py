"""Test helper: the masked attention of the GMA transformer decoder in stock torch (the formula of attention_reference in
test_gpu_transformer_decoder.py, without the in-place writes, so that torch autograd can differentiate it), the packing of
bool masks into the attention kernel's words, and the builders of the exact constructions of test_gpu_attention_exact.py /
test_attention_exact_cpu.py (inputs on the CPU with their expected results, and a NumPy float32 restatement of the streaming
softmax of csrc/m2f_attn.hip)."""
import math

import numpy as np
import torch

KB = 8                                            # keys per online-softmax step of m2f_masked_attention_kernel
G = 1024.0                                        # |q| of the argmax construction
LOG2E = np.float32(1.4426950408889634)
# edge_mask: rows that see only key 0 / only the last key / only the first key of the last chunk / nothing (rescued) / only ONE_KEY[row]
# / only an eighth of the key range (WINDOW[row] eighths from the start). Queries 31|32|33, 63|64|65 and 95|96|97 get different winners.
NEG_ROWS, LAST_ROWS, CHUNK_ROWS, RESCUE_ROWS = (3,), (1, 64), (5,), (2, 33, 97)
ONE_KEY = {32: 2, 96: 5}
WINDOW = {31: 1, 63: 2, 65: 3, 95: 4}


def pack(mask):
    """bool [..., Q] -> int32 words [..., ceil(Q/32)]."""
    Q = mask.shape[-1]
    W = (Q + 31) // 32
    m = torch.zeros(mask.shape[:-1] + (W * 32,), dtype=torch.int64, device=mask.device)
    m[..., :Q] = mask
    words = (m.view(mask.shape[:-1] + (W, 32)) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def unpack(bits, Q):
    """int32 words [..., W] -> bool [..., Q]."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(-1) >> sh) & 1).flatten(-2)[..., :Q].bool()


def attention(q, k, v, mask, B, Q, NK, A, scale=None):
    """softmax(scale q k^T + mask) v per (image, attention, head) in the dtype of q (scale: 1 / sqrt(32) when None); q [B*Q, A*256],
    k / v [B*NK, A*256], mask bool [B, A, Q, NK] (True = not allowed) or None."""
    scale = 32 ** -0.5 if scale is None else scale
    outs = []
    for a in range(A):
        sl = slice(a * 256, (a + 1) * 256)
        qq = q[:, sl].view(B, Q, 8, 32).transpose(1, 2)
        kk = k[:, sl].view(B, NK, 8, 32).transpose(1, 2)
        vv = v[:, sl].view(B, NK, 8, 32).transpose(1, 2)
        s = torch.matmul(qq * scale, kk.transpose(2, 3))
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


# ---- the exact constructions ---------------------------------------------------------------------------------------------------
def chunk_plan(NK, chunks):
    """chunk_plan of csrc/m2f_attn.hip: (keys per chunk, a multiple of 8; the chunk count actually launched)."""
    kpc = (-(-NK // chunks) + KB - 1) // KB * KB
    return kpc, -(-NK // kpc)


def edge_mask(B, A, Q, NK, chunks, g):
    """-> (mask, ok, eff): mask bool [B, A, Q, NK] (True = not allowed) as it is packed into the bit rows, ok bool [B, A, Q] the
    `allowed` bits, eff the mask the rescue rule makes of both. Rows are random at 50 % and keep at least one key. Rows WINDOW
    (NK >= 64) are random inside one eighth of the key range and masked outside it. Key NK // 2 is masked for every query (NK >= 3),
    and so is the whole chunk 1 when `chunks` makes at least three chunks. Then: rows NEG_ROWS see only key 0, LAST_ROWS only the
    last key, CHUNK_ROWS only the first key of the last chunk, ONE_KEY only that key; RESCUE_ROWS are fully masked with their
    `allowed` bit clear (at Q = 1: row 0 of the last image / attention, if there are two)."""
    kpc, n = chunk_plan(NK, chunks)
    mask = torch.rand((B, A, Q, NK), generator=g) < 0.5
    if NK >= 64:
        for r, e in WINDOW.items():
            if r < Q:
                mask[:, :, r, :e * NK // 8] = True
                mask[:, :, r, e * NK // 8 + 1] = False
                mask[:, :, r, (e + 1) * NK // 8:] = True
    if n >= 3:
        mask[..., kpc:2 * kpc] = True
    if NK >= 3:
        mask[..., NK // 2] = True
    none = mask.all(-1).nonzero()                                   # such a row gets one key of chunk 0 back, not the same for neighbours
    mask[none[:, 0], none[:, 1], none[:, 2], none[:, 2] % 8 if NK >= 17 else 0] = False
    ok = torch.ones((B, A, Q), dtype=torch.bool)
    only = [(r, 0) for r in NEG_ROWS] + [(r, NK - 1) for r in LAST_ROWS] + [(r, (n - 1) * kpc) for r in CHUNK_ROWS] + \
        [(r, min(key, NK - 1)) for r, key in ONE_KEY.items()]
    for r, key in only:
        if r < Q:
            mask[:, :, r] = True
            mask[:, :, r, key] = False
    for r in RESCUE_ROWS:
        if r < Q:
            mask[:, :, r] = True
            ok[:, :, r] = False
    if Q == 1 and B * A > 1:
        mask[-1, -1, 0] = True
        ok[-1, -1, 0] = False
    eff = mask & ok.unsqueeze(-1)
    assert not eff.all(-1).any()
    return mask, ok, eff


def _heads(t, B, N, A):
    """[B*N, A*256] -> [B, A, 8, N, 32]"""
    return t.view(B, N, A, 8, 32).permute(0, 2, 3, 1, 4)


def _rows(t, B, N, A):
    """[B, A, 8, N, 32] -> [B*N, A*256]"""
    return t.permute(0, 3, 1, 2, 4).reshape(B * N, A * 256).contiguous()


def argmax_case(B, Q, NK, A, order, seed, eff=None, scale=None):
    """The argmax construction. Per (image, attention, head) query i is +-G in the single component d(i) and every component of the
    keys is a permutation of the NK integers around 0 (`order`: "asc" -- ascending with the key index, the same in every component,
    so that the running maximum of a +G query moves at every step; "desc"; "shuffle" -- a random permutation per component). One
    integer step of k is G * scale * log2(e) ~ 261 units of the kernel's log2-domain score, so every allowed key but the best has
    exp2(<= -160) = 0 exactly. v: integers in [-8, 8], dout: integers in [-4, 4].
    -> dict of float32 CPU tensors q, k, v, dout and the expected win [B, A, 8, Q] (key index), out, lse [B, A, 8, Q] (log2 domain),
    dv; dq and dk are expected to be 0."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(NK) - NK // 2
    if order == "asc":
        kint = base.view(1, 1, 1, NK, 1).expand(B, A, 8, NK, 32)
    elif order == "desc":
        kint = base.flip(0).view(1, 1, 1, NK, 1).expand(B, A, 8, NK, 32)
    else:
        kint = base[torch.rand((B, A, 8, NK, 32), generator=g).argsort(3)]
    i = torch.arange(Q)
    sign = 1 - 2 * ((i + i // 32) % 2)                                                      # differs between i and i + 32 as well
    comp = (5 * i.view(1, 1, Q) + 3 * torch.arange(8).view(1, 8, 1) + 11 * torch.arange(A).view(A, 1, 1)) % 32   # [A, 8, Q]
    qh = torch.zeros((B, A, 8, Q, 32))
    qh.scatter_(4, comp.view(1, A, 8, Q, 1).expand(B, A, 8, Q, 1), (G * sign).float().view(1, 1, 1, Q, 1).expand(B, A, 8, Q, 1))
    vh = torch.randint(-8, 9, (B, A, 8, NK, 32), generator=g).float()
    gh = torch.randint(-4, 5, (B, A, 8, Q, 32), generator=g).float()
    # integer scores: sign_i * k_j[d(i)]
    kq = kint.gather(4, comp.view(1, A, 8, 1, Q).expand(B, A, 8, NK, Q)).transpose(3, 4)      # [B, A, 8, Q, NK]
    sc = kq * sign.view(1, 1, 1, Q, 1)
    if eff is not None:
        sc = sc.masked_fill(eff.unsqueeze(2), -(1 << 40))
    win = sc.argmax(-1)                                                                     # [B, A, 8, Q]
    kwin = kq.gather(4, win.unsqueeze(-1)).squeeze(-1)
    out = vh.gather(3, win.unsqueeze(-1).expand(B, A, 8, Q, 32))
    dv = torch.zeros((B, A, 8, NK, 32)).scatter_add_(3, win.unsqueeze(-1).expand(B, A, 8, Q, 32), gh)
    # the kernel's chain: qr = q * (scale * log2e) in fp32, then one non-zero fma term, rounded once
    sl2 = np.float32(32 ** -0.5 if scale is None else scale) * LOG2E
    qr = (G * sign).numpy().astype(np.float32) * sl2
    lse = torch.from_numpy(qr.reshape(1, 1, 1, Q) * kwin.numpy().astype(np.float32))
    return dict(q=_rows(qh, B, Q, A), k=_rows(kint.float(), B, NK, A), v=_rows(vh, B, NK, A), dout=_rows(gh, B, Q, A), win=win,
                out=_rows(out, B, Q, A), lse=lse, dv=_rows(dv, B, NK, A))


def boundary_winners_differ(win, Q, NK):
    """Queries 31/32/33, 63/64/65 and 95/96/97 (those below Q) have pairwise different winners in some head of every (image,
    attention): a shift by one bit or one word then changes the result."""
    for c in (32, 64, 96):
        if c + 1 >= Q or NK < 64:
            continue
        t = win[..., c - 1:c + 2]
        d = (t[..., 0] != t[..., 1]) & (t[..., 1] != t[..., 2]) & (t[..., 0] != t[..., 2])
        if not bool(d.any(2).all()):
            return False
    return True


def uniform_case(B, Q, NK, A, chunks, seed, masked=True):
    """The uniform construction (scale = 0: every allowed key has p = 1). Query i may attend to a run of 2^(i mod n) keys (sizes 1 ..
    min(NK, 128)) placed across a multiple of 8, across a chunk boundary of `chunks`, or at the very end of the key range (inside
    the ragged last step); masked=False: every key (exact only for NK a power of two). v: integers in [-8, 8]; q, k: N(0, 1), they do
    not matter; dout: integers in [0, 4], so that dv is a sum without cancellation.
    -> dict of CPU tensors q, k, v, dout, mask (None when not masked), ok, size [B, A, Q], and the expected out (exact), dv (float64)."""
    g = torch.Generator().manual_seed(seed)
    kpc, n = chunk_plan(NK, chunks)
    q = torch.randn((B * Q, A * 256), generator=g)
    k = torch.randn((B * NK, A * 256), generator=g)
    vh = torch.randint(-8, 9, (B, A, 8, NK, 32), generator=g).float()
    gh = torch.randint(0, 5, (B, A, 8, Q, 32), generator=g).float()
    mask = None
    member = torch.ones((B, A, Q, NK), dtype=torch.bool)
    if masked:
        npow = int(math.log2(min(NK, 128))) + 1
        edges = sorted(set(range(KB, NK, KB)) | set(range(kpc, NK, kpc))) or [0]
        chunk_edges = list(range(kpc, NK, kpc)) or edges
        for b in range(B):
            for a in range(A):
                for i in range(Q):
                    t = i + 3 * (b * A + a)
                    size = 1 << (t % npow)
                    turn = t // npow
                    if turn % 3 == 0:
                        start = NK - size                                                  # the tail: inside the ragged last step
                    elif turn % 3 == 1:
                        start = chunk_edges[turn % len(chunk_edges)] - max(1, size // 2)   # across a chunk boundary
                    else:
                        start = edges[(5 * turn) % len(edges)] - max(1, size // 2)         # across an 8-key step
                    start = min(max(start, 0), NK - size)
                    member[b, a, i] = False
                    member[b, a, i, start:start + size] = True
        mask = ~member
    size = member.sum(-1)
    assert bool(((size & (size - 1)) == 0).all())
    w = (member.double() / size.unsqueeze(-1).double()).unsqueeze(2)                         # [B, A, 1, Q, NK]
    out = torch.matmul(w, vh.double())                                                      # exact: integers over a power of two
    dv = torch.matmul(w.transpose(3, 4), gh.double())
    assert torch.equal(out.float().double(), out)
    return dict(q=q, k=k, v=_rows(vh, B, NK, A), dout=_rows(gh, B, Q, A), mask=mask, ok=torch.ones((B, A, Q), dtype=torch.bool),
                size=size, out=_rows(out.float(), B, Q, A), dv=_rows(dv, B, NK, A))


def derived_bound(q, k, v, eff, B, Q, NK, A, scale):
    """(ref64, bound) of the scale / peaked-score test: with p the float64 softmax and
    delta_i = 36 * 2^-24 * scale * max_k sum_d |q_id| |k_kd| (k over the keys query i may attend to),
    |out_id - ref_id| <= 2 * [expm1(2 delta_i) + (NK + 16) * 2^-24] * sum_k p_ik |v_kd|."""
    q, k, v = q.double(), k.double(), v.double()
    ref = attention(q, k, v, eff, B, Q, NK, A, scale)
    pv = attention(q, k, v.abs(), eff, B, Q, NK, A, scale)
    qk = torch.matmul(_heads(q.abs(), B, Q, A), _heads(k.abs(), B, NK, A).transpose(3, 4))   # [B, A, 8, Q, NK]
    if eff is not None:
        qk = qk.masked_fill(eff.unsqueeze(2), 0.0)
    delta = 36.0 * 2.0 ** -24 * scale * qk.amax(-1, keepdim=True)                          # [B, A, 8, Q, 1]
    rel = 2.0 * (torch.expm1(2.0 * delta) + (NK + 16) * 2.0 ** -24)
    return ref, _rows(rel.expand(B, A, 8, Q, 32), B, Q, A) * pv


# ---- the streaming softmax of csrc/m2f_attn.hip in NumPy float32 -----------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, one rounding of the sum to 53 bits before the one to 24."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def stream_forward(q, k, v, bits, allowed, B, Q, NK, A, scale, chunks, heads=range(8)):
    """m2f_masked_attention_kernel + m2f_attn_merge_kernel restated: lane = query, two mask words per wave of 64 lanes picked as
    the kernel picks them, 8-key steps with one rescale each, the chunk plan and the merge in chunk order. q / k / v: float32 arrays
    [B*Q | B*NK, A*256]; bits int32 [B, A, NK, W] / allowed int32 [B, A, W] or None. -> (out, lse [B, A, 8, Q]); heads outside `heads`
    are left NaN."""
    q, k, v = (np.ascontiguousarray(t, dtype=np.float32) for t in (q, k, v))
    kpc, n = chunk_plan(NK, chunks)
    QS, W = 64 * ((Q + 63) // 64), (Q + 31) // 32
    sl2 = np.float32(scale) * LOG2E
    lane_q = np.arange(QS)
    qc = np.minimum(lane_q, Q - 1)
    wave, lane = lane_q // 64, lane_q % 64
    word = np.where(lane >= 32, np.minimum(2 * wave + 1, W - 1), 2 * wave)
    sh = (lane & 31).astype(np.uint32)
    ninf = np.float32(-np.inf)
    out = np.full((B * Q, A * 256), np.nan, np.float32)
    lse = np.full((B, A, 8, Q), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for a in range(A):
                if bits is not None:
                    brow = np.asarray(bits[b, a]).view(np.uint32)
                    live = np.asarray(allowed[b, a]).view(np.uint32)[word]
                for hd in heads:
                    col = a * 256 + hd * 32
                    qr = q[b * Q + qc, col:col + 32] * sl2
                    kb, vb = k[b * NK:(b + 1) * NK, col:col + 32], v[b * NK:(b + 1) * NK, col:col + 32]
                    parts = []
                    for c in range(n):
                        k0, k1 = c * kpc, min(NK, (c + 1) * kpc)
                        m, l, acc = np.full(QS, ninf), np.zeros(QS, np.float32), np.zeros((QS, 32), np.float32)
                        for kk in range(k0, k1, KB):
                            key = np.minimum(kk + np.arange(KB), k1 - 1)
                            dot = np.zeros((QS, KB), np.float32)
                            for d in range(32):
                                dot = _fma(qr[:, d:d + 1], kb[key, d][None, :], dot)
                            masked = np.broadcast_to((kk + np.arange(KB) >= k1)[None, :], (QS, KB)).copy()
                            if bits is not None:
                                masked |= (((brow[key][:, word].T & live[:, None]) >> sh[:, None]) & 1).astype(bool)
                            s = np.where(masked, ninf, dot)
                            mn = np.maximum(m, s.max(1))
                            mref = np.where(mn == ninf, np.float32(0), mn)
                            alpha = np.exp2(m - mref)
                            l = l * alpha
                            acc = acc * alpha[:, None]
                            for j in range(KB):
                                p = np.exp2(s[:, j] - mref)
                                l = l + p
                                acc = _fma(p[:, None], vb[key[j]][None, :], acc)
                            m = mn
                        parts.append((acc, m, l))
                    if n == 1:
                        acc, m, l = parts[0]
                        o, ls = acc * (np.float32(1) / l)[:, None], m + np.log2(l)
                    else:
                        M = np.full(QS, ninf)
                        for _, m, _ in parts:
                            M = np.maximum(M, m)
                        num, den = np.zeros((QS, 32), np.float32), np.zeros(QS, np.float32)
                        for acc, m, l in parts:
                            wgt = np.where(m == ninf, np.float32(0), np.exp2(m - M))
                            num = _fma(wgt[:, None], acc, num)
                            den = _fma(wgt, l, den)
                        o, ls = num / den[:, None], M + np.log2(den)
                    out[b * Q:(b + 1) * Q, col:col + 32] = o[:Q]
                    lse[b, a, hd] = ls[:Q]
    return out, lse
