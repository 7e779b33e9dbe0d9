"""CPU: the exact constructions of tests/test_gpu_attention_exact.py stay honest without a GPU.

tests/ref_attention.py restates the streaming softmax of csrc/m2f_attn.hip in NumPy float32 (stream_forward: the lane / word / bit
addressing of the mask, the 8-key steps, the chunk plan, the merge). Here that restatement reproduces the expected values of the
argmax and the uniform construction bit for bit, on the direct and on the chunked route, and each of three addressing faults -- one
mask word shifted by one bit, the value rows of two keys swapped, the last key dropped -- breaks that equality: the constructions
can fail. The builders of every GPU case run here as well (winners at the word boundaries differ; the derived bound of the
tolerance test holds its two conditions), which is the CPU pre-flight of the GPU file."""
import numpy as np
import pytest
import torch

import ref_attention as RA
import test_gpu_attention_exact as X

# (B, Q, NK, A, chunks, order): two waves with all four words | the fourth word holds one query, a last chunk of one key
CPU_CASES = [(1, 128, 73, 1, 1, "shuffle"), (1, 97, 129, 1, 5, "asc")]
HEADS = (0, 5)


def head_cols(heads, A=1):
    return np.concatenate([np.arange(a * 256 + h * 32, a * 256 + h * 32 + 32) for a in range(A) for h in heads])


def shift_word(bits, w):
    """word w of every key, shifted up by one bit"""
    out = bits.clone()
    x = ((bits[..., w].to(torch.int64) & 0xFFFFFFFF) << 1) & 0xFFFFFFFF
    out[..., w] = torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)
    return out


def swap_rows(t, B, NK, j1, j2):
    out = t.clone().view(B, NK, -1)
    out[:, [j1, j2]] = out[:, [j2, j1]]
    return out.view(B * NK, -1)


def drop_last(t, B, NK):
    return t.view(B, NK, -1)[:, :NK - 1].reshape(B * (NK - 1), -1)


@pytest.mark.parametrize("B,Q,NK,A,chunks,order", CPU_CASES)
def test_argmax_construction_restated_and_its_faults(B, Q, NK, A, chunks, order):
    g = torch.Generator().manual_seed(5)
    mask, ok, eff = RA.edge_mask(B, A, Q, NK, chunks, g)
    c = RA.argmax_case(B, Q, NK, A, order, 11, eff)
    assert RA.boundary_winners_differ(c["win"], Q, NK)
    bits, allowed = RA.pack(mask.transpose(2, 3).contiguous()), RA.pack(ok)
    cols = head_cols(HEADS)
    want, want_lse = c["out"].numpy()[:, cols], c["lse"].numpy()[:, :, HEADS]

    def run(k=c["k"], v=c["v"], bits=bits, nk=NK):
        out, lse = RA.stream_forward(c["q"].numpy(), k.numpy(), v.numpy(), bits.numpy(), allowed.numpy(), B, Q, nk, A, 32 ** -0.5, chunks, HEADS)
        return out[:, cols], lse[:, :, HEADS]

    out, lse = run()
    assert np.array_equal(out, want) and np.array_equal(lse, want_lse)
    if chunks > 1:                                                    # the direct route gives the same bits
        o1, l1 = RA.stream_forward(c["q"].numpy(), c["k"].numpy(), c["v"].numpy(), bits.numpy(), allowed.numpy(), B, Q, NK, A, 32 ** -0.5, 1, HEADS)
        assert np.array_equal(o1[:, cols], want) and np.array_equal(l1[:, :, HEADS], want_lse)
    # the faults
    for w in range((Q + 31) // 32):
        assert not np.array_equal(run(bits=shift_word(bits, w))[0], want), f"a shifted word {w} goes unnoticed"
    win = c["win"][0, 0, HEADS[0]]
    j1, j2 = int(win[0]), int(win[Q - 1])
    assert j1 != j2
    assert not np.array_equal(run(v=swap_rows(c["v"], B, NK, j1, j2))[0], want)
    assert bool((c["win"] == NK - 1).any())
    short = bits[:, :, :NK - 1].contiguous()
    assert not np.array_equal(run(k=drop_last(c["k"], B, NK), v=drop_last(c["v"], B, NK), bits=short, nk=NK - 1)[0], want)


@pytest.mark.parametrize("B,Q,NK,A,chunks", [(1, 128, 73, 1, 1), (1, 97, 129, 1, 5)])
def test_uniform_construction_restated_and_its_faults(B, Q, NK, A, chunks):
    c = RA.uniform_case(B, Q, NK, A, chunks, 13)
    bits, allowed = RA.pack(c["mask"].transpose(2, 3).contiguous()), RA.pack(c["ok"])
    cols = head_cols(HEADS)
    want = c["out"].numpy()[:, cols]

    def run(v=c["v"], bits=bits, nk=NK, ch=chunks):
        out, lse = RA.stream_forward(c["q"].numpy(), c["k"].numpy()[:B * nk], v.numpy(), bits.numpy(), allowed.numpy(), B, Q, nk, A, 0.0, ch, HEADS)
        return out[:, cols], lse

    out, lse = run()
    assert np.array_equal(out, want)
    assert np.abs(lse[:, :, HEADS] - np.log2(c["size"].numpy())[:, :, None]).max() <= 1e-6
    assert np.array_equal(run(ch=1)[0], want)
    for w in range((Q + 31) // 32):
        assert not np.array_equal(run(bits=shift_word(bits, w))[0], want), f"a shifted word {w} goes unnoticed"
    member = ~c["mask"][0, 0, 0]                                     # query 0's run: one key inside, one outside
    j1, j2 = int(member.nonzero()[0]), int((~member).nonzero()[0])
    assert not np.array_equal(run(v=swap_rows(c["v"], B, NK, j1, j2))[0], want)
    assert B == 1                                                    # k of a shorter key range: the leading rows (k does not matter)
    assert not np.array_equal(run(v=drop_last(c["v"], B, NK), bits=bits[:, :, :NK - 1].contiguous(), nk=NK - 1)[0], want)


def test_chain_construction_restated_and_its_faults():
    """Construction 3 with the sign pattern of the float64 interpolation in the place of the mask-bits kernel's output: foreground
    and background rows (A = 2), both rescue flags in play."""
    B, Q, src, dst, chunks = 1, 65, (12, 20), (6, 10), 64
    NK = dst[0] * dst[1]
    want, ok = X.sign_rows(X.grid_logits(src, B, Q, 7 * Q + chunks, neg=Q - 2), dst)
    assert not ok[:, 0, Q - 2].any() and not ok[:, 1, 0].any()
    c = RA.argmax_case(B, Q, NK, 2, "shuffle", X.SEED + Q, want.transpose(2, 3) & ok.unsqueeze(-1))
    bits, allowed = RA.pack(want), RA.pack(ok)
    cols = head_cols(HEADS, 2)
    wanted = c["out"].numpy()[:, cols]

    def run(v=c["v"], bits=bits):
        return RA.stream_forward(c["q"].numpy(), c["k"].numpy(), v.numpy(), bits.numpy(), allowed.numpy(), B, Q, NK, 2, 32 ** -0.5, chunks, HEADS)[0][:, cols]

    assert np.array_equal(run(), wanted)
    for w in range((Q + 31) // 32):
        assert not np.array_equal(run(bits=shift_word(bits, w)), wanted), f"a shifted word {w} goes unnoticed"
    assert not np.array_equal(run(bits=bits.flip(1).contiguous()), wanted), "foreground and background rows swapped"
    win = c["win"][0, 0, HEADS[0]]
    j1 = int(win[1])
    j2 = int(win[win != j1][0])
    assert not np.array_equal(run(v=swap_rows(c["v"], B, NK, j1, j2)), wanted)


def test_every_gpu_case_builds_and_is_not_vacuous():
    """The expected-value builders of every GPU case: all winners are allowed keys; the queries next to a word boundary have
    different winners; every key range has a key that wins and a key that loses; uniform runs reach the last key, cross a chunk
    boundary and, where the last step is ragged, sit wholly inside it."""
    assert len(X.ARGMAX_CASES) <= 60 and len(X.UNIFORM_CASES) <= 60
    for case in X.ARGMAX_CASES:
        B, Q, NK, A, chunks, order, masked = case[:7]
        c, bits, allowed, eff = X.build_argmax(*case[:7])
        assert tuple(c["win"].shape) == (B, A, 8, Q)
        if masked:
            assert not bool(eff.gather(3, c["win"].permute(0, 1, 3, 2)).any()), case
            assert RA.boundary_winners_differ(c["win"], Q, NK), case
        assert torch.isfinite(c["lse"]).all()
    for case in X.UNIFORM_CASES:
        B, Q, NK, A, chunks, masked = case[:6]
        c = RA.uniform_case(B, Q, NK, A, chunks, X.SEED, masked)
        if not masked:
            assert NK & (NK - 1) == 0, case
            continue
        member = ~c["mask"]
        kpc, n = RA.chunk_plan(NK, chunks)
        first, last = member.float().argmax(-1), NK - 1 - member.flip(-1).float().argmax(-1)
        assert bool((last == NK - 1).any()), case
        if n > 1 and Q >= 16:
            assert bool(((first // kpc) != (last // kpc)).any()), case
        if Q >= 16 and NK >= 16:
            assert bool((((first // 8) != (last // 8)) & (c["size"] <= 8)).any()), case
        if NK % 8 and Q >= 8:
            assert bool((first >= NK // 8 * 8).any()), case


@pytest.mark.parametrize("B,Q,NK,A,chunks", X.TOL_SHAPES)
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("scale,t", X.TOL_INPUTS)
def test_derived_bound_conditions(B, Q, NK, A, chunks, masked, scale, t):
    """Conditions (a) and (b) of the tolerance test hold for every committed input."""
    X.build_tolerance(B, Q, NK, A, chunks, masked, scale, t)
