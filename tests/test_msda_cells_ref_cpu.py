"""The float64 MSDeformAttn reference that takes the bilinear cell as an input (tests/ref_msda_cells.py), checked without a GPU:
it is oracle/msda.py when the cell is floor(p); at an exact kink both neighbouring cells give the same out / grad_value /
grad_attn and different grad_loc; and the dyadic lattice recipe of tests/test_gpu_msda_lattice.py is exact in fp32."""
import numpy as np
import pytest

import ref_msda_cells as R
from oracle import msda as omsda

LATTICE = [
    ([(32, 64), (8, 8), (16, 32)], 2, 96, 8, 4, 32),
    ([(1, 256), (256, 1), (4, 4)], 2, 60, 8, 4, 32),
    ([(16, 32), (8, 8)], 1, 50, 4, 4, 16),
]


def _random_inputs(seed, shapes, N, Lq, M, P, D):
    rng = np.random.default_rng(seed)
    shp = np.asarray(shapes, dtype=np.int64)
    S, L = int(shp.prod(1).sum()), len(shapes)
    attn = rng.random((N, Lq, M, L, P))
    attn /= attn.sum((-1, -2), keepdims=True)
    return dict(value=rng.standard_normal((N, S, M, D)), loc=rng.uniform(-0.2, 1.2, (N, Lq, M, L, P, 2)), attn=attn,
                grad_out=rng.standard_normal((N, Lq, M * D)), shapes=shp, starts=R.level_starts(shp))


def _both(g, shift=0.0):
    c = R.cells(g["loc"], g["shapes"], shift)
    out = R.forward(g["value"], g["shapes"], g["starts"], g["loc"], g["attn"], *c)
    return (out,) + R.backward(g["value"], g["shapes"], g["starts"], g["loc"], g["attn"], g["grad_out"], *c)


def _oracle(g, dtype=np.float64):
    a = {k: g[k].astype(dtype) for k in ("value", "loc", "attn", "grad_out")}
    out = omsda.forward(a["value"], g["shapes"], g["starts"], a["loc"], a["attn"])
    return (out,) + omsda.backward(a["value"], g["shapes"], g["starts"], a["loc"], a["attn"], a["grad_out"])


@pytest.mark.parametrize("shapes,N,Lq,M,P,D", [([(6, 4), (3, 2)], 2, 7, 8, 4, 32), ([(22, 22), (44, 44), (88, 88)], 1, 40, 8, 4, 32),
                                                ([(1, 9), (9, 1), (5, 3)], 2, 33, 2, 3, 7)])
def test_shift_zero_is_the_oracle_on_random_inputs(shapes, N, Lq, M, P, D):
    g = _random_inputs(len(shapes) + Lq, shapes, N, Lq, M, P, D)
    assert 0.2 < R.cells(g["loc"], g["shapes"])[2].mean() < 0.9          # both sides of the inside test are populated
    for got, want, name in zip(_both(g), _oracle(g), ("out", "grad_value", "grad_loc", "grad_attn")):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("shapes,N,Lq,M,P,D", LATTICE)
def test_shift_zero_is_the_oracle_on_the_lattice(shapes, N, Lq, M, P, D):
    g = R.lattice_inputs(5, shapes, N, Lq, M, P, D)
    for got, want, name in zip(_both(g), _oracle(g), ("out", "grad_value", "grad_loc", "grad_attn")):
        assert got.dtype == np.float64 and np.array_equal(got, want), name


@pytest.mark.parametrize("shapes,N,Lq,M,P,D", LATTICE)
def test_the_lattice_recipe_is_exact_in_fp32(shapes, N, Lq, M, P, D):
    """oracle/msda.py run in fp32 gives what it gives in fp64, and the fp64 results are fp32 numbers: on these inputs a
    correct fp32 kernel has no rounding to hide behind, whatever order it adds in."""
    g = R.lattice_inputs(5, shapes, N, Lq, M, P, D)
    for k in ("value", "loc", "attn", "grad_out"):
        assert np.array_equal(g[k].astype(np.float32).astype(np.float64), g[k]), k
    for lo, hi, name in zip(_oracle(g, np.float32), _oracle(g), ("out", "grad_value", "grad_loc", "grad_attn")):
        assert lo.dtype == np.float32 and hi.dtype == np.float64
        assert np.array_equal(hi.astype(np.float32).astype(np.float64), hi), name
        assert np.array_equal(lo.astype(np.float64), hi), name
        assert np.abs(hi).max() > 0, name


def test_lattice_coordinates_cover_kinks_and_borders():
    shapes = [(32, 64), (8, 8), (16, 32)]
    g = R.lattice_inputs(5, shapes, 2, 256, 8, 4, 32)
    p = g["p"]
    assert 0.45 < (p == np.round(p)).mean() < 0.55                       # half of all coordinates are exact integers
    assert np.array_equal(R.pixel_coords(g["loc"], shapes), p)
    for l, (H, W) in enumerate(shapes):
        for ax, E in ((0, W), (1, H)):
            for edge in (-1, 0, E - 1, E):
                assert (p[:, :, :, l, :, ax] == edge).any(), (l, ax, edge)
    inside = R.cells(g["loc"], shapes)[2]
    assert 0.4 < inside.mean() < 0.9


def test_both_cells_of_an_exact_kink_agree_except_in_grad_loc():
    """Every coordinate an exact integer: shift = -2e-5 puts each sample into the cell below / left of the one floor() picks.
    The bilinear surface is continuous there, so out, grad_value and grad_attn agree to 1e-12; grad_loc is the derivative
    on the other side of the kink and differs."""
    shapes = [(8, 16), (4, 4)]
    rng = np.random.default_rng(11)
    g = _random_inputs(2, shapes, 2, 40, 4, 4, 8)
    p = R.lattice_coords(rng, shapes, 2, 40, 4, 4)
    p = np.floor(p)
    g["loc"] = (p + 0.5) / g["shapes"][None, None, None, :, None, ::-1]
    assert np.array_equal(R.pixel_coords(g["loc"], shapes), p)
    lo, mid, hi = _both(g, -2e-5), _both(g, 0.0), _both(g, 2e-5)
    y0l, x0l, ins = R.cells(g["loc"], shapes, -2e-5)
    y0h, x0h, _ = R.cells(g["loc"], shapes, 2e-5)
    assert ins.any() and (y0l[ins] == y0h[ins] - 1).all() and (x0l[ins] == x0h[ins] - 1).all()
    for i, name in ((0, "out"), (1, "grad_value"), (3, "grad_attn")):
        np.testing.assert_allclose(lo[i], hi[i], rtol=0, atol=1e-12, err_msg=name)
        assert np.abs(hi[i]).max() > 0.1, name
    for a, b in zip(mid, hi):                                             # floor() itself is the high side at an exact integer
        assert np.array_equal(a, b)
    diff = np.abs(lo[2] - hi[2])
    assert diff.max() > 0.1 and (diff[ins] > 1e-6).mean() > 0.5


def test_samples_failing_the_inside_test_contribute_nothing():
    """NaN, infinite and absurd coordinates fail the test of .cuh:293 like any outside sample: the result is that of the same
    inputs with those samples' weight set to 0, finite everywhere."""
    shapes = [(6, 4), (3, 2)]
    g = _random_inputs(3, shapes, 2, 7, 8, 4, 32)
    bad = [(0, 0, 0, 0, 0, 0, np.nan), (0, 1, 2, 1, 3, 1, np.inf), (1, 6, 7, 0, 2, 0, -np.inf), (1, 3, 4, 1, 0, 1, 3e38),
           (0, 5, 1, 0, 1, 0, -3e38), (1, 0, 0, 1, 1, 1, 1e30)]
    clean = {k: v.copy() for k, v in g.items()}
    for n, q, m, l, pt, ax, v in bad:
        g["loc"][n, q, m, l, pt, ax] = v
        clean["loc"][n, q, m, l, pt] = 0.5
        clean["attn"][n, q, m, l, pt] = 0
    want_all = _both(clean)
    for n, q, m, l, pt, ax, v in bad:
        assert want_all[3][n, q, m, l, pt] != 0
        want_all[3][n, q, m, l, pt] = 0          # the stand-in sample at (0.5, 0.5) has a weight gradient, the skipped one has none
    for got, want, name in zip(_both(g), want_all, ("out", "grad_value", "grad_loc", "grad_attn")):
        assert np.isfinite(got).all(), name
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, err_msg=name)
