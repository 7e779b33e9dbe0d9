"""The route of the DeepLab head's ASPP block (multishiftseg_amd/aspp_plan.py) without a GPU: a table of steps -- map size, mode,
switches, GEMM route, tile hook, X' budget -- with the plan fields each must get. The expected fields were worked out from the head
forward as it stood before the plan existed (every decision it took in between its launches); tests/test_gpu_aspp_head_traces.py
holds the launches themselves against that commit on the GPU. A new ASPP route adds a field to AsppPlan and a row here."""
import ctypes

import pytest

from multishiftseg_amd import _lib, aspp_plan as ap

RATES = (12, 24, 36)
W3 = [(256, 4096, 3, 3)] * 3
SWITCHES = ("MSS_ASPP_COMPOSE", "MSS_ASPP_DROPOUT_COMPACT", "MSS_WINO_ASPP3", "MSS_WINO_PAIR", "MSS_WINOGRAD", "MSS_WINO_TILE",
            "MSS_WINO_MAX_TILE")


def step_plan(N, H, W, mode, route="native", hook=False, budget=ap.XT_BUDGET_BYTES):
    """The plan of a DeepWV3Plus step on an N x H x W x 4096 trunk output, with the facts as deepv3 states them: the trunk hands over
    its factors where DeepWV3Plus._aspp_compose_gate says so (compose_wanted and tiles), a Dropout2d mask with its per-sample affine
    comes with them in train mode, and a stage-2 step (`train`) keeps for a backward that wants all three weight gradients."""
    train, keep = mode == "train", mode in ("train", "stage1")
    factored = ap.compose_wanted(hook) and ap.tiles(H, W, 4096, RATES, W3, hook) is not None
    facts = dict(factored=True, c0=2048, aff_dims=(1, 2 if mode != "eval" else 1), mask=mode != "eval") if factored else {}
    return ap.plan(N, H, W, 4096, W3, RATES, keep=keep, wgrad=(train,) * 3, route=route, hook=hook, budget=budget, **facts)


BIG = ap.XT_BUDGET_BYTES
# fields every row states: tiles, pair_tile, single_read, dropped, dropped_separate, gap_from_kernel, materialise, keep_xt (one value
# for the three branches), max_bytes
DROPPED = dict(pair_tile=0, single_read=True, dropped=True, dropped_separate=False, gap_from_kernel=True, materialise=False,
               keep_xt=True, max_bytes=None)
COMPOSED = dict(DROPPED, dropped=False)                                               # the two-source kernel, dense products
SEPARATE = dict(DROPPED, single_read=False, dropped_separate=True)
DENSE = dict(COMPOSED, gap_from_kernel=False)                                         # the trunk's map as an Act, one kernel
ALONE = dict(DENSE, single_read=False)                                                # each branch transforms for itself
T444, T664 = (4, 4, 4), (6, 6, 4)
CASES = [
    # ---- stage-2 steps: 2 x 74 x 75 (592 x 600 images), 2 x 128 x 256 (1024 x 2048), 4 x 88 x 88 (700 x 700) -----------------------
    ("s2_74x75", (2, 74, 75, "train"), {}, {}, dict(DROPPED, tiles=T444)),
    ("s2_128x256", (2, 128, 256, "train"), {}, {}, dict(DROPPED, tiles=T664)),
    ("s2_88x88", (4, 88, 88, "train"), {}, {}, dict(DROPPED, tiles=T444)),
    ("s2_74x75_dense", (2, 74, 75, "train"), {"MSS_ASPP_DROPOUT_COMPACT": "0"}, {}, dict(COMPOSED, tiles=T444)),
    ("s2_128x256_dense", (2, 128, 256, "train"), {"MSS_ASPP_DROPOUT_COMPACT": "0"}, {}, dict(COMPOSED, tiles=T664)),
    ("s2_74x75_present", (2, 74, 75, "train"), {"MSS_ASPP_COMPOSE": "0"}, {}, dict(DENSE, tiles=T444)),
    ("s2_88x88_present", (4, 88, 88, "train"), {"MSS_ASPP_COMPOSE": "0"}, {}, dict(DENSE, tiles=T444)),
    ("s2_74x75_separate", (2, 74, 75, "train"), {"MSS_WINO_ASPP3": "0"}, {}, dict(SEPARATE, tiles=T444)),
    ("s2_128x256_separate", (2, 128, 256, "train"), {"MSS_WINO_ASPP3": "0"}, {}, dict(SEPARATE, tiles=T664)),
    # MSS_WINO_ASPP3=0 without the dropped products: the kernel's sums-only mode, w materialised, each branch transforms it
    ("s2_74x75_separate_dense", (2, 74, 75, "train"), {"MSS_WINO_ASPP3": "0", "MSS_ASPP_DROPOUT_COMPACT": "0"}, {},
     dict(COMPOSED, tiles=T444, single_read=False, materialise=True)),
    ("s2_74x75_separate_present", (2, 74, 75, "train"), {"MSS_WINO_ASPP3": "0", "MSS_ASPP_COMPOSE": "0"}, {}, dict(ALONE, tiles=T444)),
    # MSS_WINOGRAD=0: no composed route, no tiles; X' is "kept" by layers that then make none (kernels.conv3x3 leaves the dict empty)
    ("s2_74x75_direct", (2, 74, 75, "train"), {"MSS_WINOGRAD": "0"}, {}, dict(ALONE, tiles=None)),
    ("s2_74x75_pair_off", (2, 74, 75, "train"), {"MSS_WINO_PAIR": "0"}, {}, dict(DROPPED, tiles=T444)),       # (no pair in a kept step anyway)
    ("s2_74x75_bf16x3", (2, 74, 75, "train"), {}, dict(route="bf16x3"), dict(COMPOSED, tiles=T444)),          # no dropped products there
    ("s2_128x256_bf16x3", (2, 128, 256, "train"), {}, dict(route="bf16x3"), dict(COMPOSED, tiles=T664)),
    ("s2_74x75_hook", (2, 74, 75, "train"), {}, dict(hook=True), dict(ALONE, tiles=None)),                    # attribution runs: the present path
    # a tile edge of 2 at dilation 36: no single-read kernel and no composed route
    ("s2_37x38", (2, 37, 38, "train"), {}, {}, dict(ALONE, tiles=None)),
    ("s2_37x38_separate", (2, 37, 38, "train"), {"MSS_WINO_ASPP3": "0"}, {}, dict(ALONE, tiles=None)),
    # over the X' budget (2 x 74 x 75: 2.89 GB of X'; the only test of this branch's decision): nothing is kept, X' is not taken
    # from the kernel, which still leaves GAP(w); w is materialised for the branches and their weight gradients
    ("s2_74x75_over", (2, 74, 75, "train"), {}, dict(budget=1 << 30),
     dict(COMPOSED, tiles=T444, single_read=False, materialise=True, keep_xt=False, max_bytes=1 << 30)),
    ("s2_74x75_over_present", (2, 74, 75, "train"), {"MSS_ASPP_COMPOSE": "0"}, dict(budget=1 << 30),
     dict(ALONE, tiles=T444, keep_xt=False, max_bytes=1 << 30)),
    # 2000 images: 36 x 2000 (position, image) batch entries > 65535 (and offsets past 32 bits): the dense products
    ("s2_2000x74x75", (2000, 74, 75, "train"), {}, dict(budget=1 << 50), dict(COMPOSED, tiles=T444)),
    # ---- a stage-1 step: the backward wants no ASPP weight gradient, so no X' is kept; the dropped products run all the same ------
    ("s1_74x75", (2, 74, 75, "stage1"), {}, {}, dict(DROPPED, tiles=T444, keep_xt=False)),
    # ---- the one-image eval forward: nothing kept, X' under the budget, dilations 12 and 24 in one product launch -----------------
    ("eval_74x75", (1, 74, 75, "eval"), {}, {}, dict(COMPOSED, tiles=T444, pair_tile=4, keep_xt=False, max_bytes=BIG)),
    ("eval_128x256", (1, 128, 256, "eval"), {}, {}, dict(COMPOSED, tiles=T664, pair_tile=6, keep_xt=False, max_bytes=BIG)),
    ("eval_74x75_no_pair", (1, 74, 75, "eval"), {"MSS_WINO_PAIR": "0"}, {}, dict(COMPOSED, tiles=T444, keep_xt=False, max_bytes=BIG)),
    ("eval_74x75_present", (1, 74, 75, "eval"), {"MSS_ASPP_COMPOSE": "0"}, {}, dict(DENSE, tiles=T444, pair_tile=4, keep_xt=False, max_bytes=BIG)),
    # MSS_WINO_ASPP3=0 with the pair: the pair transforms the materialised map itself
    ("eval_74x75_separate", (1, 74, 75, "eval"), {"MSS_WINO_ASPP3": "0"}, {},
     dict(COMPOSED, tiles=T444, pair_tile=4, single_read=False, materialise=True, keep_xt=False, max_bytes=BIG)),
    ("eval_74x75_bf16x3", (1, 74, 75, "eval"), {}, dict(route="bf16x3"), dict(COMPOSED, tiles=T444, pair_tile=4, keep_xt=False, max_bytes=BIG)),
    ("eval_2x74x75", (2, 74, 75, "eval"), {}, {}, dict(COMPOSED, tiles=T444, keep_xt=False, max_bytes=BIG)),  # two images fill the rounds: no pair
    ("eval_74x75_direct", (1, 74, 75, "eval"), {"MSS_WINOGRAD": "0"}, {}, dict(ALONE, tiles=None, keep_xt=False, max_bytes=BIG)),
    ("eval_74x75_hook", (1, 74, 75, "eval"), {}, dict(hook=True), dict(ALONE, tiles=None, keep_xt=False, max_bytes=BIG)),
    ("eval_37x38", (1, 37, 38, "eval"), {}, {}, dict(ALONE, tiles=None, keep_xt=False, max_bytes=BIG)),
    ("eval_74x75_over", (1, 74, 75, "eval"), {}, dict(budget=1 << 30),
     dict(COMPOSED, tiles=T444, pair_tile=4, single_read=False, materialise=True, keep_xt=False, max_bytes=1 << 30)),
]


@pytest.mark.parametrize("name,step,env,facts,want", CASES, ids=[c[0] for c in CASES])
def test_plan_of_a_step(monkeypatch, name, step, env, facts, want):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N, H, W, mode = step
    p = step_plan(N, H, W, mode, **facts)
    got = {k: getattr(p, k) for k in want}
    assert got == dict(want, tiles=want["tiles"], keep_xt=(want["keep_xt"],) * 3), (name, p)
    # tile counts and positions go with the tiles
    if p.tiles is None:
        assert p.Ts is None and p.Ps is None
    else:
        assert p.Ps == tuple((t + 2) ** 2 for t in p.tiles)
        assert p.Ts == tuple(_lib.value("mss_wino_num_tiles", N, H, W, r, t) for r, t in zip(RATES, p.tiles))
    # what no plan may say at once
    assert not (p.dropped_separate and (p.single_read or not p.dropped))
    assert not (p.dropped and (p.pair_tile or p.materialise or not p.gap_from_kernel))
    assert p.tiles is not None or not (p.single_read or p.dropped or p.gap_from_kernel)
    with pytest.raises(Exception):
        p.dropped = True                                                              # immutable


def test_the_tiles_the_gpu_tests_assert():
    assert [ap.wino_tile(74, 75, r) for r in RATES] == [4, 4, 4]
    assert [ap.wino_tile(128, 256, r) for r in RATES] == [6, 6, 4]
    assert [ap.wino_tile(88, 88, r) for r in RATES] == [4, 4, 4]
    assert ap.wino_tile(37, 38, 36) == 2


def test_per_image_products_gate():
    """The per-image products' gate, stated once: 32-bit operand offsets (4 P T C bytes), whole images (T % N) and 65535 batch
    entries (P N)."""
    assert ap.per_image_products_fit(2, 4096, (36, 36, 36), (1152, 1152, 2592))
    assert not ap.per_image_products_fit(2, 4096, (36, 36, 36), (1152, 1153, 2592))                 # T % N
    assert ap.per_image_products_fit(1820, 128, (36,) * 3, (1820,) * 3)                             # 36 x 1820 = 65520 entries
    assert not ap.per_image_products_fit(1821, 128, (36,) * 3, (1821,) * 3)                         # 36 x 1821 = 65556
    assert ap.per_image_products_fit(2, 4096, (64,) * 3, (4094,) * 3)                               # 4 x 64 x 4094 x 4096 < 2^32 - 1
    assert not ap.per_image_products_fit(2, 4096, (64,) * 3, (4096,) * 3)                           # = 2^32


def _supported(N, H, W, C, d, tiles, two_source):
    return _lib.value("mss_wino_aspp3_supported", N, H, W, C, d, (ctypes.c_int * 3)(*tiles), two_source)


def test_supported_query_refuses_what_the_launchers_refuse():
    # a 512 x 1024 map at d = 12: base sub-grids of Hs x Ws = 43 x 86 pixels. The kernel stages (Hs + 1) rows of at least Ws columns
    # of at least 32 + 4 floats: 44 x 86 x 36 x 4 = 544 896 bytes > 80 KiB = 81 920, whatever the tiles
    assert 44 * 86 * 36 * 4 > 80 * 1024
    for two in (0, 1):
        assert _supported(1, 512, 1024, 8, 12, (6, 6, 6), two) == 0
        assert _supported(2, 512, 1024, 4096, 12, (4, 4, 4), two) == 0
        assert _supported(2, 128, 256, 4096, 12, (6, 6, 4), two) == 1                # the benchmark's map: 11 x 22 sub-grids
        assert _supported(2, 74, 75, 4096, 12, (2, 4, 4), two) == 0                  # a tile edge of 2
        assert _supported(2, 74, 75, 4096, 12, (4, 4, 8), two) == 0
        assert _supported(2, 74, 75, 4096, 0, (4, 4, 4), two) == 0                   # d < 1: the launchers' bad argument, not a shape they take
    assert _supported(1 << 20, 24, 24, 4096, 12, (4, 4, 4), 0) == 0                  # 2^20 x 144 x 64 channel chunks >= 2^31 workgroups
    assert _supported(1, 24, 24, (1 << 24) + 4, 12, (4, 4, 4), 1) == 0               # C0 + C1 > 2^24 (two-source forms only)
    assert _supported(1, 24, 24, (1 << 24) + 4, 12, (4, 4, 4), 0) == 1


def test_supported_query_takes_every_shape_of_the_kernel_tests():
    from test_gpu_aspp_compose_kernels import CASES as SRC2_CASES
    from test_gpu_aspp_dropped_kernels import TRANSFORM_CASES
    assert len(SRC2_CASES) == 4 and len(TRANSFORM_CASES) == 3
    for n, H, W, C0, C1, d, tiles in SRC2_CASES + TRANSFORM_CASES:
        assert _supported(n, H, W, C0 + C1, d, tiles, 1) == 1, (n, H, W, C0, C1, d, tiles)
        assert _supported(n, H, W, C0 + C1, d, tiles, 0) == 1
