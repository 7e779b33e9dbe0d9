"""The class count of the DeepLab half, without a device: the fused-heads layout, the constructor's range, and the argument
checks of the two OOD-score-tail entry points (they return before any HIP call)."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib
    return _lib


def formula(C):
    """The issue's layout, written out: q = 4*ceil(C/4), Kh = 16*ceil(2q/16)."""
    q = 4 * -(-C // 4)
    return q, 16 * -(-2 * q // 16)


def test_heads_layout_at_19_is_todays_buffer():
    from multishiftseg_amd.deepv3 import heads_layout
    assert heads_layout(19) == (20, 48)


@pytest.mark.parametrize("C", [1, 2, 4, 5, 12, 16, 17, 19, 32, 33, 100])
def test_heads_layout_follows_the_formula(C):
    from multishiftseg_amd.deepv3 import heads_layout
    q, Kh = heads_layout(C)
    assert (q, Kh) == formula(C)
    assert q % 4 == 0 and Kh % 16 == 0
    final6, ood = set(range(0, C)), set(range(q, q + C))
    assert not final6 & ood                      # rows never overlap
    assert max(ood) < Kh                         # and both heads fit
    expected = {1: (4, 16), 2: (4, 16), 4: (4, 16), 5: (8, 16), 12: (12, 32), 16: (16, 32), 17: (20, 48), 19: (20, 48),
                32: (32, 64), 33: (36, 80), 100: (100, 208)}
    assert (q, Kh) == expected[C]


@pytest.mark.parametrize("C", [2, 12, 33, 100])
def test_constructor_accepts_the_class_count(C):
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    model = DeepWV3Plus(C)
    assert model.num_classes == C
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v) for k, v in synth.deepwv3plus_param_shapes(num_classes=C).items()}
    assert got == want
    assert got["final.6.weight"] == got["ood_head.weight"] == (C, 256, 1, 1)
    model.uncertainty_func_init()
    assert torch.equal(model.ood_head.weight, model.final[6].weight)


@pytest.mark.parametrize("C", [1, 101, 0, -3])
def test_constructor_refuses_a_count_outside_the_range(C):
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    with pytest.raises(ValueError, match=r"2\.\.100"):
        DeepWV3Plus(C)


def test_entry_points_check_the_class_count_before_any_launch(lib):
    """Raw calls with a NULL stream and a pointer nothing dereferences: every case returns before its launch. Order of the checks:
    the class range, the NULL-pointer combinations, then the empty problem."""
    OK, BAD, UNSUPPORTED = 0, lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    handle = lib.load()
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)

    def fwd(C, N=2, dec2=X, dec1=X, score=X, logit=X, label=X):
        return handle.mss_ood_score_f32(dec2, 48, dec1, 48, N, 13, 18, C, 26, 36, score, logit, label, None)

    def bwd(C, N=2, dec2=X, ddec2=X):
        return handle.mss_ood_score_bwd_f32(dec2, 48, X, X, N, 13, 18, C, 26, 36, ddec2, 48, X, 48, None)

    for C in (0, 101, -1):
        assert fwd(C) == UNSUPPORTED and bwd(C) == UNSUPPORTED, C
        assert fwd(C, N=0) == UNSUPPORTED and bwd(C, N=0) == UNSUPPORTED, C        # the range comes first
        assert fwd(C, dec2=None) == UNSUPPORTED and bwd(C, dec2=None) == UNSUPPORTED, C
    for C in (1, 12, 19, 33, 100):
        assert fwd(C, N=0) == OK and bwd(C, N=0) == OK, C                          # nothing launched
        assert fwd(C, dec2=None) == BAD, C                                         # a score wants dec2
        assert fwd(C, dec1=None) == BAD, C                                         # logits / labels want dec1
        assert fwd(C, dec1=None, score=None, logit=None) == BAD, C                 # the label alone wants it too
        assert fwd(C, N=0, dec2=None) == BAD and fwd(C, N=0, dec1=None) == BAD, C  # the pointers come before the empty problem
        assert fwd(C, N=0, dec2=None, score=None) == OK, C                         # no score: dec2 may be NULL
        assert fwd(C, N=0, dec1=None, logit=None, label=None) == OK, C
        assert bwd(C, dec2=None) == BAD and bwd(C, N=0, dec2=None) == BAD, C
        assert bwd(C, N=0, dec2=None, ddec2=None) == OK, C
