"""CPU: the numpy restatement of the reference's target build on a hand-written map, the argument checks of
mss_m2f_targets_from_labels (they return before any HIP call), and prepare_targets failing loudly without a device."""
import ctypes

import numpy as np
import pytest

import ref_m2f_targets as ref


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from multishiftseg_amd import _lib
    return _lib


def test_restatement_on_a_hand_written_map():
    """2 x 3 x 4, label_threshold 100, ignore 255, padded to 4 x 4 (divisibility 4). 99 is the last class, 100 is neither a
    class nor OOD, 101 and 254 are OOD, 255 is ignored."""
    sem = np.array([[[0, 0, 99, 100],
                     [101, 254, 255, 7],
                     [7, 7, 0, 99]],
                    [[255, 255, 255, 255],
                     [255, 100, 255, 255],
                     [255, 255, 255, 254]]], dtype=np.int64)
    t = ref.prepare_targets(sem, size_divisibility=4)
    assert [x["labels"].tolist() for x in t] == [[0, 7, 99], []]
    assert all(x["labels"].dtype == np.int64 and x["masks"].dtype == bool and x["ood_mask"].dtype == bool for x in t)
    assert t[0]["masks"].shape == (3, 4, 4) and t[1]["masks"].shape == (0, 4, 4) and t[1]["ood_mask"].shape == (4, 4)
    want0 = np.array([[[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]],
                      [[0, 0, 0, 0], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0]],
                      [[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]], dtype=bool)
    assert np.array_equal(t[0]["masks"], want0)
    assert np.array_equal(t[0]["ood_mask"], np.array([[0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=bool))
    assert np.array_equal(t[1]["ood_mask"], np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], dtype=bool))
    # no padding with divisibility 0 / 1; the uint8 map gives the same answer
    for d in (0, 1):
        u = ref.prepare_targets(sem.astype(np.uint8), size_divisibility=d)
        assert np.array_equal(u[0]["masks"], want0[:, :3]) and u[0]["labels"].tolist() == [0, 7, 99]
    # the documented deviation: the reference keeps a negative value as a class, the product's restatement drops it
    neg = sem.copy()
    neg[0, 0, 0] = -3
    assert ref.prepare_targets(neg, drop_negative=False)[0]["labels"].tolist() == [-3, 0, 7, 99]
    got = ref.prepare_targets(neg)[0]
    assert got["labels"].tolist() == [0, 7, 99] and not got["ood_mask"][0, 0] and not got["masks"][:, 0, 0].any()


def test_entry_point_validates_arguments_before_any_launch(lib):
    """Raw calls with a NULL stream and pointers nothing dereferences: every case returns before its first HIP call.
    Base case: int64 maps 2 x 5 x 7 padded to 8 x 8, label_threshold 100, 3 targets."""
    BAD, UNSUPPORTED = lib.MSS_ERR_BAD_ARG, lib.MSS_ERR_UNSUPPORTED
    handle = lib.load()
    buf = (ctypes.c_char * 64)()
    X = ctypes.addressof(buf)

    def run(phase, sem=X, sem_bytes=8, B=2, H=5, W=7, Hp=8, Wp=8, thr=100, present=X, tstart=X, labels=X, rank=X, total_t=3, tmask=X, ood=X):
        return handle.mss_m2f_targets_from_labels(sem, sem_bytes, B, H, W, Hp, Wp, thr, 255, phase, present, tstart, labels, rank, total_t,
                                                  tmask, ood, None)
    both = {"thr=0": (dict(thr=0), UNSUPPORTED), "thr=129": (dict(thr=129), UNSUPPORTED), "sem_bytes=2": (dict(sem_bytes=2), UNSUPPORTED),
            "sem_bytes=0": (dict(sem_bytes=0), UNSUPPORTED), "B=0": (dict(B=0), BAD), "H=0": (dict(H=0), BAD), "W=0": (dict(W=0), BAD),
            "Hp<H": (dict(Hp=4), BAD), "Wp<W": (dict(Wp=6), BAD), "total_t<0": (dict(total_t=-1), BAD), "null sem": (dict(sem=None), BAD),
            "null tstart": (dict(tstart=None), BAD), "null rank": (dict(rank=None), BAD)}
    for phase in (0, 1):
        for name, (kw, want) in both.items():
            assert run(phase, **kw) == want, (phase, name)
    for phase in (-1, 2):
        assert run(phase) == BAD, phase
    assert run(0, present=None) == BAD and run(0, labels=None) == BAD
    assert run(1, ood=None) == BAD and run(1, tmask=None) == BAD
    assert run(1, tmask=None, ood=None, total_t=0) == BAD            # total_t == 0 frees tmask only: ood is still written


def test_prepare_targets_fails_loudly_without_gpu():
    """A label map on the host is refused, with or without a device in the machine: there is no CPU path to fall back to."""
    import torch
    from multishiftseg_amd import prepare_targets
    from multishiftseg_amd import kernels as K
    sem = torch.zeros((2, 4, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="CPU"):
        prepare_targets(sem)
    with pytest.raises(RuntimeError, match="CPU"):
        K.m2f_targets_count(sem)
    with pytest.raises(RuntimeError, match="CPU"):
        K.m2f_targets_fill(sem, torch.zeros(3, dtype=torch.int32), torch.zeros((2, 100), dtype=torch.int32), 0, (4, 4))
