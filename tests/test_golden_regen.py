"""The comparator behind tools/check_golden.py, which re-runs tools/gen_golden.py against the reference project into a temporary
directory and compares every array with the committed fixtures bit for bit (VERDICT r05 missing #3). The
re-generation itself needs the reference's sources, which are not part of this repository; it is run by hand with
`python tools/check_golden.py` (`--all` / by name for the minutes-long fixtures)."""
import os
import sys

from conftest import ROOT


def test_check_golden_detects_a_changed_array(tmp_path):
    """The comparator itself: a one-bit change, a renamed array and an uncommitted fixture are all reported."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_golden
    g = np.load(os.path.join(check_golden.GOLDEN, "msda_testpy_f32.npz"))
    arrays = {k: g[k].copy() for k in g.files}
    np.savez(tmp_path / "msda_testpy_f32.npz", **arrays)
    assert check_golden.compare(str(tmp_path)) == (["msda_testpy_f32.npz"], [])
    k0 = next(k for k in arrays if arrays[k].dtype == np.float32 and arrays[k].size)
    flipped = arrays[k0].copy()
    flipped.view(np.uint32).reshape(-1)[0] ^= 1
    np.savez(tmp_path / "msda_testpy_f32.npz", **dict(arrays, **{k0: flipped}))
    assert check_golden.compare(str(tmp_path))[1] == [("msda_testpy_f32.npz", k0, "bytes differ")]
    np.savez(tmp_path / "msda_testpy_f32.npz", **{("x" + k if k == k0 else k): v for k, v in arrays.items()})
    assert "array names differ" in check_golden.compare(str(tmp_path))[1][0][2]
    np.savez(tmp_path / "never_committed.npz", a=np.zeros(1))
    assert ("never_committed.npz", "*", "not committed") in check_golden.compare(str(tmp_path))[1]
