"""What the GPU tests of the neighbour rows share (tests/test_neighbours_gpu.py, tests/test_neighbours_limits_gpu.py, tests/test_gpu_poison.py): the device's outputs
against tests/neighbour_oracle.py, the integers equal and the doubles bit for bit.  numpy only."""
import numpy as np


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])


def assert_equals_oracle(got, ref, what="", without=()):
    """``without``: outputs the call was made without (`neighbours` is optional), which ``got`` then must not hold."""
    assert not set(without) & set(got), (what, without)
    for k in ("n_near", "n_rows", "neighbours"):
        if k in without:
            continue
        assert got[k].shape == ref[k].shape, (what, k)
        bad = np.nonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[0]
        assert not len(bad), (what, k, bad[:8], got[k][bad[:8]], ref[k][bad[:8]])
    bad = [b for b in range(len(ref["c_eta"])) if not bits_equal(got["c_eta"][b], ref["c_eta"][b])]
    assert not bad, (what, "c_eta", bad[:8], got["c_eta"][bad[0]], ref["c_eta"][bad[0]])
