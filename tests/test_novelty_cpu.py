"""The novelty rule on the host: rmcv_icon_sad and rmcv_harvest_novel_host -- rmcv_amd/csrc/device_novelty.h compiled for the
host -- equal tests/novelty_ref.py, the rule restated in numpy from the header's text, on every seeded call of tests/novelty_cases.py; the
cases are what they claim (the census); the host entry points refuse what the header says they refuse.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import novelty_cases as K
import novelty_ref as R
from rmcv_amd import HARVEST_RING_MAX, HARVEST_SKIP, ICON_SAD_MAX, RmcvError, harvest_novel, icon_sad
from rmcv_amd.abi import lib, ptr


def test_constants():
    assert (ICON_SAD_MAX, HARVEST_RING_MAX, HARVEST_SKIP) == (R.SAD_MAX, R.RING_MAX, R.SKIP) == (306000, 8, -2**31)


def test_census():
    seen = K.census()
    assert seen["kept"] and seen["near"]


def test_icon_sad_equals_the_restatement():
    b = K.base_row(1)
    zeros, full = np.zeros(R.ROW, np.uint8), np.full(R.ROW, 255, np.uint8)
    assert icon_sad(zeros, full) == icon_sad(full, zeros) == 306000 and icon_sad(b, b) == 0
    for at in (0, 1023, 1024, 1199):
        assert icon_sad(b, K.bump(b, at)) == icon_sad(K.bump(b, at), b) == 1
    r = np.random.RandomState(7)
    for _ in range(32):
        x, y = r.randint(0, 256, (2, R.ROW)).astype(np.uint8)
        assert icon_sad(x, y) == R.sad(x, y)
    assert icon_sad(b, K.tail_diff(b, 5001)) == 5001
    with pytest.raises(RmcvError):
        icon_sad(b[:100], b)


@pytest.mark.parametrize("case", K.cases(), ids=[c.name for c in K.cases()])
def test_host_rule_equals_the_restatement(case):
    e = K.expected(case)
    n_streams = max(len(a[1]) for a in case.appends)
    rings, pushed, near = np.zeros((n_streams, case.R, R.ROW), np.uint8), np.zeros(n_streams, np.int64), 0
    for (rows, n, lb, _), keep, dist, after in zip(case.appends, e["keeps"], e["sads"], e["states"]):
        s = len(n)
        got_keep, got_sad, got_near, rg, pu = harvest_novel(rows, n, lb, case.R, case.T, rings[:s], pushed[:s])
        near += got_near
        rings[:s], pushed[:s] = rg, pu
        assert np.array_equal(got_keep.astype(bool), keep)
        assert np.array_equal(got_sad.astype(np.int64), dist)
        assert near == after.near and np.array_equal(rings, after.rings[:n_streams]) and np.array_equal(pushed, after.pushed[:n_streams])
    assert not e["rings"][n_streams:].any() and not e["pushed"][n_streams:].any()


def test_host_refusals():
    rows, n, lb = np.zeros((2, R.ROW), np.uint8), np.array([2], np.int32), np.array([1], np.int32)
    rings, pushed, keep = np.zeros((1, 8, R.ROW), np.uint8), np.zeros(1, np.int64), np.zeros(2, np.uint8)
    call = lib().rmcv_harvest_novel_host
    ok = lambda **kw: call(*[kw.get(k, v) for k, v in (("rows", ptr(rows)), ("n", ptr(n)), ("lb", ptr(lb)), ("s", 1), ("R", 2), ("T", 0), ("rings", ptr(rings)),
                                                        ("pushed", ptr(pushed)), ("keep", ptr(keep)), ("sad", None), ("near", None))])
    assert ok() == 0 and list(keep) == [1, 0] and pushed[0] == 1                # min_sad_out and near_out are nullable
    for bad in ({"R": -1}, {"R": HARVEST_RING_MAX + 1}, {"T": -1}, {"T": ICON_SAD_MAX + 1}, {"s": -1}, {"rows": None}, {"n": None}, {"lb": None}, {"rings": None},
                {"pushed": None}, {"keep": None}, {"n": ptr(np.array([-1], np.int32))}):
        assert ok(**bad) != 0, bad
    assert pushed[0] == 1                                                        # nothing was touched by any of them
    assert ok(R=0, rings=None, pushed=None) == 0 and list(keep) == [1, 1]        # depth 0 needs no state
    assert ok(R=HARVEST_RING_MAX, T=ICON_SAD_MAX) == 0
    assert lib().rmcv_icon_sad(None, ptr(rows)) < 0
    near = C.c_int64(-1)
    assert ok(near=C.byref(near)) == 0 and near.value == 2                       # both rows are zeros, like the ring's row: near
    with pytest.raises(RmcvError):
        harvest_novel(rows, [3], [1], 2, 0)                                      # counts that do not add up to the rows
