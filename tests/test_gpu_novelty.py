"""The dataset harvest's novelty rings on the GPU (k_novelty.hip): rows, metadata, count, dropped, near, rings and pushed equal,
byte for byte, what tests/novelty_ref.py -- the rule restated from the text of device_novelty.h -- makes of the same candidates.  The
candidates of a batch are the rows of a second dataset with novelty off fed by the same appends (tests/test_gpu_harvest.py pins that path to
the oracle); seeded rows go through DeviceDataset.append_rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import novelty_cases as K
import novelty_ref as R
import raw_ref as RR
from rmcv_amd import (CAMP_BLUE, HARVEST_MISSES, HARVEST_RING_MAX, HARVEST_SKIP, ICON_SAD_MAX, STAGE_ALL, STAGE_IDENTITY, Context, DeviceDataset, Pipeline, RmcvError,
                      default_params, synth)
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu

LABELS = np.array([1, 2, HARVEST_SKIP, 3, 4, 5, 6, 0], np.int32)   # (the label table of tests/test_gpu_harvest.py: frame 2 is skipped)
META_KEYS = ("tag", "frame", "armour", "label", "identity", "win_x", "win_y")


@functools.lru_cache(maxsize=None)
def frames_of(w, h):
    f = np.stack([synth.frame(i, w, h, CAMP_BLUE, 0) for i in range(8)])
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def small():
    c = Context(device=0, max_frames=8, max_width=320, max_height=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide():
    c = Context(device=0, max_frames=264, max_width=200, max_height=136)
    yield c
    c.close()


def check_state(ds, state, streams=None):
    """near, rings and pushed of the dataset against a novelty_ref.State"""
    rings, pushed = ds.rings()
    n = len(pushed) if streams is None else streams
    assert ds.novelty["near"] == state.near
    assert np.array_equal(pushed[:n], state.pushed[:n]) and not pushed[n:].any()
    assert np.array_equal(rings[:n], state.rings[:n]) and not rings[n:].any()


class Mirror:
    """what a dataset with novelty on must hold, from the candidates a dataset with novelty off (`off`) received in the same appends"""

    def __init__(self, streams, depth, T, capacity):
        self.state, self.T, self.capacity = R.State(streams, depth), T, capacity
        self.rows, self.meta, self.count, self.dropped, self.sads, self.keeps, self.mosts = [], [], 0, 0, [], [], []

    def append(self, rows, meta):
        """rows, meta: one append's slice of `off`, in slot order (= frame-major, armour-major)"""
        streams = len(self.state.pushed)
        n_rows = np.bincount(meta["frame"], minlength=streams)
        assert (np.diff(meta["frame"]) >= 0).all()
        keep, dist, most = R.append(self.state, self.T, rows, n_rows, np.zeros(streams, np.int64))
        kept = np.flatnonzero(keep)
        fits = kept[:max(0, self.capacity - self.count)]
        self.rows.append(rows[fits]), self.meta.append(meta[fits])
        self.dropped += len(kept) - len(fits)
        self.count += len(fits)
        self.sads.append(dist), self.keeps.append(keep), self.mosts.append(most)
        return keep

    def check(self, ds):
        assert (ds.count, ds.dropped) == (self.count, self.dropped)
        assert np.array_equal(ds.rows(), np.concatenate(self.rows)) and ds.meta().tobytes() == np.concatenate(self.meta).tobytes()
        check_state(ds, self.state)


def smallest_kept_distance(appends, streams, depth):
    """t: the smallest distance among the candidates the restatement keeps at T = 0 -- at T = t that decision flips, at T = t - 1 none does"""
    m = Mirror(streams, depth, 0, 1 << 30)
    for rows, meta in appends:
        m.append(rows, meta)
    d = np.concatenate(m.sads)[np.concatenate(m.keeps)]
    d = d[d != R.NO_SAD]
    assert len(d) and d.min() > 0
    return int(d.min())


# ---------------------------------------------------------------- 1. seeded calls through append_rows
@pytest.mark.parametrize("case", K.cases(), ids=[c.name for c in K.cases()])
def test_seeded_calls_equal_the_host_rule(request, case):
    c = request.getfixturevalue("small" if case.cap == 8 else "wide")
    e = K.expected(case)
    ds = DeviceDataset(c, min(case.capacity, sum(len(a[0]) for a in case.appends) + 1))
    ds.set_novelty(case.R, case.T)
    for (rows, n, lb, tag), count, state in zip(case.appends, e["counts"], e["states"]):
        ds.append_rows(rows, n, lb, tag)
        assert ds.count == count
        if case.R:
            check_state(ds, state)
    assert (ds.count, ds.dropped) == (e["count"], e["dropped"]) and ds.novelty == {"ring_rows": case.R, "max_sad": case.T, "near": e["near"]}
    assert np.array_equal(ds.rows(), e["rows"])
    m = ds.meta()
    assert [tuple(int(m[k][i]) for k in META_KEYS) for i in range(len(m))] == e["meta"] and not m["icon"].any()
    ds.close()


# ---------------------------------------------------------------- 2. frames: A, A rolled by one stream, A again
def harvest_all(c, batches, datasets, flags=0, stages=STAGE_ALL, labels=LABELS):
    """each batch uploaded and run once, then appended to every dataset; -> the count of datasets[0] behind each append"""
    ends = []
    for tag, frames in enumerate(batches):
        c.upload(frames)
        c.run(default_params(), stages)
        for ds in datasets:
            c.harvest(ds, labels, flags, tag=tag)
        ends.append(datasets[0].count)
    return ends


def slices(off, ends):
    rows, meta = off.rows(), off.meta()
    return [(rows[a:b], meta[a:b]) for a, b in zip([0] + ends[:-1], ends)]


@pytest.mark.parametrize("w,h", [(320, 256), (200, 136)], ids=["320x256", "200x136"])
def test_three_appends_of_frames(small, w, h):
    c, A = small, frames_of(w, h)
    batches = [A, np.roll(A, 1, axis=0), A]
    off = DeviceDataset(c, 512)
    cands = slices(off, harvest_all(c, batches, [off]))
    assert off.dropped == 0 and all(len(r) >= 3 for r, _ in cands)
    settings = [(depth, T) for depth in (1, 8) for t in [smallest_kept_distance(cands, 8, depth)] for T in (0, t - 1, t, ICON_SAD_MAX)]
    datasets, mirrors = [], []
    for depth, T in settings:
        ds = DeviceDataset(c, 512)
        ds.set_novelty(depth, T)
        datasets.append(ds), mirrors.append(Mirror(8, depth, T, 512))
    harvest_all(c, batches, datasets)
    for m, ds in zip(mirrors, datasets):
        for rows, meta in cands:
            m.append(rows, meta)
        m.check(ds)
        ds.close()
    by = dict(zip(settings, mirrors))
    kept = {k: [int(x.sum()) for x in m.keeps] for k, m in by.items()}
    near = {k: [len(x) - int(x.sum()) for x in m.keeps] for k, m in by.items()}
    assert any(a > 0 and b > 0 for a, b in zip(kept[(8, 0)], near[(8, 0)]))              # kept and near in one append
    assert max(by[(1, 0)].mosts) > 1 and (w != 320 or max(by[(8, 0)].mosts) > 8)             # a ring wraps inside an append
    assert kept[(1, 0)][2] != kept[(8, 0)][2]                                                # depth 1 has forgotten what depth 8 remembers
    for depth, t in ((1, settings[2][1]), (8, settings[6][1])):                               # exactly at t a decision flips, and none below it
        same = lambda T: all(np.array_equal(x, y) for x, y in zip(by[(depth, T)].keeps, by[(depth, 0)].keeps))
        assert same(t - 1) and not same(t)
    assert sum(kept[(8, ICON_SAD_MAX)]) <= 7 and kept[(8, ICON_SAD_MAX)][2] == 0             # at most one row per live stream: nothing is ever new again
    assert w != 320 or kept[(8, ICON_SAD_MAX)] == [7, 0, 0]
    off.close()


# ---------------------------------------------------------------- 3. every pixel accessor, and misses
def one_append(c, upload, flags=0, stages=STAGE_ALL, windows=None, depth=2, labels=LABELS):
    """one batch appended to a dataset with novelty off, then -- at a threshold that makes the nearest kept candidate near -- to one with it on"""
    c.upload(upload)
    if windows is not None:
        c.set_windows(*windows)
    c.run(default_params(), stages)
    off = DeviceDataset(c, 128)
    c.harvest(off, labels, flags, tag=3)
    cands = slices(off, [off.count])
    assert len(cands[0][0]) >= 3
    T = smallest_kept_distance(cands, 8, depth)
    ds = DeviceDataset(c, 128)
    ds.set_novelty(depth, T)
    c.harvest(ds, labels, flags, tag=3)
    m = Mirror(8, depth, T, 128)
    keep = m.append(*cands[0])
    m.check(ds)
    assert keep.any() and not keep.all()
    ds.close()
    off.close()
    return cands[0][1]


def test_windowed_batch():
    w, h, ww, wh = 320, 256, 208, 160
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    origins = np.array([(40 + 9 * f, 30 + 5 * f) for f in range(8)], np.int32)
    meta = one_append(c, frames_of(w, h), windows=(origins, ww, wh))
    assert meta["win_x"].any() and meta["win_y"].any()
    c.close()


def test_bayer_8_bit():
    w, h = 320, 256
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_input_format(BR.BG)
    one_append(c, BR.mosaic(frames_of(w, h), BR.BG))
    c.close()


def test_bayer_16_bit_mirrored_and_flipped():
    w, h, pattern = 320, 256, BR.GB
    m = BR.mosaic(frames_of(w, h), RR.derived_pattern(pattern, w, h, True, True))
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_input_format(pattern)
    c.set_input_layout(16, 4, True, True)
    one_append(c, synth.raw_frame(m, 16, 4, True, True, np.random.default_rng(3)))
    c.close()


def test_enhanced_batch():
    w, h = 320, 256
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_enhance(True)
    one_append(c, ER.dim(frames_of(w, h), 80))
    c.close()


def test_misses_with_the_synthetic_model():
    w, h = 320, 256
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.svm_load(*synth.svm_weights())
    c.upload(frames_of(w, h))
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY)
    c.sync()
    (arm, offs), ident = c.armours(), c.identities()
    labels = np.array([ident[offs[f]] if offs[f + 1] > offs[f] and f % 2 == 0 else 99 for f in range(8)], np.int32)   # some armours match, some do not
    meta = one_append(c, frames_of(w, h), HARVEST_MISSES, STAGE_ALL | STAGE_IDENTITY, labels=labels)
    assert 0 < len(meta) < len(arm) and (meta["identity"] != meta["label"]).all() and (ident[offs[:-1][::2]] == labels[::2]).any()   # only misses were candidates
    c.close()


# ---------------------------------------------------------------- 4. 264 frames, a capacity smaller than the kept rows
def test_264_frames_and_a_full_dataset(wide):
    w, h, n_frames = 200, 136, 264
    c = wide
    frames = np.concatenate([frames_of(w, h)] * 33)
    labels = (np.arange(n_frames) % 7).astype(np.int32)
    labels[::5] = HARVEST_SKIP
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    off = DeviceDataset(c, 4096)
    for tag in range(2):
        c.harvest(off, labels, tag=tag)
    per = off.count // 2
    assert off.dropped == 0 and per >= 100
    cands = slices(off, [per, 2 * per])
    T = smallest_kept_distance(cands, n_frames, 2)
    roomy = Mirror(n_frames, 2, T, 1 << 30)
    for rows, meta in cands:
        roomy.append(rows, meta)
    assert roomy.state.near > 0 and roomy.keeps[1].any()                          # the second append has both kinds
    capacity = per + int(roomy.keeps[1].sum()) // 2                               # ends inside the second append's kept rows
    ds, m = DeviceDataset(c, capacity), Mirror(n_frames, 2, T, capacity)
    ds.set_novelty(2, T)
    for tag, (rows, meta) in enumerate(cands):
        c.harvest(ds, labels, tag=tag)
        m.append(rows, meta)
    m.check(ds)
    assert ds.dropped > 0 and ds.count == capacity
    assert m.state.near == roomy.state.near and np.array_equal(m.state.rings, roomy.state.rings) and np.array_equal(m.state.pushed, roomy.state.pushed)
    ds.close()
    off.close()


# ---------------------------------------------------------------- 5. a pipeline
def test_pipeline_filters_in_ticket_order_without_blocking(small):
    w, h = 320, 256
    c, A = small, frames_of(w, h)
    batches = [A, np.roll(A, 1, axis=0)] * 2 + [A]
    off = DeviceDataset(c, 512)
    cands = slices(off, harvest_all(c, batches, [off]))
    bufs = []
    for frames in batches[:2]:
        d = C.c_void_p()
        assert lib().rmcv_device_alloc(0, C.c_int64(frames.nbytes), C.byref(d)) == 0
        assert lib().rmcv_device_upload(0, d, ptr(np.ascontiguousarray(frames)), C.c_int64(frames.nbytes)) == 0
        bufs.append(d)
    pl = Pipeline(device=0, depth=3, max_frames=8, max_width=w, max_height=h)
    ds, m = DeviceDataset(c, 512), Mirror(8, 8, 0, 512)
    ds.set_novelty(8, 0)
    pl.set_harvest(ds, LABELS)
    tickets = [pl.submit(bufs[t % 2].value, 8, h, w, default_params(), STAGE_ALL) for t in range(5)]
    pl.wait(tickets[-1])
    for rows, meta in cands:
        m.append(rows, meta)
    m.check(ds)
    assert tickets == list(range(5)) and m.state.near > 0 and sum(int(k.sum()) for k in m.keeps[2:]) > 0
    assert pl.get_info().host_blocking_calls == 0
    pl.set_harvest(None)
    pl.close()
    ds.close()
    off.close()
    for d in bufs:
        lib().rmcv_device_free(0, d)


# ---------------------------------------------------------------- 6. novelty off again, clear
def test_novelty_off_after_use_and_clear(small):
    w, h = 320, 256
    c = small
    c.upload(frames_of(w, h))
    c.run(default_params(), STAGE_ALL)
    ds, never = DeviceDataset(c, 256), DeviceDataset(c, 256)
    assert ds.novelty == {"ring_rows": 0, "max_sad": 0, "near": 0} and ds.rings()[0].shape == (8, 0, abi.SVM_FEATURES)
    ds.set_novelty(2, 0)
    c.harvest(ds, LABELS, tag=1)
    c.harvest(ds, LABELS, tag=1)
    first, near = ds.count, ds.novelty["near"]
    assert near > 0 and ds.rings()[1].any()
    ds.set_novelty(0, 0)
    c.harvest(ds, LABELS, tag=2)
    c.harvest(never, LABELS, tag=2)
    assert never.count >= 3 and ds.count == first + never.count
    assert np.array_equal(ds.rows(first), never.rows()) and ds.meta(first).tobytes() == never.meta().tobytes()
    assert ds.novelty == {"ring_rows": 0, "max_sad": 0, "near": near}
    ds.set_novelty(2, 5)                                                        # every ring is empty again: the next append keeps what the first kept
    assert not ds.rings()[0].any() and not ds.rings()[1].any() and ds.novelty["near"] == near
    c.harvest(ds, LABELS, tag=3)
    ds.clear()
    assert (ds.count, ds.dropped) == (0, 0) and ds.novelty == {"ring_rows": 2, "max_sad": 5, "near": 0}
    assert not ds.rings()[0].any() and not ds.rings()[1].any()
    ds.close()
    never.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(small):
    c = small
    ds = DeviceDataset(c, 32)
    for depth, T, what in ((-1, 0, "ring_rows outside"), (HARVEST_RING_MAX + 1, 0, "ring_rows outside"), (1, -1, "max_sad outside"), (1, ICON_SAD_MAX + 1, "max_sad outside")):
        with pytest.raises(RmcvError, match=what):
            ds.set_novelty(depth, T)
    assert ds.novelty == {"ring_rows": 0, "max_sad": 0, "near": 0}
    ds.set_novelty(HARVEST_RING_MAX, ICON_SAD_MAX)
    rows = np.zeros((3, abi.SVM_FEATURES), np.uint8)
    ma = c.limits.max_armours
    with pytest.raises(RmcvError, match="n_streams outside"):
        ds.append_rows(rows[:0], [], [])
    with pytest.raises(RmcvError, match="n_streams outside"):
        ds.append_rows(rows[:0], [0] * 9, [1] * 9)
    with pytest.raises(RmcvError, match="n_rows outside"):
        ds.append_rows(np.zeros((ma + 1, abi.SVM_FEATURES), np.uint8), [ma + 1], [1])
    one, lb = np.array([3], np.int32), np.array([1], np.int32)
    bad = np.array([-1], np.int32)
    call = lib().rmcv_dataset_append_rows
    for args in ((None, ptr(one), ptr(lb), 1), (ptr(rows), None, ptr(lb), 1), (ptr(rows), ptr(one), None, 1), (ptr(rows), ptr(bad), ptr(lb), 1)):
        assert call(ds._h, *args, C.c_uint64(0)) == abi.ERR_BAD_ARG
    assert "append_rows" in lib().rmcv_dataset_last_error(ds._h).decode()
    assert call(None, ptr(rows), ptr(one), ptr(lb), 1, C.c_uint64(0)) == abi.ERR_BAD_ARG
    for first, n in ((-1, 1), (0, 9), (8, 1)):
        with pytest.raises(RmcvError, match="streams outside"):
            ds.rings(first, n)
    assert lib().rmcv_dataset_set_novelty(None, 1, 0) == abi.ERR_BAD_ARG and lib().rmcv_dataset_novelty(None, None, None, None) == abi.ERR_BAD_ARG
    assert lib().rmcv_dataset_get_rings(None, 0, 1, None, None) == abi.ERR_BAD_ARG
    # a context whose armour tables are wider than the keep bytes of the dataset's creator
    big = Context(device=0, max_frames=8, max_width=200, max_height=136, max_armours=ma + 8)
    big.upload(frames_of(200, 136))
    big.run(default_params(), STAGE_ALL)
    with pytest.raises(RmcvError, match="max_armours is beyond"):
        big.harvest(ds, LABELS)
    big.close()
    assert (ds.count, ds.dropped) == (0, 0) and ds.novelty["near"] == 0 and not ds.rings()[1].any()   # nothing was enqueued by any of them
    ds.append_rows(rows, [3], [1])                                              # ... and the dataset still works: one kept, two near
    assert ds.count == 1 and ds.novelty["near"] == 2
    ds.close()
