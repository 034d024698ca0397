"""The dataset harvest on the GPU (k_harvest.hip): rows equal the icons the oracle's classify_armours cuts from what each
pixel accessor reads (the frame, its window's crop, D(m), D(T(r)), E(f)); slots, metadata, count and dropped equal tests/harvest_ref.py;
a pipeline appends in ticket order without a blocking call; training and prediction read the dataset in place, bit for bit as
svm.train_auto / Model.predict on the downloaded rows; every refusal comes with its message."""
import ctypes as C
import functools

import numpy as np
import pytest

import bayer_ref as BR
import enhance_ref as ER
import harvest_ref as R
import raw_ref as RR
import svm_cases as SK
import window_ref as WR
from rmcv_amd import (CAMP_BLUE, HARVEST_META, HARVEST_MISSES, HARVEST_SKIP, STAGE_ALL, STAGE_ARMOURS, STAGE_IDENTITY, Context, DeviceDataset, Pipeline,
                      RmcvError, default_params, svm, synth)
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu

SIZES = {(320, 256): (0, 1, 2, 3, 4, 5, 6, 7), (200, 136): (0, 1, 2, 3, 4, 5, 6, 7)}   # the synthetic stream's indices per size (checked on the CPU: >= 3 armours)
LABELS = np.array([1, 2, HARVEST_SKIP, 3, 4, 5, 6, 0], np.int32)


@functools.lru_cache(maxsize=None)
def frames_of(w, h):
    f = np.stack([synth.frame(i, w, h, CAMP_BLUE, 0) for i in SIZES[(w, h)]])
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def small():
    c = Context(device=0, max_frames=8, max_width=320, max_height=256)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_svm():
    c = Context(device=0, max_frames=8, max_width=320, max_height=256)
    c.svm_load(*synth.svm_weights())
    yield c
    c.close()


def tables_of(c):
    """(armours, offsets, n_armours, status, the armours as the [frame, max_armours] table's occupied rows) of the batch run last"""
    c.sync()
    arm, offs = c.armours()
    k = c.counts()
    return arm, offs, k["n_armours"], k["status"]


def expect(oracle, images, arm, offs, items, size):
    """rows and clamped icon quadrilaterals of `items` from the oracle: classify_armours(image, armours, svm) returns the icons"""
    svm_ = synth.svm_weights()
    rows, quads = [], []
    cache = {}
    for f, a, _ in items:
        if f not in cache:
            cache[f] = oracle.classify_armours(images[f], arm[offs[f]:offs[f + 1]], svm_)
        _, ra, icons = cache[f]
        rows.append(np.asarray(icons[a], np.uint8).reshape(-1))
        quads.append(R.clamp_icon(arm[offs[f] + a]["icon"], *size))
        assert np.array_equal(quads[-1], ra[a]["icon"])      # (the restated clamp is the reference's)
    return np.array(rows, np.uint8).reshape(len(items), abi.SVM_FEATURES), np.array(quads, np.float32).reshape(len(items), 4, 2)


def check_dataset(ds, oracle, images, arm, offs, items, labels, identity, tag, size, origins=None, first=0):
    rows, quads = expect(oracle, images, arm, offs, items, size)
    n = len(items)
    assert np.array_equal(ds.rows(first, n), rows)
    m = ds.meta(first, n)
    want = R.expected_meta(items, labels, identity, tag, origins)
    got = [tuple(int(m[k][i]) for k in ("tag", "frame", "armour", "label", "identity", "win_x", "win_y")) for i in range(n)]
    assert got == want
    assert m["icon"].tobytes() == quads.tobytes()


def ident_table(c, offs):
    """the identities as a [frame, max_armours] table"""
    ident = c.identities()
    out = np.full((len(offs) - 1, c.limits.max_armours), -7, np.int32)
    for f in range(len(offs) - 1):
        out[f, :offs[f + 1] - offs[f]] = ident[offs[f]:offs[f + 1]]
    return out


# ---------------------------------------------------------------- 1. no model loaded
@pytest.mark.parametrize("w,h", list(SIZES), ids=["320x256", "200x136"])
def test_no_model_rows_metadata_and_untouched_armours(small, oracle, w, h):
    c, frames = small, frames_of(w, h)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    arm, offs, n, st = tables_of(c)
    ds = DeviceDataset(c, 64)
    c.harvest(ds, LABELS, tag=77)
    items, count, dropped = R.plan(n, st, LABELS, None, c.limits.max_armours, 0, 0, 64)
    assert len(items) >= 3 and (ds.count, ds.dropped) == (count, 0) and dropped == 0
    assert 2 not in items[:, 0] and n[2] > 0                                 # the skipped frame had armours to give
    check_dataset(ds, oracle, frames, arm, offs, items, LABELS, None, 77, (w, h))
    assert c.armours()[0].tobytes() == arm.tobytes()                         # the armour table is only read
    ds.close()


# ---------------------------------------------------------------- 2. with a model
@pytest.mark.parametrize("w,h", list(SIZES), ids=["320x256", "200x136"])
def test_with_identity_stage_and_misses(small_svm, oracle, w, h):
    c, frames = small_svm, frames_of(w, h)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY)
    arm, offs, n, st = tables_of(c)
    ident = ident_table(c, offs)
    assert len(arm) >= 3
    labels = np.arange(8, dtype=np.int32)
    ds = DeviceDataset(c, 64)
    c.harvest(ds, labels, tag=5)
    items, count, _ = R.plan(n, st, labels, ident, c.limits.max_armours, 0, 0, 64)
    assert ds.count == count == len(arm)
    rows, meta = ds.rows(), ds.meta()
    at = 0
    for f in range(8):                                                       # Context.icons(f), row for row
        icons = c.icons(f)
        assert np.array_equal(rows[at:at + len(icons)], icons.reshape(len(icons), abi.SVM_FEATURES)), f
        at += len(icons)
    assert np.array_equal(meta["identity"], c.identities())
    check_dataset(ds, oracle, frames, arm, offs, items, labels, ident, 5, (w, h))
    # labels under which some armours match and some do not: exactly the mismatching ones are kept
    flat = c.identities()
    labels = np.array([flat[offs[f]] if offs[f + 1] > offs[f] and f % 2 == 0 else 99 for f in range(8)], np.int32)
    ds.clear()
    c.harvest(ds, labels, HARVEST_MISSES, tag=6)
    items, count, _ = R.plan(n, st, labels, ident, c.limits.max_armours, HARVEST_MISSES, 0, 64)
    assert 0 < count < len(arm) and ds.count == count                        # both kinds occur
    check_dataset(ds, oracle, frames, arm, offs, items, labels, ident, 6, (w, h))
    assert all(ident[f][a] != labels[f] for f, a, _ in items)
    ds.close()


# ---------------------------------------------------------------- 3. every pixel accessor
def run_and_check(c, oracle, images, upload, size, stages=STAGE_ALL, origins=None):
    c.upload(upload)
    if origins is not None:
        c.set_windows(origins[0], origins[1], origins[2])
    c.run(default_params(), stages)
    arm, offs, n, st = tables_of(c)
    eff = c.windows()[0] if origins is not None else None
    ds = DeviceDataset(c, 64)
    c.harvest(ds, LABELS, tag=9)
    items, count, _ = R.plan(n, st, LABELS, None, c.limits.max_armours, 0, 0, 64)
    assert len(items) >= 3 and ds.count == count
    if callable(images):
        images = images(eff)
    check_dataset(ds, oracle, images, arm, offs, items, LABELS, None, 9, size, eff)
    ds.close()
    return arm


def test_windowed_batch(oracle):
    w, h, ww, wh = 320, 256, 208, 160
    frames = frames_of(w, h)
    origins = []
    for f in range(8):                                                       # windows around each frame's first armour, some cutting it
        a = oracle.detect_frame(frames[f], oracle.default_params())["armours"]
        cx, cy = (a[0]["vertices"].reshape(-1, 2).mean(0) if len(a) else (w / 2, h / 2))
        origins.append((int(cx) - ww // 2 + (37 if f % 3 == 0 else 0), int(cy) - wh // 2 - (25 if f % 3 == 0 else 0)))
    origins = np.array(origins, np.int32)
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    crops = lambda eff: [WR.crop(frames[f], eff[f], ww, wh) for f in range(8)]
    run_and_check(c, oracle, crops, frames, (ww, wh), origins=(origins, ww, wh))
    assert np.array_equal(c.windows()[0], WR.effective_origins(origins, w, h, ww, wh)) and c.windows()[0].any()
    c.close()


@pytest.mark.parametrize("w,h", list(SIZES), ids=["320x256", "200x136"])
def test_bayer_8_bit(oracle, w, h):
    mos = BR.mosaic(frames_of(w, h), BR.BG)
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_input_format(BR.BG)
    run_and_check(c, oracle, [BR.demosaic(mos[f], BR.BG) for f in range(8)], mos, (w, h))
    c.close()


def test_bayer_16_bit_mirrored_and_flipped(oracle):
    w, h, pattern = 320, 256, BR.GB
    dp = RR.derived_pattern(pattern, w, h, True, True)
    m = BR.mosaic(frames_of(w, h), dp)
    r = synth.raw_frame(m, 16, 4, True, True, np.random.default_rng(3))
    assert np.array_equal(RR.T(r, 4, True, True), m)
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_input_format(pattern)
    c.set_input_layout(16, 4, True, True)
    run_and_check(c, oracle, [BR.demosaic(m[f], dp) for f in range(8)], r, (w, h))
    c.close()


def test_enhanced_batch(oracle):
    w, h = 320, 256
    frames = ER.dim(frames_of(w, h), 80)
    fe = [ER.E(f, 100.0, 50.0)[0] for f in frames]
    assert any(not np.array_equal(fe[f], frames[f]) for f in range(8))
    c = Context(device=0, max_frames=8, max_width=w, max_height=h)
    c.set_enhance(True)
    run_and_check(c, oracle, fe, frames, (w, h))
    c.close()


# ---------------------------------------------------------------- 4. weird icons
def test_icons_outside_the_frame_and_of_zero_area(small, oracle):
    """through the batch's own armour table (rmcv_batch_device_views): frame 0 is given test_classify.py's three armours"""
    w, h = 320, 256
    c, frames = small, frames_of(w, h)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    weird = np.zeros(3, abi.ARMOUR)
    weird[0]["icon"] = [[-50, 300], [-50, -30], [400, -30], [400, 300]]       # leaves the frame on every side: clamped
    weird[1]["icon"] = [[100, 100], [100, 100], [100, 100], [100, 100]]       # zero area: a row, not a fault
    weird[2]["icon"] = [[150, 100], [160, 50], [230, 70], [220, 120]]
    d_arm, d_cnt, cap, n = c.device_views()
    assert cap >= 3 and n == 8
    three = np.array([3], np.int32)
    assert lib().rmcv_device_upload(0, C.c_void_p(d_arm), ptr(weird), C.c_int64(weird.nbytes)) == 0
    assert lib().rmcv_device_upload(0, C.c_void_p(d_cnt), ptr(three), C.c_int64(4)) == 0
    labels = np.full(8, HARVEST_SKIP, np.int32)
    labels[0] = 4
    ds = DeviceDataset(c, 8)
    c.harvest(ds, labels, tag=1)
    assert (ds.count, ds.dropped) == (3, 0)
    _, ra, icons = oracle.classify_armours(frames[0], weird, synth.svm_weights())
    rows, meta = ds.rows(), ds.meta()
    assert np.array_equal(rows, np.asarray(icons, np.uint8).reshape(3, -1))
    assert meta["icon"].tobytes() == ra["icon"].tobytes() and (ra["icon"][0] != weird["icon"][0]).any()
    assert not np.array_equal(rows[1], rows[2]) and rows[0].any()
    assert c.armours()[0][:3].tobytes() == weird.tobytes()                   # still unclamped: the table is only read
    ds.close()


# ---------------------------------------------------------------- 5. scan and capacity
def test_264_frames_scan_and_capacity(oracle):
    w, h, n_frames = 200, 136, 264
    eight = frames_of(w, h)
    frames = np.concatenate([eight] * 33)
    labels = (np.arange(n_frames) % 7).astype(np.int32)
    labels[::5] = HARVEST_SKIP
    c = Context(device=0, max_frames=n_frames, max_width=w, max_height=h)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    arm, offs, n, st = tables_of(c)
    ma = c.limits.max_armours
    every, kept, _ = R.plan(n, st, labels, None, ma, 0, 0, 1 << 30)
    assert kept >= 3 * 33 * 0.5
    frames_with_two = [f for f in range(8, n_frames) if labels[f] != HARVEST_SKIP and n[f] >= 2]
    inside = int(every[every[:, 0] == frames_with_two[len(frames_with_two) // 2]][0][2]) + 1   # a capacity that ends inside that frame's rows
    ds = DeviceDataset(c, inside)
    c.harvest(ds, labels, tag=1)
    items, count, dropped = R.plan(n, st, labels, None, ma, 0, 0, inside)
    assert (ds.count, ds.dropped) == (count, dropped) == (inside, kept - inside)
    m = ds.meta()
    assert np.array_equal(np.stack([m["frame"], m["armour"], np.arange(count)], 1), items)
    assert np.array_equal(m["label"], labels[items[:, 0]])
    # the oracle on the eight distinct frames; the other 256 repeat them
    ref_rows, _ = expect(oracle, eight, arm, offs, np.array([(f, a, 0) for f in range(8) for a in range(min(n[f], ma))], np.int32).reshape(-1, 3), (w, h))
    by_fa = {(f, a): ref_rows[i] for i, (f, a) in enumerate((f, a) for f in range(8) for a in range(min(n[f], ma)))}
    got = ds.rows()
    assert all(np.array_equal(got[i], by_fa[(int(f) % 8, int(a))]) for i, (f, a, _) in enumerate(items))
    ds.close()
    # a second append onto a partly filled dataset, then one onto a full dataset
    cap = kept + kept // 2
    ds = DeviceDataset(c, cap)
    c.harvest(ds, labels, tag=1)
    assert (ds.count, ds.dropped) == (kept, 0)
    c.harvest(ds, labels, tag=2)
    items2, count2, dropped2 = R.plan(n, st, labels, None, ma, 0, kept, cap)
    assert (ds.count, ds.dropped) == (count2, dropped2) == (cap, kept - kept // 2)
    m = ds.meta()
    assert np.array_equal(np.stack([m["frame"][kept:], m["armour"][kept:], np.arange(kept, cap)], 1), items2)
    assert set(m["tag"][:kept]) == {1} and set(m["tag"][kept:]) == {2}
    got = ds.rows()
    assert all(np.array_equal(got[s], by_fa[(int(f) % 8, int(a))]) for f, a, s in items2)
    before = (got.tobytes(), m.tobytes())
    c.harvest(ds, labels, tag=3)
    _, count3, dropped3 = R.plan(n, st, labels, None, ma, 0, cap, cap, dropped2)
    assert (ds.count, ds.dropped) == (count3, dropped3) == (cap, dropped2 + kept)
    assert (ds.rows().tobytes(), ds.meta().tobytes()) == before
    ds.close()
    c.close()


# ---------------------------------------------------------------- 6. the pipeline
def test_pipeline_appends_in_ticket_order_without_blocking(small):
    w, h = 320, 256
    c, frames = small, frames_of(w, h)
    labels = LABELS
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    bare = DeviceDataset(c, 256)
    for t in range(5):
        c.harvest(bare, labels, tag=t)
    per = bare.count // 5
    assert per >= 3 and bare.count == 5 * per
    d_frames = C.c_void_p()
    assert lib().rmcv_device_alloc(0, C.c_int64(frames.nbytes), C.byref(d_frames)) == 0
    assert lib().rmcv_device_upload(0, d_frames, ptr(np.ascontiguousarray(frames)), C.c_int64(frames.nbytes)) == 0
    pl = Pipeline(device=0, depth=3, max_frames=8, max_width=w, max_height=h)
    ds = DeviceDataset(c, 256)
    pl.set_harvest(ds, labels)
    tickets = [pl.submit(d_frames.value, 8, h, w, default_params(), STAGE_ALL) for _ in range(5)]
    pl.wait(tickets[-1])                                                     # (the newest batch's back half is enqueued by the call that waits for it)
    assert tickets == list(range(5)) and ds.count == bare.count and ds.dropped == 0
    assert np.array_equal(ds.rows(), bare.rows()) and ds.meta().tobytes() == bare.meta().tobytes()
    assert list(ds.meta()["tag"]) == sorted(ds.meta()["tag"]) and set(ds.meta()["tag"]) == set(range(5))
    assert pl.get_info().host_blocking_calls == 0
    # a batch with more frames than the label table is refused before anything is enqueued
    pl.set_harvest(ds, labels[:4])
    with pytest.raises(RmcvError, match="more frames than the label table"):
        pl.submit(d_frames.value, 8, h, w, default_params(), STAGE_ALL)
    with pytest.raises(RmcvError, match="RMCV_STAGE_ARMOURS"):
        pl.submit(d_frames.value, 4, h, w, default_params(), STAGE_ALL & ~STAGE_ARMOURS)
    assert pl.get_info().submitted == 5
    pl.set_harvest(None)
    t = pl.submit(d_frames.value, 8, h, w, default_params(), STAGE_ALL)
    pl.wait(t)
    assert ds.count == bare.count
    pl.close()
    ds.close()
    bare.close()
    lib().rmcv_device_free(0, d_frames)


# ---------------------------------------------------------------- 7. training in place
def place(ds, rows, labels):
    """rows and labels into a dataset through its device views"""
    d_rows, d_meta, d_count = ds.device()
    meta = np.zeros(len(rows), HARVEST_META)
    meta["label"], meta["frame"] = labels, np.arange(len(rows))
    count = np.array([len(rows)], np.int32)
    for dst, src in ((d_rows, np.ascontiguousarray(rows, np.uint8)), (d_meta, meta), (d_count, count)):
        assert lib().rmcv_device_upload(0, C.c_void_p(dst), ptr(src), C.c_int64(src.nbytes)) == 0


def test_training_and_prediction_in_place(small_svm):
    c = small_svm
    rows, cls = SK._icons(np.random.RandomState(21), 3, 30, 60)
    order = np.random.RandomState(22).permutation(len(rows))
    rows, resp = rows[order], (cls[order] * 3 + 2).astype(np.int32)           # labels are not class indices
    ds = DeviceDataset(c, 128)
    place(ds, rows, resp)
    assert ds.count == 90 and np.array_equal(ds.rows(), rows) and np.array_equal(ds.meta()["label"], resp)
    head, tail = ds.sample(0.6, seed=1)
    assert sorted(head) == [2, 5, 8] and all(len(head[k]) == 18 and len(tail[k]) == 12 for k in head)
    sub = np.concatenate([head[k] for k in sorted(head)])
    perm = np.random.RandomState(23).permutation(len(sub)).astype(np.int32)
    params = {"eps": 1e-3, "max_iter": 1000, "k_fold": 3, "c_grid": [0.1, 0.5]}
    got = ds.train_auto(sub, perm, **params)
    want = svm.train_auto(ds.rows()[sub], ds.meta()["label"][sub], perm, ctx=c, **params)
    for g, w_ in ((got, want), (ds.train_auto(None, None, **params), svm.train_auto(rows, resp, None, ctx=c, **params))):
        assert g.weights.tobytes() == w_.weights.tobytes() and g.rho.tobytes() == w_.rho.tobytes() and g.labels.tobytes() == w_.labels.tobytes()
        assert g.report["best_index"] == w_.report["best_index"] and g.report["best_c"] == w_.report["best_c"] and g.report["cv_errors"] == w_.report["cv_errors"]
        assert np.array_equal(g.report["iterations"], w_.report["iterations"]) and np.array_equal(g.report["converged"], w_.report["converged"])
        assert g.report["objective"].tobytes() == w_.report["objective"].tobytes()
    assert list(got.labels) == [2, 5, 8]
    held = np.concatenate([tail[k] for k in sorted(tail)])
    try:
        got.load_into(c)
        assert np.array_equal(ds.predict(held), got.predict(rows[held])) and np.array_equal(ds.predict(), got.predict(rows))
        assert (ds.predict(held) == resp[held]).mean() > 0.9                   # optimizer.cpp:27-40's validation accuracy, rows in place
    finally:
        c.svm_load(*synth.svm_weights())
    ds.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(small_svm):
    c = small_svm
    w, h = 200, 136
    with pytest.raises(RmcvError, match="capacity_rows < 1"):
        DeviceDataset(c, 0)
    ds = DeviceDataset(c, 32)
    fresh = Context(device=0, max_frames=8, max_width=w, max_height=h)
    with pytest.raises(RmcvError, match="no frames bound"):
        fresh.harvest(ds, LABELS)
    fresh.close()
    c.upload(frames_of(w, h))
    c.run(default_params(), STAGE_ALL & ~STAGE_ARMOURS)
    with pytest.raises(RmcvError, match="lacked RMCV_STAGE_ARMOURS"):
        c.harvest(ds, LABELS)
    c.run(default_params(), STAGE_ALL)
    with pytest.raises(RmcvError, match="RMCV_HARVEST_MISSES needs a run with RMCV_STAGE_IDENTITY"):
        c.harvest(ds, LABELS, HARVEST_MISSES)
    with pytest.raises(RmcvError, match="unknown flags"):
        c.harvest(ds, LABELS, 2)
    assert ds.count == 0                                                     # nothing was enqueued by any of them
    import torch
    if torch.cuda.device_count() > 1:                                        # (one device: the rule is checked on the host, tests/test_harvest_plan.py)
        other = Context(device=1, max_frames=8, max_width=w, max_height=h)
        far = DeviceDataset(other, 8)
        with pytest.raises(RmcvError, match="another device"):
            c.harvest(far, LABELS)
        far.close()
        other.close()
    c.harvest(ds, LABELS)
    count = ds.count
    assert count >= 3
    with pytest.raises(RmcvError, match="outside 0 .. count - 1"):
        ds.train_auto([0, count])
    with pytest.raises(RmcvError, match="outside 0 .. count - 1"):
        ds.train_auto([-1, 0])
    with pytest.raises(RmcvError, match="outside 0 .. count - 1"):
        ds.predict([count])
    with pytest.raises(RmcvError, match="RMCV_SVM_MAX_SAMPLES"):
        ds.train_auto(np.zeros(abi.SVM_MAX_SAMPLES + 1, np.int32))
    # the trainer's own refusals, unchanged: the message svm.train_auto gives on the same rows
    one = np.flatnonzero(ds.meta()["label"] == ds.meta()["label"][0]).astype(np.int32)
    with pytest.raises(RmcvError) as mine:
        ds.train_auto(one)
    with pytest.raises(RmcvError) as theirs:
        svm.train_auto(ds.rows()[one], ds.meta()["label"][one], ctx=c)
    assert str(mine.value) == str(theirs.value) and str(mine.value)
    ds.close()
