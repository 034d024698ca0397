"""What a batch context keeps and drops between bindings, and what its table and gather getters hand out (rmcv_host.hip): a new binding
-- through rmcv_batch_upload or rmcv_batch_set_device_frames -- switches every per-frame mode of the one before off (windows, camps and
lower bounds, cameras) and starts with nothing run; the four effective-table getters respect `cap` and give the documented values with
their mode off and on; the gather getters equal the device rows taken by the counts; rmcv_ctx_set_option takes exactly the ends of every
option's range.  Small frames (128 x 96, windows of 64 x 48, at most 4 of them, one without an armour): every call runs once.

rmcv_batch_get_gammas is the one table getter that refuses a null pointer with cap 0 (the other three document that they take it): pinned
here as it is."""
import ctypes as C

import numpy as np
import pytest

import bind_plan_ref as BR
import camera_cases as CK
import window_ref as W
from rmcv_amd import (CAMP_BLUE, CAMP_RED, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Context, RmcvError, Tracker, abi, default_params, default_pnp_config,
                      synth)
from rmcv_amd.abi import lib, ptr
from test_gpu_attitude import device_array, download
from test_oracle_pnp import rodrigues

pytestmark = pytest.mark.gpu

N, FW, FH, WW, WH = 4, 128, 96, 64, 48
SEEDS = (323, 324, 325, 317)          # synthetic frames with 5, 0, 1 and 3 armours at this size
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
ORIGINS = np.array([[20, 8], [0, 0], [70, 60], [33, 16]], np.int32)
CAMPS, BOUNDS, CAMERAS = [CAMP_RED, CAMP_BLUE, 2, CAMP_BLUE], [60, 0, 300, 90], [1, 0, 1, 1]


@pytest.fixture(scope="module")
def scene():
    frames = np.stack([synth.frame(s, FW, FH, CAMP_BLUE, 0) for s in SEEDS])
    rng = np.random.default_rng(5)
    mats = np.tile(np.eye(4), (N, 1, 1))
    for f in range(N):
        mats[f, :3, :3] = rodrigues(rng.uniform(-1, 1, 3))
        mats[f, :3, 3] = rng.uniform(-50, 50, 3)
    return frames, mats, [default_pnp_config(), CK.other_camera()]


def context(scene, max_frames=N):
    """identities and poses loaded, at most 8 armours a frame (rows longer than any frame's count)"""
    c = Context(device=0, max_frames=max_frames, max_width=FW, max_height=FH, max_armours=8)
    c.svm_load(*synth.svm_weights())
    c.pnp_load_cameras(scene[2])
    return c


def full_run(c, params=None):
    """armours, offsets, identities and poses of a full run, as bytes"""
    c.run(params or default_params(), FULL)
    c.sync()
    arm, offs = c.armours()
    return (arm.tobytes(), offs.tolist(), c.identities().tobytes()) + tuple(x.tobytes() for x in c.poses())


def set_every_mode(c, mats):
    c.set_windows(ORIGINS, WW, WH)
    c.set_frame_camps(CAMPS, BOUNDS)
    c.set_frame_cameras(CAMERAS)
    c.set_base2gripper(mats)


def test_rebinding_resets_every_mode(scene):
    frames, mats, cams = scene
    fresh = context(scene)
    fresh.upload(frames)
    fresh.set_base2gripper(mats)
    want = full_run(fresh)
    assert np.frombuffer(want[2], np.int32).size == sum(np.diff(want[1])) > 0 and 0 in np.diff(want[1])   # armours, and a frame without
    fresh.close()

    c = context(scene)
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH)
    p = default_params()
    p.camp, p.lower_bound = CAMP_RED, 77
    d_frames = device_array(frames)
    binders = (lambda: c.upload(frames), lambda: c.bind_device_frames(d_frames.data_ptr(), N, FH, FW, keepalive=d_frames))
    c.upload(frames)
    for rebind in binders:
        set_every_mode(c, mats)
        c.run(p, FULL)
        c.sync()
        # every mode is on, and the run used it
        eff, ww, wh = c.windows()
        assert (ww, wh) == (WW, WH) and np.array_equal(eff, W.effective_origins(ORIGINS, FW, FH, WW, WH)) and eff.any()
        assert c.frame_keys().tolist() == [list(abi.frame_key(k, b)) for k, b in zip(CAMPS, BOUNDS)]
        assert c.frame_cameras().tolist() == CAMERAS
        rebind()
        eff, ww, wh = c.windows()
        assert (ww, wh) == (0, 0) and not eff.any() and c.device_windows() == (None, 0, 0)
        assert c.frame_keys().tolist() == [list(abi.frame_key(CAMP_RED, 77))] * N        # the last run's key, for every frame
        assert c.frame_cameras().tolist() == [0] * N
        with pytest.raises(RmcvError) as e:
            c.track(trk, 1)
        assert e.value.code == abi.ERR_BAD_ARG and "RMCV_STAGE_ARMOURS" in str(e.value)  # nothing of the new batch has run
        assert full_run(c) == want
        assert c.frame_cameras().tolist() == [0] * N and c.frame_keys().tolist() == [list(abi.frame_key(CAMP_BLUE, 80))] * N
    assert c.check_guards()[0] == 0
    trk.close()
    c.close()


SENTINEL = 0x5A5A5A5A


def table_getters(c):
    """(name, call(pointer, cap), int32 words per entry) of the four effective-table getters"""
    h, L = c._h, lib()
    return (("windows", lambda p, cap: L.rmcv_batch_get_windows(h, p, cap, None, None), 2),
            ("frame_keys", lambda p, cap: L.rmcv_batch_get_frame_keys(h, p, cap), 4),
            ("frame_cameras", lambda p, cap: L.rmcv_batch_get_frame_cameras(h, p, cap), 1),
            ("gammas", lambda p, cap: L.rmcv_batch_get_gammas(h, p, cap), 1))


def check_caps(c, want):
    """want: name -> the table's n entries as int32 words (n, words); every getter with cap 0, n - 1, n and n + 1"""
    for name, get, words in table_getters(c):
        full = np.asarray(want[name]).view(np.int32).reshape(N, words)
        assert get(None, -1) == abi.ERR_BAD_ARG, name
        assert get(None, 0) == (abi.ERR_BAD_ARG if name == "gammas" else abi.OK), name
        for cap in (0, N - 1, N, N + 1):
            buf = np.full((N + 2, words), SENTINEL, np.int32)
            assert get(ptr(buf), cap) == abi.OK, (name, cap)
            n = min(cap, N)
            assert np.array_equal(buf[:n], full[:n]) and np.all(buf[n:] == SENTINEL), (name, cap)


def test_table_getters_respect_cap_off_and_on(scene):
    frames, mats, cams = scene
    c = context(scene)
    c.upload(frames)
    p = default_params()
    p.camp, p.lower_bound = CAMP_RED, 91
    c.run(p, FULL)
    c.sync()
    ones = np.ones(N, np.float32)
    check_caps(c, dict(windows=np.zeros((N, 2), np.int32), frame_keys=np.array([abi.frame_key(CAMP_RED, 91)] * N, np.int32), frame_cameras=np.zeros(N, np.int32),
                       gammas=ones))                                                                   # every mode off
    c.set_windows(ORIGINS, WW, WH)
    c.set_frame_camps(CAMPS, BOUNDS)
    c.set_frame_cameras(CAMERAS)
    c.run(p, FULL)
    c.sync()
    check_caps(c, dict(windows=W.effective_origins(ORIGINS, FW, FH, WW, WH), frame_keys=np.array([abi.frame_key(k, b) for k, b in zip(CAMPS, BOUNDS)], np.int32),
                       frame_cameras=np.array(CAMERAS, np.int32), gammas=ones))                         # windows, keys and cameras on
    ww, wh = C.c_int32(-1), C.c_int32(-1)
    assert lib().rmcv_batch_get_windows(c._h, None, 0, C.byref(ww), C.byref(wh)) == abi.OK and (ww.value, wh.value) == (WW, WH)
    c.close()
    # RMCV_OPT_ENHANCE goes with neither windows nor per-frame camps: a context of its own
    c = context(scene)
    c.set_enhance(True)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    gam = np.array([abi.enhance_gamma(f.reshape(-1, 3).sum(0, dtype=np.uint64), FW * FH) for f in frames], np.float32)
    assert len(set(gam.tolist())) > 1 and not np.any(gam == 1.0)
    check_caps(c, dict(windows=np.zeros((N, 2), np.int32), frame_keys=np.array([abi.frame_key(CAMP_BLUE, 80)] * N, np.int32), frame_cameras=np.zeros(N, np.int32),
                       gammas=gam))
    c.close()


def test_gather_getters_equal_the_device_rows(scene):
    frames, mats, cams = scene
    n = 3
    c = context(scene)
    c.upload(frames[:n])
    c.run(default_params(), FULL)
    c.sync()
    d_arm, d_cnt, row_cap, nf = c.device_views()
    assert (row_cap, nf) == (8, n)
    cnt = download(d_cnt, np.int32, n)
    assert cnt.tolist() == c.counts()["n_armours"].tolist() and 0 in cnt and cnt.max() > 1 and cnt.max() < row_cap
    rows = download(d_arm, abi.ARMOUR, n * row_cap).reshape(n, row_cap)
    arm, offs = c.armours()
    total = int(cnt.sum())
    assert offs.tolist() == [0] + np.cumsum(cnt).tolist() and len(arm) == total
    assert arm.tobytes() == b"".join(rows[f, :cnt[f]].tobytes() for f in range(n))
    # identities and poses have no device view: a one-frame batch's rows are its first count entries, so the batch's gather is their concatenation
    ids, poses = c.identities(), c.poses()
    one = context(scene, max_frames=2)    # (room for the camera table; it binds one frame at a time)
    want_ids, want_poses = [], [[], [], []]
    for f in range(n):
        one.upload(frames[f:f + 1])
        one.run(default_params(), FULL)
        one.sync()
        assert one.armours()[0].tobytes() == rows[f, :cnt[f]].tobytes()
        want_ids.append(one.identities())
        for k, x in enumerate(one.poses()):
            want_poses[k].append(x)
    one.close()
    assert ids.tobytes() == np.concatenate(want_ids).tobytes() and len(ids) == total
    for got, want in zip(poses, want_poses):
        assert got.shape == (total, 3) and got.tobytes() == np.concatenate(want).tobytes()
    # one entry short: RMCV_ERR_CAPACITY, with the total reported
    h, L = c._h, lib()
    arm_buf, id_buf, pose_buf, offs_buf = np.zeros(total, abi.ARMOUR), np.zeros(total, np.int32), np.zeros((3, total, 3)), np.zeros(n + 1, np.int32)
    for call in (lambda t: L.rmcv_batch_get_armours(h, ptr(arm_buf), total - 1, ptr(offs_buf), C.byref(t)),
                 lambda t: L.rmcv_batch_get_identities(h, ptr(id_buf), total - 1, C.byref(t)),
                 lambda t: L.rmcv_batch_get_poses(h, ptr(pose_buf[0]), ptr(pose_buf[1]), ptr(pose_buf[2]), total - 1, C.byref(t))):
        t = C.c_int32(-1)
        assert call(t) == abi.ERR_CAPACITY and t.value == total
        assert "output capacity exceeded" in L.rmcv_last_error(h).decode()
    assert offs_buf.tolist() == offs.tolist()       # the offsets are written before the capacity is held against the total
    c.close()


def test_option_bounds():
    c = Context(device=0, max_frames=1, max_width=FW, max_height=FH)
    h, L = c._h, lib()
    assert set(BR.OPTION_ENDS) == set(BR.OPTIONS)
    for option, (lo, hi) in BR.OPTION_ENDS.items():
        for value, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
            if value > BR.INT_MAX:
                continue
            rc = L.rmcv_ctx_set_option(h, option, value)
            assert rc == (abi.OK if ok else abi.ERR_BAD_ARG), (option, value)
            if not ok:
                assert L.rmcv_last_error(h).decode() == "unknown option or value", (option, value)
        assert L.rmcv_ctx_set_option(h, option, lo) == abi.OK     # (back to the low end: no delay, no slowed copy left behind)
    for option in (0, 6, 24, 1000, 1002, -1):
        assert L.rmcv_ctx_set_option(h, option, 0) == abi.ERR_BAD_ARG, option
    c.close()
