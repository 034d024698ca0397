"""The device-resident tracker on the GPU (rmcv_tracker_*, rmcv_batch_track, rmcv_pipeline_submit_tracked): after every step, every
stream's tracks, side records and requested origin equal -- byte for byte -- the CPU oracle's tracker with only hypot replaced
(tests/track_ref.py), fed with that step's collected armours, identities and poses; the effective origins of batch k + 1 are the
clamp-and-snap of the origins step k wrote.  Every GPU step runs once, with the library's deadlines as they are."""
import numpy as np
import pytest

import track_ref as T
import window_ref as W
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_BINARY, STAGE_IDENTITY, STAGE_POSE, Context, Pipeline, RmcvError, Tracker, default_params, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

FW, FH, WW, WH = 1280, 1024, 512, 384
MS = 1_000_000


def moving_scene(first, n, steps, dx=5, dy=3):
    """per stream a sequence of frames carrying a translated target: the synthetic frame of the stream, moved (dx, dy) a step"""
    base = synth.batch(first, n, FW, FH, CAMP_BLUE, 0, threads=16)
    out = []
    for k in range(steps):
        f = np.zeros_like(base)
        sx, sy = k * dx, k * dy
        f[:, sy:, sx:] = base[:, :FH - sy, :FW - sx]
        out.append(f)
    return out


def first_armour_origins(oracle, frames):
    o = []
    for f in frames:
        a = oracle.detect_frame(f, oracle.default_params())["armours"]
        assert len(a)
        o.append(W.window_origin(W.get_roi(a[0]["vertices"], (1.0, 1.0), (FW, FH)), WW, WH))
    return np.array(o, np.int32)


def ref_streams(n, win, origins, cap=64):
    return [T.RefStream(T.lib(), cap=cap, frame=(FW, FH), win=win, origin=tuple(int(v) for v in origins[f])) for f in range(n)]


def feed(refs, arm, offs, ids, pos, eff, ts):
    """one step of every reference stream with the batch's collected results; armours -> frame coordinates by rmcv_armours_to_frame"""
    for f, r in enumerate(refs):
        lo, hi = int(offs[f]), int(offs[f + 1])
        a = abi.armours_to_frame(arm[lo:hi], int(eff[f][0]), int(eff[f][1]))
        assert r.step(a, None if ids is None else ids[lo:hi], None if pos is None else pos[lo:hi], ts), f


def same(trk, refs):
    n_tr, st = trk.counts()
    for f, r in enumerate(refs):
        tr, side, org = trk.get(f)
        assert len(tr) == len(r.tracks) == n_tr[f] and st[f] == r.status, (f, len(tr), len(r.tracks), st[f])
        assert tr.tobytes() == r.tracks.tobytes(), f
        assert side.tobytes() == r.side.tobytes() and org == r.origin, (f, org, r.origin)


# ---------------------------------------------------------------- 1. context path
def test_context_closed_loop_windows_identity_pose(oracle):
    n, steps = 16, 7
    scene = moving_scene(0, n, steps)
    origins = first_armour_origins(oracle, scene[0])
    trk = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    trk.set_origins(origins)
    refs = ref_streams(n, (WW, WH), origins)
    c = Context(device=0, max_frames=n, max_width=FW, max_height=FH)
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    stages = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
    matched = 0
    for k in range(steps):
        c.upload(scene[k])
        c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
        c.set_windows(trk.device_origins(), WW, WH)
        c.run(default_params(), stages)
        c.track(trk, (k + 1) * 8 * MS)
        c.sync()
        eff = c.windows()[0]
        # batch k read its frames through the clamp-and-snap of what step k - 1 wrote (the initial requests for k = 0)
        want = W.effective_origins(np.array([r.origin for r in refs], np.int32), FW, FH, WW, WH)
        assert np.array_equal(eff, want), k
        arm, offs = c.armours()
        feed(refs, arm, offs, c.identities(), c.poses()[2], eff, (k + 1) * 8 * MS)
        same(trk, refs)
        matched += sum(int((r.tracks["initialized"] == 1).sum()) for r in refs)
    assert matched > 0 and all(len(r.tracks) for r in refs)
    assert len({r.origin for r in refs}) > 4 and any(r.origin != tuple(origins[f]) for f, r in enumerate(refs))   # the windows followed
    assert not trk.counts()[1].any() and c.check_guards()[0] == 0
    trk.reset()
    assert not trk.counts()[0].any()
    c.close()
    trk.close()


def test_context_whole_frames_without_identity_and_pose():
    n, steps = 8, 3
    scene = moving_scene(40, n, steps, dx=2, dy=1)
    trk = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, track_cap=16)
    refs = ref_streams(n, (0, 0), np.zeros((n, 2), np.int32), cap=16)
    c = Context(device=0, max_frames=n, max_width=FW, max_height=FH)
    for k in range(steps):
        c.upload(scene[k])
        c.run(default_params(), STAGE_ALL)
        c.track(trk, (k + 1) * 5 * MS)
        c.sync()
        arm, offs = c.armours()
        feed(refs, arm, offs, None, None, np.zeros((n, 2), np.int32), (k + 1) * 5 * MS)
        same(trk, refs)
    assert sum(len(r.tracks) for r in refs) >= n
    assert all((r.tracks["identity"] == -1).all() and not r.tracks["position"].any() for r in refs)
    c.close()
    trk.close()


# ---------------------------------------------------------------- 3. refusals and lifetime
def test_refusals_and_destroy_with_work_in_flight():
    n = 4
    frames = synth.batch(0, n, FW, FH, CAMP_BLUE, 0, threads=8)
    c = Context(device=0, max_frames=8, max_width=1920, max_height=1200)

    def refused(trk, text):
        with pytest.raises(RmcvError) as e:
            c.track(trk, 1)
        assert e.value.code == abi.ERR_BAD_ARG and text in str(e.value), str(e.value)

    good = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    c.upload(frames)
    refused(good, "RMCV_STAGE_ARMOURS")                       # nothing has run on this batch yet
    c.run(default_params(), STAGE_BINARY)
    refused(good, "RMCV_STAGE_ARMOURS")                       # ... and a pixel pass alone leaves nothing to track
    c.run(default_params(), STAGE_ALL)
    for kw, text in ((dict(n_streams=n + 1, frame_w=FW, frame_h=FH), "streams"), (dict(n_streams=n, frame_w=1920, frame_h=1200), "1920 x 1200")):
        t = Tracker(device=0, **kw)
        refused(t, text)
        t.close()
    c.set_windows(np.zeros((n, 2), np.int32), 256, 128)
    c.run(default_params(), STAGE_ALL)
    refused(good, "256 x 128")                                # windows of another size than the tracker writes origins for
    c.set_windows(None, 0, 0)
    c.run(default_params(), STAGE_ALL)
    c.track(good, 1)                                          # whole frames are fine for a windowed tracker (the host decides per batch)
    c.sync()
    for bad in (dict(n_streams=0), dict(track_cap=65), dict(track_cap=0), dict(tick_frequency=0.0), dict(win_w=512, win_h=0), dict(win_w=2000, win_h=100)):
        with pytest.raises(RmcvError):
            Tracker(device=0, **bad)
    # destroy with a step in flight drains first
    c.run(default_params(), STAGE_ALL)
    c.track(good, 2)
    good.close()
    c.sync()
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 2. pipeline path
def test_pipeline_two_trackers_interleaved_with_untracked_submits(oracle):
    """bursts of tracked submits with nothing collected in between: the host only submits, batch k + 1 of a tracker reads the origins its
    step k wrote.  Tracker A is windowed (identity + pose), tracker B tracks whole frames, untracked submits alternate with both."""
    import torch
    n, steps, burst = 16, 6, 2
    scene_a, scene_b = moving_scene(0, n, steps), moving_scene(100, n, steps, dx=3, dy=2)
    dev_a = [torch.from_numpy(f).cuda() for f in scene_a]
    dev_b = [torch.from_numpy(f).cuda() for f in scene_b]
    origins = first_armour_origins(oracle, scene_a[0])
    trk_a = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    trk_a.set_origins(origins)
    trk_b = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, track_cap=16)
    refs_a, refs_b = ref_streams(n, (WW, WH), origins), ref_streams(n, (0, 0), np.zeros((n, 2), np.int32), cap=16)
    # (hot_contexts off: the per-stage getters of a ticket need its context untouched by the untracked batches' rotation)
    pl = Pipeline(device=0, hot_contexts=-1, max_frames=n, max_width=FW, max_height=FH)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
        c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
    full = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
    p = default_params()
    untracked_ref = None
    replay = []                                            # (requested origins before the step, frames, the tracked batch's record)
    for k0 in range(0, steps, burst):
        tickets = []
        for k in range(k0, k0 + burst):
            ts = (k + 1) * 8 * MS
            ta = pl.submit(dev_a[k].data_ptr(), n, FH, FW, p, full, tracker=trk_a, timestamp=ts)
            tu = pl.submit(dev_a[0].data_ptr(), n, FH, FW, p, STAGE_ALL)
            tb = pl.submit(dev_b[k].data_ptr(), n, FH, FW, p, STAGE_ALL, tracker=trk_b, timestamp=ts)
            tickets.append((k, ts, ta, tu, tb))
            assert pl.get_info().host_blocking_calls == 0
        for k, ts, ta, tu, tb in tickets:
            arm, offs = pl.collect(ta)
            ca = pl.context_of(ta)
            eff = ca.windows()[0]
            req = np.array([r.origin for r in refs_a], np.int32)
            assert np.array_equal(eff, W.effective_origins(req, FW, FH, WW, WH)), k    # step k - 1's origins, clamped and snapped
            feed(refs_a, arm, offs, ca.identities(), ca.poses()[2], eff, ts)
            replay.append((req, k, arm.tobytes(), offs.tobytes()))
            arm, offs = pl.collect(tb)
            feed(refs_b, arm, offs, None, None, np.zeros((n, 2), np.int32), ts)
            arm, offs = pl.collect(tu)                      # the untracked batches: the same frames every time, the same record every time
            if untracked_ref is None:
                untracked_ref = (arm.tobytes(), offs.tobytes())
            assert (arm.tobytes(), offs.tobytes()) == untracked_ref
        same(trk_a, refs_a)                                 # after the burst: both trackers are where their references are
        same(trk_b, refs_b)
    assert sum(int((r.tracks["initialized"] == 1).sum()) for r in refs_a) > 0 and all(len(r.tracks) for r in refs_a + refs_b)
    assert any(r.origin != tuple(origins[f]) for f, r in enumerate(refs_a))
    # the records of the tracked batches are those of submit_windows given the same origins from the host
    for req, k, arm_b, offs_b in replay[::2]:
        d_req = torch.from_numpy(req).cuda()
        t = pl.submit(dev_a[k].data_ptr(), n, FH, FW, p, full, windows=(d_req.data_ptr(), WW, WH), keepalive=d_req)
        arm, offs = pl.collect(t)
        assert arm.tobytes() == arm_b and offs.tobytes() == offs_b, k
    assert pl.get_info().host_blocking_calls == 0
    # refusals of the tracked submit come before anything is enqueued
    for kw, args, text in ((dict(n_streams=n + 1, frame_w=FW, frame_h=FH), (n, FH, FW, p, STAGE_ALL), "n_streams"),
                           (dict(n_streams=n, frame_w=640, frame_h=480), (n, FH, FW, p, STAGE_ALL), "frame size"),
                           (dict(n_streams=n, frame_w=FW, frame_h=FH), (n, FH, FW, p, STAGE_BINARY), "RMCV_STAGE_ARMOURS")):
        t = Tracker(device=0, **kw)
        with pytest.raises(RmcvError) as e:
            pl.submit(dev_a[0].data_ptr(), *args, tracker=t, timestamp=1)
        assert e.value.code == abi.ERR_BAD_ARG and text in str(e.value), str(e.value)
        t.close()
    # destroy with work in flight drains first
    pl.submit(dev_a[0].data_ptr(), n, FH, FW, p, full, tracker=trk_a, timestamp=99 * MS)
    pl.close()
    trk_a.close()
    trk_b.close()


# ---------------------------------------------------------------- 4. the object's tables, without a kernel
def test_tables_before_first_use_switched_tables_and_put_get():
    """what the getters hand out of tables that have never been allocated, a refused setter, every switched table on, off and on again, and
    a list put and read back: host calls and copies only, no launch"""
    from rmcv_amd import CAMP_RED, default_aim_config
    n = 3
    trk = Tracker(device=0, n_streams=n, track_cap=2, frame_w=FW, frame_h=FH)
    # never used: what the tables would hold
    att, err = trk.attitudes()
    assert trk.aims().tobytes() == bytes(72 * n) and att.tobytes() == bytes(24 * n) and err.tolist() == [0] * n
    want = np.zeros(n, abi.AIM_INPUT)
    want["world2camera"] = np.eye(4)
    assert trk.aim_inputs().tobytes() == want.tobytes() and want.nbytes == 136 * n
    camps_before = trk.device_camps()
    cfgs = [default_aim_config(v0=10.0 + f) for f in range(n)]
    with pytest.raises(RmcvError) as e:
        trk.set_aim_configs(cfgs)
    assert e.value.code == abi.ERR_BAD_ARG and "aiming is off" in str(e.value)
    assert [c.tolist() for c in trk.counts()] == [[0] * n, [0] * n]          # (still usable)
    # every switched table on, off, on: a tracked submit takes the tracker's own two tables whatever was switched meanwhile
    trk.set_aim()
    trk.set_aim_configs(cfgs)
    trk.set_aim_configs(None)
    trk.set_aim_configs(cfgs)
    trk.set_stream_cameras(np.tile(np.eye(4).reshape(16), (n, 1)))
    trk.set_stream_cameras(None)
    trk.set_camps([CAMP_BLUE, CAMP_RED, CAMP_BLUE], [100, 110, 120])
    trk.set_camps(None)
    assert trk.device_camps() == camps_before and all(camps_before)
    assert trk.aims().tobytes() == bytes(72 * n) and trk.aim_inputs().tobytes() == want.tobytes()   # (allocated now: zero records, the defaults)
    # a list goes in and comes back byte for byte; no side records given: zeros
    two = np.frombuffer(np.random.default_rng(5).integers(0, 256, 2 * abi.TRACK.itemsize, dtype=np.uint8).tobytes(), abi.TRACK).copy()
    trk.put(1, two)
    tr, side, _ = trk.get(1)
    assert tr.tobytes() == two.tobytes() and side.tobytes() == bytes(2 * 8 * 4)
    assert trk.counts()[0].tolist() == [0, 2, 0] and len(trk.get(0)[0]) == len(trk.get(2)[0]) == 0
    trk.close()
