"""Device-resident aiming on the GPU (k_aim behind the tracker's step; rmcv_tracker_set_aim / _aim / _get_aims / _put): every stream's
rmcv_aim equals -- byte for byte -- tests/aim_ref.c fed with the stream's tracks.  Seeded lists reach the kernel's corners without pixels;
the context and pipeline paths run the closed loop with aiming on.  Every GPU step runs once, with the library's deadlines as they are."""
import numpy as np
import pytest

import aim_cases as K
import aim_ref as R
import window_ref as W
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Context, Pipeline, RmcvError, Tracker, default_aim_config, default_params,
                      default_pnp_config, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

FW, FH, WW, WH = 1280, 1024, 512, 384
MS = K.MS


def expect(cfg, lists, inputs, now):
    """AIM[n]: the reference's record of every stream"""
    return np.array([R.step(cfg, K.TICK, tr, now, None if inputs is None else inputs[f:f + 1])[0] for f, tr in enumerate(lists)], abi.AIM)


# ---------------------------------------------------------------- 1. the kernel's corners without pixels
@pytest.mark.parametrize("cap,names", [(64, ("empty", "one_id7", "tie63", "tie64_last_wins", "mixed7")), (5, ("empty", "five", "three"))])
def test_seeded_lists_every_configuration(cap, names):
    L = K.lists()
    lists = [L[n] for n in names]
    assert [len(t) for t in lists] == ([0, 1, 63, 64, 7] if cap == 64 else [0, 5, 3])
    trk = Tracker(device=0, n_streams=len(lists), track_cap=cap, frame_w=FW, frame_h=FH)
    assert trk.aims().tobytes() == bytes(72 * len(lists))                  # zero until the first step, aiming never set
    with pytest.raises(RmcvError) as e:
        trk.aim(K.NOW)                                                      # aiming is off
    assert e.value.code == abi.ERR_BAD_ARG
    for f, tr in enumerate(lists):
        trk.put(f, tr)
        got = trk.get(f)[0]
        assert got.tobytes() == tr.tobytes()
    if cap == 5:
        with pytest.raises(RmcvError) as e:
            trk.put(0, L["mixed7"])                                         # 7 > track_cap
        assert e.value.code == abi.ERR_CAPACITY
    inputs = K.aim_inputs(len(lists))
    seen = set()
    for use_inputs in (None, inputs, K.aim_inputs_huge(len(lists))):         # ... and a motor angle whose tangent is NaN by pinned_math.h's rule
        trk.set_aim_inputs(use_inputs)
        for name, cfg in K.configs().items():
            trk.set_aim(cfg)
            trk.aim(K.NOW)
            got = trk.aims()
            want = expect(cfg, lists, use_inputs, K.NOW)
            assert got.tobytes() == want.tobytes(), (name, use_inputs is not None, got, want)
            seen |= {(int(a["track"]), int(a["status"])) for a in got}
    if cap == 64:
        tracks = {t for t, _ in seen}
        assert {-1, 0, 63} <= tracks                                        # no target; the tie's lowest index; the winner in the last lane
        assert any(s == abi.AIM_NO_SOLUTION for _, s in seen) and any(s == 0 and t >= 0 for t, s in seen)
        # the stream whose only candidate is masked out (identity 7) has no target under the masked configurations, one without the mask
        trk.set_aim(K.configs()["p0_s0_h0_l1"])
        trk.aim(K.NOW)
        assert trk.aims()[1]["status"] == abi.AIM_NO_TARGET
        trk.set_aim(K.configs()["defaults"])
        trk.aim(K.NOW)
        assert trk.aims()[1]["track"] == 0
    for f, tr in enumerate(lists):                                          # aiming reads and never writes
        assert trk.get(f)[0].tobytes() == tr.tobytes()
    with pytest.raises(RmcvError) as e:
        trk.set_aim(default_aim_config(mode=abi.COMPENSATE_NI))
    assert e.value.code == abi.ERR_BAD_ARG and "NI" in str(e.value)
    trk.close()


# ---------------------------------------------------------------- 2. / 3. / 4. the closed loop with aiming on
N, STEPS = 4, 4


def moving_scene(first, n, steps, dx=5, dy=3):
    base = synth.batch(first, n, FW, FH, CAMP_BLUE, 0, threads=16)
    out = []
    for k in range(steps):
        f = np.zeros_like(base)
        sx, sy = k * dx, k * dy
        f[:, sy:, sx:] = base[:, :FH - sy, :FW - sx]
        out.append(f)
    return out


def loop_config():
    return default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, lead_iterations=1)


def loop_inputs():
    """positions of a pipelined RMCV_STAGE_POSE are in the gripper's frame (base2gripper = identity): world2camera = gripper2camera^-1"""
    a = np.zeros(N, abi.AIM_INPUT)
    a["world2camera"] = abi.rigid_inverse(np.array(default_pnp_config().gripper2camera).reshape(4, 4))
    return a


@pytest.fixture(scope="module")
def scene(oracle):
    frames = moving_scene(0, N, STEPS)
    o = []
    for f in frames[0]:
        a = oracle.detect_frame(f, oracle.default_params())["armours"]
        assert len(a)
        o.append(W.window_origin(W.get_roi(a[0]["vertices"], (1.0, 1.0), (FW, FH)), WW, WH))
    return frames, np.array(o, np.int32)


@pytest.fixture(scope="module")
def context_path(scene):
    """the closed loop of test_gpu_tracker.py::test_context_closed_loop_windows_identity_pose with aiming on: per step (aims, tracks of every
    stream, timestamp)"""
    frames, origins = scene
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    trk.set_origins(origins)
    trk.set_aim(loop_config())
    trk.set_aim_inputs(loop_inputs())
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    out = []
    for k in range(STEPS):
        ts = (k + 1) * 8 * MS
        c.upload(frames[k])
        c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
        c.set_windows(trk.device_origins(), WW, WH)
        c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
        c.track(trk, ts)
        c.sync()
        out.append((trk.aims(), [trk.get(f)[0] for f in range(N)], ts))
    # 4. off is off: a further step moves the tracks and leaves the records alone
    trk.set_aim(None)
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    c.track(trk, (STEPS + 1) * 8 * MS)
    c.sync()
    after_off = (trk.aims(), [trk.get(f)[0] for f in range(N)])
    assert c.check_guards()[0] == 0
    c.close()
    trk.close()
    return out, after_off


def test_context_path_aims_equal_the_reference(context_path):
    steps, _ = context_path
    cfg, inputs = loop_config(), loop_inputs()
    unled_cfg = default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, lead_iterations=0)
    led = 0
    for aims, tracks, ts in steps:
        want = expect(cfg, tracks, inputs, ts)
        assert aims.tobytes() == want.tobytes(), (ts, aims, want)
        unled = expect(unled_cfg, tracks, inputs, ts)
        led += sum(1 for a, u in zip(aims, unled) if a["status"] == 0 and np.isfinite(a["point"]).all() and a["point"].tolist() != u["point"].tolist())
    assert all(len(t) for t in steps[-1][1]) and (steps[-1][0]["track"] >= 0).all()
    assert led > 0                                                          # a finite solution with a non-zero lead


def test_off_is_off(context_path):
    steps, (aims_after, tracks_after) = context_path
    assert aims_after.tobytes() == steps[-1][0].tobytes()                   # the records: byte-identical
    assert any(a.tobytes() != b.tobytes() for a, b in zip(tracks_after, steps[-1][1]))   # ... while the tracker stepped on


def test_pipeline_path_burst_with_aiming_on(scene, context_path):
    import torch
    frames, origins = scene
    steps, _ = context_path
    dev = [torch.from_numpy(f).cuda() for f in frames]
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    off = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    for t in (trk, off):
        t.set_origins(origins)
    trk.set_aim(loop_config())
    trk.set_aim_inputs(loop_inputs())
    pl = Pipeline(device=0, max_frames=N, max_width=FW, max_height=FH)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
        c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
    p, full = default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
    for k in range(STEPS):                                                  # a burst nobody collects in between: the host only submits
        pl.submit(dev[k].data_ptr(), N, FH, FW, p, full, tracker=trk, timestamp=(k + 1) * 8 * MS)
        pl.submit(dev[k].data_ptr(), N, FH, FW, p, full, tracker=off, timestamp=(k + 1) * 8 * MS)
    pl.drain()
    assert pl.get_info().host_blocking_calls == 0
    assert trk.aims().tobytes() == steps[-1][0].tobytes()                   # the context path's final aims
    assert off.aims().tobytes() == bytes(72 * N)                            # aiming off: the records stay zero ...
    for f in range(N):                                                      # ... and the tracks are the aimed tracker's: aiming never writes them
        a, b = trk.get(f), off.get(f)
        assert a[0].tobytes() == b[0].tobytes() == steps[-1][1][f].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    pl.close()
    trk.close()
    off.close()
