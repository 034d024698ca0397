"""The per-stream gimbal attitude on the GPU (k_attitude in front of a tracked batch; rmcv_tracker_set_attitude, rmcv_batch_attitude,
rmcv_pipeline_submit_tracked_serial): every byte the step writes equals tests/attitude_ref.c; the closed loop with packets in equals the
loop driven through rmcv_batch_set_base2gripper / rmcv_tracker_set_aim_inputs / rmcv_tracker_set_camps from the host, byte for byte.  Every
GPU step runs once, with the library's deadlines as they are."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import attitude_cases as K
import attitude_ref as R
import window_ref as W
from rmcv_amd import (CAMP_BLUE, CAMP_RED, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Context, Pipeline, RmcvError, Tracker, abi, default_aim_config,
                      default_attitude_config, default_params, default_pnp_config, synth)
from test_gpu_aim import FH, FW, MS, WH, WW, moving_scene

pytestmark = pytest.mark.gpu


def device_array(a):
    """a host array in device memory (a torch tensor: keep it alive while the library borrows it)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def download(d_ptr, dtype, n):
    out = np.zeros(n, dtype)
    assert abi.lib().rmcv_device_download(0, abi.ptr(out), C.c_void_p(d_ptr), C.c_int64(out.nbytes)) == 0
    return out


# ---------------------------------------------------------------- 1. the kernel's corners without pixels
@pytest.mark.parametrize("n", [1, 5, 64, 65, 130])   # one lane; a partial workgroup; a full one; one lane into the second; a partial third
def test_every_byte_of_every_stream(n):
    c = Context(device=0, max_frames=n, max_width=64, max_height=64)
    c.pnp_load()
    c.upload(np.zeros((n, 1, 1, 3), np.uint8))                             # the smallest geometry there is: the step reads no pixel
    p1, p2 = K.packets(n, 41)[0], K.packets(n, 42, shift=3)[0]
    d1, d2 = device_array(p1), device_array(p2)
    for camps_on, mode in itertools.product((False, True), (abi.ATT_MOTOR_KEEP, abi.ATT_MOTOR_PITCH)):
        trk = Tracker(device=0, n_streams=n, track_cap=1, frame_w=1, frame_h=1)
        assert trk.attitudes()[0].tobytes() == bytes(24 * n) and trk.aim_inputs()["world2camera"].tobytes() == np.tile(np.eye(4), (n, 1, 1)).tobytes()
        with pytest.raises(RmcvError) as e:
            c.attitude(trk, d1.data_ptr())                                  # attitude is off
        assert e.value.code == abi.ERR_BAD_ARG and "off" in str(e.value)
        cfg = trk.set_attitude(motor_angle_mode=mode, gripper2camera=K.gripper2camera(43) if camps_on else np.array(default_pnp_config().gripper2camera))
        att, camps, inp = K.start_tables(n, 44)
        err = np.zeros(n, np.int32)
        trk.set_attitudes(att)
        trk.set_aim_inputs(inp)
        if camps_on:
            trk.set_camps(camps)
        d_camps = trk.device_camps()[0]
        for rnd, (pk, dev) in enumerate(((p1, d1), (p2, d2), (None, None))):
            if pk is None:                                                  # no packets: the table as the host has just set it
                att = K.start_tables(n, 45)[0]
                trk.set_attitudes(att)
            c.attitude(trk, None if dev is None else dev.data_ptr())
            att, new_camps, err, b2g, inp = R.tables(cfg, pk, att, camps if camps_on else None, err, inp)
            got_att, got_err = trk.attitudes()
            assert got_att.tobytes() == att.tobytes() and got_err.tolist() == err.tolist(), (camps_on, mode, rnd)
            assert c.base2gripper().tobytes() == b2g.tobytes(), (camps_on, mode, rnd)
            assert trk.aim_inputs().tobytes() == inp.tobytes(), (camps_on, mode, rnd)
            got_camps = download(d_camps, np.int32, n)
            if camps_on:
                camps = new_camps
                assert got_camps.tolist() == camps.tolist()
            else:
                assert not got_camps.any()                                  # the table is off: never written
        assert err.sum() > 0 or n == 1
        trk.close()
    # a context without pose tables: the step runs, nothing of the context is written
    bare = Context(device=0, max_frames=n, max_width=64, max_height=64)
    bare.upload(np.zeros((n, 1, 1, 3), np.uint8))
    trk = Tracker(device=0, n_streams=n, track_cap=1, frame_w=1, frame_h=1)
    cfg = trk.set_attitude()
    bare.attitude(trk, d1.data_ptr())
    want = R.tables(cfg, p1, np.zeros(n, abi.ATTITUDE), None, np.zeros(n, np.int32), trk_defaults(n), base2gripper=False)
    assert trk.attitudes()[0].tobytes() == want[0].tobytes() and trk.aim_inputs().tobytes() == want[4].tobytes()
    with pytest.raises(RmcvError):
        bare.base2gripper()
    if n > 1:                                                               # frame f is stream f: the counts must agree
        c.upload(np.zeros((n - 1, 1, 1, 3), np.uint8))
        with pytest.raises(RmcvError) as e:
            c.attitude(trk, d1.data_ptr())
        assert e.value.code == abi.ERR_BAD_ARG and "streams" in str(e.value)
    for broken in (dict(motor_angle_mode=2), dict(gripper2camera=np.full(16, math.nan))):
        with pytest.raises(RmcvError) as e:
            trk.set_attitude(**broken)
        assert e.value.code == abi.ERR_BAD_ARG and "attitude config" in str(e.value)
    assert c.check_guards()[0] == 0 and bare.check_guards()[0] == 0
    trk.close()
    bare.close()
    c.close()


def trk_defaults(n):
    a = np.zeros(n, abi.AIM_INPUT)
    a["world2camera"] = np.eye(4)
    return a


# ---------------------------------------------------------------- 2. / 3. / 4. the closed loop with packets in
N, STEPS = 4, 4
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
REJECTED = (1, 2)    # (step, stream): a packet with a broken CRC -- the stream keeps step 0's attitude
RED = (2, 3)         # (step, stream): a valid packet that says the enemy is red -- the blue scene then shows that stream nothing


def loop_aim():
    return default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, lead_iterations=1)


def loop_attitude():
    return default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH)


def loop_packets():
    """per step (N, 24) uint8: every stream's yaw, pitch and roll change every step"""
    out = []
    for k in range(STEPS):
        pk = []
        for f in range(N):
            p = bytearray(K.py_packet(1 if (k, f) == RED else 0, 4.0 * (k + 1) + 11.0 * f, -2.5 * k + 3.0 * f - 4.0, 1.5 * k - 2.0 * f))
            if (k, f) == REJECTED:
                p[23] ^= 0x40
            pk.append(bytes(p))
        out.append(np.frombuffer(b"".join(pk), np.uint8).reshape(N, 24).copy())
    return out


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
def reference_tables():
    """per step what the reference leaves: (attitudes, camps, packet_errors, base2gripper, aim inputs)"""
    att, camps, err, inp = np.zeros(N, abi.ATTITUDE), np.full(N, CAMP_BLUE, np.int32), np.zeros(N, np.int32), trk_defaults(N)
    out = []
    for pk in loop_packets():
        att, camps, err, b2g, inp = R.tables(loop_attitude(), pk, att, camps, err, inp)
        out.append((att, camps, err, b2g, inp))
    return out


def new_tracker(origins):
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    trk.set_origins(origins)
    trk.set_aim(loop_aim())
    trk.set_camps(np.full(N, CAMP_BLUE, np.int32))
    return trk


def new_context():
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    return c


def state(trk):
    return trk.aims(), [trk.get(f) for f in range(N)], trk.counts()


def same_state(a, b):
    if a[0].tobytes() != b[0].tobytes() or a[2][0].tolist() != b[2][0].tolist() or a[2][1].tolist() != b[2][1].tolist():
        return False
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2] for x, y in zip(a[1], b[1]))


def context_step(c, trk, frames, k):
    c.upload(frames[k])
    c.set_windows(trk.device_origins(), WW, WH)
    c.set_frame_camps(trk.device_camps()[0])


@pytest.fixture(scope="module")
def run_a(scene, reference_tables):
    """Context.attitude(trk, packets) in front of every run: per step the tracker's state"""
    frames, origins = scene
    trk, c = new_tracker(origins), new_context()
    trk.set_attitude(loop_attitude())
    dev = [device_array(p) for p in loop_packets()]
    out = []
    for k in range(STEPS):
        context_step(c, trk, frames, k)
        c.attitude(trk, dev[k].data_ptr())
        c.run(default_params(), FULL)
        c.track(trk, (k + 1) * 8 * MS)
        c.sync()
        att, camps, err, b2g, inp = reference_tables[k]
        got_att, got_err = trk.attitudes()
        assert got_att.tobytes() == att.tobytes() and got_err.tolist() == err.tolist()
        assert c.base2gripper().tobytes() == b2g.tobytes() and trk.aim_inputs().tobytes() == inp.tobytes()
        assert download(trk.device_camps()[0], np.int32, N).tolist() == camps.tolist()
        out.append(state(trk))
    assert c.check_guards()[0] == 0
    c.close()
    trk.close()
    return out


def test_context_closed_loop_equals_the_host_driven_one(scene, reference_tables, run_a):
    frames, origins = scene
    # run B, the API as it was: the reference's matrices, inputs and camps set from the host in front of every run
    trk, c = new_tracker(origins), new_context()
    for k in range(STEPS):
        att, camps, err, b2g, inp = reference_tables[k]
        context_step(c, trk, frames, k)
        c.set_base2gripper(b2g)
        trk.set_aim_inputs(inp)
        trk.set_camps(camps)
        c.run(default_params(), FULL)
        c.track(trk, (k + 1) * 8 * MS)
        c.sync()
        assert same_state(state(trk), run_a[k]), k                          # every rmcv_track, every count, every rmcv_aim
    c.close()
    trk.close()
    # the rejected packet was counted and skipped; the red one blinded its stream for a step
    assert reference_tables[-1][2].tolist() == [1 if f == REJECTED[1] else 0 for f in range(N)]
    assert reference_tables[REJECTED[0]][0][REJECTED[1]].tobytes() == reference_tables[REJECTED[0] - 1][0][REJECTED[1]].tobytes()
    assert reference_tables[RED[0]][1].tolist() == [CAMP_RED if f == RED[1] else CAMP_BLUE for f in range(N)]
    assert all(len(t[0]) for t in run_a[-1][1]) and (run_a[-1][0]["track"] >= 0).all()
    # an identity-attitude run (one step is enough) puts the same armours elsewhere: the attitude reached the filter
    trk, c = new_tracker(origins), new_context()
    context_step(c, trk, frames, 0)
    c.run(default_params(), FULL)
    c.track(trk, 8 * MS)
    c.sync()
    for f in range(N):
        ident, turned = trk.get(f)[0], run_a[0][1][f][0]
        assert len(ident) == len(turned) > 0 and ident["armour"].tobytes() == turned["armour"].tobytes()
        assert (ident["position"] != turned["position"]).any()
        # ... by exactly the rotation: |p| is the same to rounding
        assert np.allclose(np.linalg.norm(ident["position"], axis=1), np.linalg.norm(turned["position"], axis=1), rtol=1e-12, atol=0)
    c.close()
    trk.close()


# ---------------------------------------------------------------- 3. pipeline burst, host only submits
def new_pipeline():
    pl = Pipeline(device=0, max_frames=N, max_width=FW, max_height=FH)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
        c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
    return pl


def plain_tracker(origins):
    """a tracker that knows nothing of this feature: aiming on, today's inputs for a pipeline (gripper frame)"""
    t = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    t.set_origins(origins)
    t.set_aim(loop_aim())
    a = trk_defaults(N)
    a["world2camera"] = abi.rigid_inverse(np.array(default_pnp_config().gripper2camera).reshape(4, 4))
    t.set_aim_inputs(a)
    return t


def burst(pl, dev, trackers, packets):
    """STEPS submits per tracker, interleaved, nothing collected in between"""
    p = default_params()
    for k in range(STEPS):
        for t, pk in zip(trackers, packets):
            pl.submit(dev[k].data_ptr(), N, FH, FW, p, FULL, tracker=t, timestamp=(k + 1) * 8 * MS, packets=None if pk is None else pk[k].data_ptr())
    pl.drain()
    assert pl.get_info().host_blocking_calls == 0


@pytest.fixture(scope="module")
def device_frames(scene):
    return [device_array(f) for f in scene[0]]


def test_pipeline_burst_packets_in_aims_out(scene, device_frames, run_a, reference_tables):
    _, origins = scene
    # without this feature's calls: one plain tracker on a pipeline of its own
    pl, base = new_pipeline(), plain_tracker(origins)
    burst(pl, device_frames, [base], [None])
    want_plain = state(base)
    pl.close()
    base.close()
    # the burst: a tracker with attitude on, each step's packets in a device tensor of their own, interleaved with a plain tracker
    pl, trk, off = new_pipeline(), new_tracker(origins), plain_tracker(origins)
    trk.set_attitude(loop_attitude())
    pk = [device_array(p) for p in loop_packets()]
    burst(pl, device_frames, [trk, off], [pk, None])
    assert same_state(state(trk), run_a[-1])                                # final tracks and aims: run A's
    att, camps, err, b2g, inp = reference_tables[-1]
    assert trk.attitudes()[0].tobytes() == att.tobytes() and trk.attitudes()[1].tolist() == err.tolist() and trk.aim_inputs().tobytes() == inp.tobytes()
    assert same_state(state(off), want_plain)                               # the plain tracker beside it: as if the feature were not there
    assert off.attitudes()[0].tobytes() == bytes(24 * N)
    pl.close()
    trk.close()
    off.close()


def test_submit_without_packets_uses_the_table(scene, device_frames, reference_tables):
    """rmcv_pipeline_submit_tracked on a tracker with attitude on is _serial with no packets: the attitudes a host (or a device-side producer)
    has put into the table; whole-frame tracker, so the wait for the previous step is the attitude step's own"""
    _, origins = scene
    att = reference_tables[0][0]
    pl = new_pipeline()
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH)
    trk.set_aim(loop_aim())
    cfg = trk.set_attitude(loop_attitude())
    trk.set_attitudes(att)
    p = default_params()
    for k in range(2):
        pl.submit(device_frames[k].data_ptr(), N, FH, FW, p, FULL, tracker=trk, timestamp=(k + 1) * 8 * MS)
    pl.drain()
    assert pl.get_info().host_blocking_calls == 0
    want = R.tables(cfg, None, att, None, np.zeros(N, np.int32), trk_defaults(N))
    assert trk.aim_inputs().tobytes() == want[4].tobytes() and trk.attitudes()[0].tobytes() == att.tobytes()
    # the same two steps with the matrices and inputs set from the host
    ref = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH)
    ref.set_aim(loop_aim())
    ref.set_aim_inputs(want[4])
    pl2 = new_pipeline()
    for c in pl2.contexts:
        c.set_base2gripper(want[3])
    for k in range(2):
        pl2.submit(device_frames[k].data_ptr(), N, FH, FW, p, FULL, tracker=ref, timestamp=(k + 1) * 8 * MS)
    pl2.drain()
    assert same_state(state(trk), state(ref))
    assert all(len(trk.get(f)[0]) for f in range(N))
    for x in (pl, pl2, trk, ref):
        x.close()


# ---------------------------------------------------------------- 4. refusals leave the pipeline usable
def test_refusals_leave_the_pipeline_usable(scene, device_frames, run_a):
    _, origins = scene
    pl, trk, off = new_pipeline(), new_tracker(origins), plain_tracker(origins)
    pk = [device_array(p) for p in loop_packets()]
    p = default_params()

    def refused(what, **kw):
        before = pl.get_info().submitted
        with pytest.raises(RmcvError) as e:
            pl.submit(**kw)
        assert e.value.code == abi.ERR_BAD_ARG and what in str(e.value), str(e.value)
        assert pl.get_info().submitted == before

    frames0 = device_frames[0].data_ptr()
    # packets given and attitude off (never set; and set, then turned off again)
    refused("attitude is off", data_ptr=frames0, n=N, h=FH, w=FW, params=p, stages=FULL, tracker=off, timestamp=8 * MS, packets=pk[0].data_ptr())
    refused("attitude is off", data_ptr=frames0, n=N, h=FH, w=FW, params=p, stages=FULL, tracker=trk, timestamp=8 * MS, packets=pk[0].data_ptr())
    trk.set_attitude(loop_attitude())
    trk.set_attitude(None)
    refused("attitude is off", data_ptr=frames0, n=N, h=FH, w=FW, params=p, stages=FULL, tracker=trk, timestamp=8 * MS, packets=pk[0].data_ptr())
    # a config that is refused leaves attitude as it was: off
    for broken in (dict(motor_angle_mode=-1), dict(gripper2camera=[math.inf] + [0.0] * 15)):
        with pytest.raises(RmcvError):
            trk.set_attitude(**broken)
    refused("attitude is off", data_ptr=frames0, n=N, h=FH, w=FW, params=p, stages=FULL, tracker=trk, timestamp=8 * MS, packets=pk[0].data_ptr())
    trk.set_attitude(loop_attitude())
    # n_frames != n_streams
    refused("n_streams", data_ptr=frames0, n=N - 1, h=FH, w=FW, params=p, stages=FULL, tracker=trk, timestamp=8 * MS, packets=pk[0].data_ptr())
    for k in range(STEPS):
        pl.submit(device_frames[k].data_ptr(), N, FH, FW, p, FULL, tracker=trk, timestamp=(k + 1) * 8 * MS, packets=pk[k].data_ptr())
        if k == 1:                                                          # ... and in the middle of the burst
            refused("n_streams", data_ptr=frames0, n=N - 1, h=FH, w=FW, params=p, stages=FULL, tracker=trk, timestamp=8 * MS, packets=pk[0].data_ptr())
            refused("attitude is off", data_ptr=frames0, n=N, h=FH, w=FW, params=p, stages=FULL, tracker=off, timestamp=8 * MS, packets=pk[0].data_ptr())
    pl.drain()
    assert pl.get_info().host_blocking_calls == 0
    assert same_state(state(trk), run_a[-1])                                # the accepted submits' result is run A's
    assert trk.attitudes()[1].tolist() == [1 if f == REJECTED[1] else 0 for f in range(N)]   # (a refused submit decoded nothing)
    for x in (pl, trk, off):
        x.close()
