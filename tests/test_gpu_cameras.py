"""Per-stream camera model and ballistics on the GPU: the context's camera table selected per frame by k_pnp
(rmcv_pnp_load_cameras, rmcv_batch_set_[device_]frame_cameras, rmcv_pipeline_set_frame_cameras), the tracker's per-stream hand-eye matrices
in k_attitude (rmcv_tracker_set_stream_cameras) and per-stream aim configs in k_aim (rmcv_tracker_set_aim_configs).  Poses are held, byte
for byte, against oracle.locate_armours with each frame's camera; the attitude and aim steps against the per-stream host statements
(rmcv_attitude_step_host / rmcv_aim_step_host with stream f's matrix or config); the closed loop against the same loop run once per stream
through the single-config calls.  Every GPU step runs once, with the library's deadlines as they are."""
import numpy as np
import pytest

import aim_cases as AIMK
import attitude_cases as ATTK
import camera_cases as CK
import window_ref as W
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Context, Pipeline, RmcvError, Tracker, abi, default_aim_config,
                      default_attitude_config, default_params, default_pnp_config, synth)
from test_gpu_aim import FH, FW, MS, WH, WW, moving_scene
from test_gpu_attitude import device_array, loop_packets
from test_oracle_pnp import rodrigues
from test_gpu_window import crops_of, first_armour_origins

pytestmark = pytest.mark.gpu

POSE = STAGE_ALL | STAGE_POSE


def check_poses(c, oracle, cams, idx, mats, eff=None):
    """the context's batch (run and synced): frame f's rvec, tvec, position equal the oracle's with cams[idx[f]] (eff: the frames' window
    origins, added to the vertices in float as mobility.cpp:172 does); returns (armours, offsets, tvecs)"""
    arm, offs = c.armours()
    r, t, p = c.poses()
    assert len(r) == len(arm) > 0
    ocfg = [CK.to_oracle_cfg(oracle, cam) for cam in cams]
    for f in range(len(idx)):
        sl = slice(offs[f], offs[f + 1])
        a = arm[sl].copy()
        if eff is not None:
            a["vertices"] = a["vertices"] + eff[f].astype(np.float32)
        wr, wt, wp = oracle.locate_armours(a, ocfg[idx[f]], mats[f])
        assert r[sl].tobytes() == wr.tobytes() and t[sl].tobytes() == wt.tobytes(), (f, idx[f])
        assert p[sl].tobytes() == wp.tobytes(), (f, idx[f])
    return arm, offs, t


# ---------------------------------------------------------------- 1. / 2. the pose table
N_POSE = 6
IDX = [2, 0, 1, 1, 2, 0]     # no frame's index is its own number


@pytest.fixture(scope="module")
def pose_scene():
    """tests/test_gpu_pnp.py::test_batch_pose_stage's own: frames, per-frame base2gripper; and the three cameras"""
    frames = synth.batch(900, N_POSE, 1280, 1024, CAMP_BLUE, 0)
    rng = np.random.default_rng(2)
    mats = np.tile(np.eye(4), (N_POSE, 1, 1))
    for f in range(N_POSE):
        mats[f, :3, :3] = rodrigues(rng.uniform(-1, 1, 3))
        mats[f, :3, 3] = rng.uniform(-50, 50, 3)
    return frames, mats, [default_pnp_config(), CK.other_camera(), CK.moved_camera(203)]


def pose_context(scene):
    frames, mats, cams = scene
    c = Context(device=0, max_frames=N_POSE, max_width=1280, max_height=1024)
    c.pnp_load_cameras(cams)
    c.upload(frames)
    c.set_base2gripper(mats)
    return c


def run_pose(c):
    c.run(default_params(), POSE)
    c.sync()


def test_pose_table(pose_scene, oracle):
    frames, mats, cams = pose_scene
    c = pose_context(pose_scene)
    assert c.frame_cameras().tolist() == [0] * N_POSE                      # selection is off until it is set
    c.set_frame_cameras(IDX)
    run_pose(c)
    arm, offs, t = check_poses(c, oracle, cams, IDX, mats)
    assert c.frame_cameras().tolist() == IDX
    # every camera serves a frame with an armour, and the cameras tell: another lens moves tvec, another mount the position alone
    assert all(any(offs[f + 1] > offs[f] for f in range(N_POSE) if IDX[f] == k) for k in range(3))
    o = [CK.to_oracle_cfg(oracle, cam) for cam in cams]
    one = arm[:1]
    assert oracle.locate_armours(one, o[0], mats[0])[1].tobytes() != oracle.locate_armours(one, o[1], mats[0])[1].tobytes()
    assert oracle.locate_armours(one, o[0], mats[0])[1].tobytes() == oracle.locate_armours(one, o[2], mats[0])[1].tobytes()
    assert oracle.locate_armours(one, o[0], mats[0])[2].tobytes() != oracle.locate_armours(one, o[2], mats[0])[2].tobytes()
    # selection off: every frame through camera 0
    c.set_frame_cameras(None)
    run_pose(c)
    check_poses(c, oracle, cams, [0] * N_POSE, mats)
    assert c.frame_cameras().tolist() == [0] * N_POSE
    # a new binding returns to off
    c.set_frame_cameras(IDX)
    c.upload(frames)
    c.set_base2gripper(mats)
    run_pose(c)
    check_poses(c, oracle, cams, [0] * N_POSE, mats)
    # rmcv_pnp_load: a table of one, selection off -- what the batch gave before there were tables
    c.set_frame_cameras(IDX)
    c.pnp_load(default_pnp_config())
    run_pose(c)
    check_poses(c, oracle, cams[:1], [0] * N_POSE, mats)
    assert c.frame_cameras().tolist() == [0] * N_POSE
    # the stage-wise call uses camera 0 whatever the frames' cameras are
    c.pnp_load_cameras(cams[::-1])
    c.set_frame_cameras(IDX)
    got = c.locate_armours(arm[:3], mats[1])
    want = oracle.locate_armours(arm[:3], o[2], mats[1])
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    with pytest.raises(RmcvError) as e:
        c.pnp_load_cameras(cams * 3)                                        # 9 cameras, 6 frame slots
    assert e.value.code == abi.ERR_BAD_ARG and "n_cameras" in str(e.value)
    assert c.check_guards()[0] == 0
    c.close()


def test_device_table_with_stray_values(pose_scene, oracle):
    frames, mats, cams = pose_scene
    stray = [-1, 3, 2**31 - 1, 1, 2, -2**31]
    eff = [0, 0, 0, 1, 2, 0]
    assert [abi.frame_camera(i, 3) for i in stray] == eff
    c = pose_context(pose_scene)
    # the host setter refuses the list, and the table it had stays in force
    c.set_frame_cameras(IDX)
    with pytest.raises(RmcvError) as e:
        c.set_frame_cameras(stray)
    assert e.value.code == abi.ERR_BAD_ARG and "camera" in str(e.value) and "frame 0" in str(e.value)
    run_pose(c)
    check_poses(c, oracle, cams, IDX, mats)
    assert c.frame_cameras().tolist() == IDX
    # in device memory any value may stand: the rule makes it an entry of the table
    d = device_array(np.array(stray, np.int32))
    c.set_frame_cameras(d.data_ptr(), keepalive=d)
    run_pose(c)
    check_poses(c, oracle, cams, eff, mats)
    assert c.frame_cameras().tolist() == eff
    # borrowed: the next run reads it again
    d[3] = 7
    d[0] = 2
    import torch
    torch.cuda.synchronize()
    run_pose(c)
    check_poses(c, oracle, cams, [2, 0, 0, 0, 2, 0], mats)
    assert c.frame_cameras().tolist() == [2, 0, 0, 0, 2, 0]
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 3. windows
def test_cameras_on_windows(oracle):
    n, fw, fh, ww, wh = 4, 1920, 1200, 512, 384
    frames = synth.batch(400, n, fw, fh, CAMP_BLUE, 0, threads=4)
    origins, _ = first_armour_origins(oracle, frames, ww, wh)
    cams, idx = [default_pnp_config(), CK.other_camera()], [1, 0, 0, 1]
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    c.pnp_load_cameras(cams)
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    c.set_frame_cameras(idx)
    mats = np.tile(np.eye(4), (n, 1, 1))
    c.set_base2gripper(mats)
    run_pose(c)
    eff = W.effective_origins(origins, fw, fh, ww, wh)
    assert np.array_equal(c.windows()[0], eff) and eff.any()
    arm, offs, _ = check_poses(c, oracle, cams, idx, mats, eff)
    crops = crops_of(frames, eff, ww, wh)
    for f in range(n):                                                      # (the armours are the crops')
        assert arm[offs[f]:offs[f + 1]].tobytes() == oracle.detect_frame(crops[f], oracle.default_params())["armours"].tobytes()
    assert all(any(offs[f + 1] > offs[f] for f in range(n) if idx[f] == k) for k in range(2))   # both cameras located something
    assert c.frame_cameras().tolist() == idx
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 4. pipeline
def test_pipeline_sticky_table(oracle):
    n, w, h = 4, 512, 640
    cams, idx = CK.fleet(3), [2, 0, 1, 1]
    batches = [synth.batch(first, n, w, h, CAMP_BLUE, 0) for first in (900, 30, 31)]
    # the context path
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.pnp_load_cameras(cams)
    want = []
    for fr in batches:
        c.upload(fr)
        c.set_frame_cameras(idx)
        run_pose(c)
        check_poses(c, oracle, cams, idx, np.tile(np.eye(4), (n, 1, 1)))
        want.append((c.armours()[0].tobytes(),) + tuple(x.tobytes() for x in c.poses()))
    c.close()
    assert len(set(want)) == 3

    def got(pl, t):
        pl.wait(t)
        cc = pl.context_of(t)
        assert cc.frame_cameras().tolist() == idx
        return (cc.armours()[0].tobytes(),) + tuple(x.tobytes() for x in cc.poses())

    pl = Pipeline(device=0, depth=2, max_frames=n, max_width=w, max_height=h)
    for cc in pl.contexts:
        cc.pnp_load_cameras(cams)
    dev = [device_array(fr) for fr in batches]
    d_idx = device_array(np.array(idx, np.int32))
    pl.set_frame_cameras(d_idx.data_ptr(), n, keepalive=d_idx)             # once: it sticks
    p = default_params()
    t0 = pl.submit(dev[0].data_ptr(), n, h, w, p, POSE)
    t1 = pl.submit(dev[1].data_ptr(), n, h, w, p, POSE)
    assert got(pl, t0) == want[0]
    t2 = pl.submit(dev[2].data_ptr(), n, h, w, p, POSE)                    # the ring wraps: slot 0 again
    assert got(pl, t1) == want[1] and got(pl, t2) == want[2]
    assert pl.get_info().host_blocking_calls == 0

    def refused(what, n_frames):
        before = pl.get_info().submitted
        with pytest.raises(RmcvError) as e:
            pl.submit(dev[0].data_ptr(), n_frames, h, w, p, POSE)
        assert e.value.code == abi.ERR_BAD_ARG and what in str(e.value), str(e.value)
        assert pl.get_info().submitted == before

    # a pose submit whose n_frames is not the table's (a submit without the pose stage does not read the table: accepted)
    refused("camera table", n - 1)
    t = pl.submit(dev[0].data_ptr(), n - 1, h, w, p, STAGE_ALL)
    pl.wait(t)
    t = pl.submit(dev[1].data_ptr(), n, h, w, p, POSE)
    assert got(pl, t) == want[1]
    # one slot with another n_cameras
    pl.drain()
    pl.contexts[1].pnp_load_cameras(cams[:2])
    refused("n_cameras differs", n)
    pl.contexts[1].pnp_load_cameras(cams)
    ts = [pl.submit(dev[k].data_ptr(), n, h, w, p, POSE) for k in (2, 0)]
    assert got(pl, ts[0]) == want[2] and got(pl, ts[1]) == want[0]
    # off again: camera 0 for every frame
    pl.set_frame_cameras(None)
    t = pl.submit(dev[0].data_ptr(), n, h, w, p, POSE)
    pl.wait(t)
    cc = pl.context_of(t)
    check_poses(cc, oracle, cams, [0] * n, np.tile(np.eye(4), (n, 1, 1)))
    assert cc.frame_cameras().tolist() == [0] * n
    assert pl.get_info().host_blocking_calls == 0
    assert all(cc.check_guards()[0] == 0 for cc in pl.contexts)
    pl.close()


# ---------------------------------------------------------------- 5. k_attitude and k_aim corners without pixels
def host_statements(att_cfgs, aim_cfgs, packets, att, err, inp, lists):
    """what the per-stream host statements leave: (attitudes, errors, base2gripper, aim inputs, aims)"""
    n = len(lists)
    o_att, o_err, o_inp = att.copy(), err.copy(), inp.copy()
    b2g, aims = np.zeros((n, 4, 4)), np.zeros(n, abi.AIM)
    for f in range(n):
        a, _, e, b, i = Tracker.attitude_host(att_cfgs[f], None if packets is None else packets[f].tobytes(), att[f:f + 1], None, int(err[f]), inp[f:f + 1])
        o_att[f], o_err[f], o_inp[f], b2g[f] = a, e, i, b
        aims[f] = Tracker.aim_host(aim_cfgs[f], AIMK.TICK, lists[f], AIMK.NOW, (i["world2camera"], float(i["motor_angle"])))
    return o_att, o_err, b2g, o_inp, aims


@pytest.mark.parametrize("n", [1, 65])   # one lane; one lane into a second workgroup of k_attitude (k_aim: a workgroup per stream)
def test_every_byte_of_every_stream_with_tables(n):
    c = Context(device=0, max_frames=n, max_width=64, max_height=64)
    c.pnp_load()
    c.upload(np.zeros((n, 1, 1, 3), np.uint8))                             # the smallest geometry there is: the steps read no pixel
    L = AIMK.lists()
    names = [k for k in L]
    lists = [L[names[(f + 1) % len(names)]] for f in range(n)]            # (stream 0: one track, not the empty list)
    trk = Tracker(device=0, n_streams=n, track_cap=64, frame_w=1, frame_h=1)
    for f, tr in enumerate(lists):
        trk.put(f, tr)
    one_att = default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH, gripper2camera=CK.hand_eye(299))
    one_aim = CK.aim_config(399)
    mats = np.array([CK.hand_eye(300 + f) for f in range(n)])
    att_cfgs = [default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH, gripper2camera=m) for m in mats]
    aim_cfgs = [CK.aim_config(400 + f) for f in range(n)]
    with pytest.raises(RmcvError) as e:
        trk.set_aim_configs(aim_cfgs)                                       # aiming is off
    assert e.value.code == abi.ERR_BAD_ARG and "off" in str(e.value)
    trk.set_attitude(one_att)
    trk.set_aim(one_aim)
    # what is refused names the stream and changes nothing
    bad_m = mats.copy()
    bad_m[n - 1, 2, 3] = np.inf
    bad_a = list(aim_cfgs)
    bad_a[n - 1] = default_aim_config(mode=abi.COMPENSATE_NI)
    for call, arg in ((trk.set_stream_cameras, bad_m), (trk.set_aim_configs, bad_a)):
        with pytest.raises(RmcvError) as e:
            call(arg)
        assert e.value.code == abi.ERR_BAD_ARG and "stream %d" % (n - 1) in str(e.value), str(e.value)
    att, _, inp = ATTK.start_tables(n, 44)
    err = np.zeros(n, np.int32)
    trk.set_attitudes(att)
    trk.set_aim_inputs(inp)
    pk = ATTK.packets(n, 41)[0]
    d_pk = device_array(pk)

    def step_and_compare(packets, att_c, aim_c, att, err, inp, what):
        c.attitude(trk, None if packets is None else d_pk.data_ptr())
        trk.aim(AIMK.NOW)
        w_att, w_err, w_b2g, w_inp, w_aims = host_statements(att_c, aim_c, packets, att, err, inp, lists)
        g_att, g_err = trk.attitudes()
        assert g_att.tobytes() == w_att.tobytes() and g_err.tolist() == w_err.tolist(), what
        assert c.base2gripper().tobytes() == w_b2g.tobytes(), what
        assert trk.aim_inputs().tobytes() == w_inp.tobytes(), what
        assert trk.aims().tobytes() == w_aims.tobytes(), what
        return w_att, w_err, w_inp, w_aims

    # the refused tables left the single configs in force
    att, err, inp, aims_one = step_and_compare(pk, [one_att] * n, [one_aim] * n, att, err, inp, "single")
    trk.set_stream_cameras(mats)
    trk.set_aim_configs(aim_cfgs)
    att, err, inp, aims_tab = step_and_compare(pk, att_cfgs, aim_cfgs, att, err, inp, "tables, packets")
    att, err, inp, _ = step_and_compare(None, att_cfgs, aim_cfgs, att, err, inp, "tables, no packets")
    assert aims_tab.tobytes() != aims_one.tobytes()
    # PnpConfigs are taken for their gripper2camera
    trk.set_stream_cameras([CK.moved_camera(300 + f) for f in range(n)])
    att, err, inp, _ = step_and_compare(None, att_cfgs, aim_cfgs, att, err, inp, "tables from PnpConfigs")
    # one table off at a time, then both: back to what the single config gives
    trk.set_stream_cameras(None)
    att, err, inp, _ = step_and_compare(None, [one_att] * n, aim_cfgs, att, err, inp, "matrices off")
    trk.set_aim_configs(None)
    att, err, inp, _ = step_and_compare(pk, [one_att] * n, [one_aim] * n, att, err, inp, "both off")
    assert c.check_guards()[0] == 0
    trk.close()
    c.close()


# ---------------------------------------------------------------- 6. the closed loop
N, STEPS = 4, 4
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
CAM_IDX = [1, 2, 3, 0]


def closed_loop(frames, origins, cams, idx, att_cfg, stream_cams, aim_cfg, aim_cfgs):
    """packets in, identity + pose, context path; per step, per stream: (tracks, side records, origin, aim input, aim)"""
    trk = Tracker(device=0, n_streams=N, frame_w=FW, frame_h=FH, win_w=WW, win_h=WH)
    trk.set_origins(origins)
    trk.set_camps(np.full(N, CAMP_BLUE, np.int32))
    trk.set_aim(aim_cfg)
    trk.set_attitude(att_cfg)
    if stream_cams is not None:
        trk.set_stream_cameras(stream_cams)
        trk.set_aim_configs(aim_cfgs)
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.svm_load(*synth.svm_weights())
    if idx is not None:
        c.pnp_load_cameras(cams)
    else:
        c.pnp_load(cams[0])                                                 # the single-config call
    dev = [device_array(p) for p in loop_packets()]
    out = []
    for k in range(STEPS):
        c.upload(frames[k])
        c.set_windows(trk.device_origins(), WW, WH)
        c.set_frame_camps(trk.device_camps()[0])
        if idx is not None:
            c.set_frame_cameras(idx)
        c.attitude(trk, dev[k].data_ptr())
        c.run(default_params(), FULL)
        c.track(trk, (k + 1) * 8 * MS)
        c.sync()
        inp, aims = trk.aim_inputs(), trk.aims()
        out.append([trk.get(f) + (inp[f].tobytes(), aims[f].tobytes()) for f in range(N)])
    assert c.check_guards()[0] == 0
    c.close()
    trk.close()
    return out


def same_stream(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3] and a[4] == b[4]


def test_closed_loop_equals_one_loop_per_robot(oracle):
    frames = moving_scene(0, N, STEPS)
    origins = []
    for f in frames[0]:
        a = oracle.detect_frame(f, oracle.default_params())["armours"]
        assert len(a)
        origins.append(W.window_origin(W.get_roi(a[0]["vertices"], (1.0, 1.0), (FW, FH)), WW, WH))
    origins = np.array(origins, np.int32)
    cams = CK.fleet(4)
    mine = [cams[CAM_IDX[f]] for f in range(N)]                             # stream f's camera
    aim_cfgs = [CK.aim_config(500 + f) for f in range(N)]

    def att(cam):
        return default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH, gripper2camera=np.array(cam.gripper2camera))

    table = closed_loop(frames, origins, cams, CAM_IDX, att(cams[0]), mine, aim_cfgs[0], aim_cfgs)
    assert all(len(s[0]) for s in table[-1])                                # every stream tracks something at the end
    others = 0
    for f in range(N):                                                      # the SAME loop with stream f's camera, matrix and aim config as THE config
        single = closed_loop(frames, origins, [mine[f]], None, att(mine[f]), None, aim_cfgs[f], None)
        for k in range(STEPS):
            assert same_stream(table[k][f], single[k][f]), (f, k)
            others += sum(not same_stream(table[k][g], single[k][g]) for g in range(N) if g != f)
    assert others > 0                                                       # ... and the other streams' results are not that robot's
