"""The hand-eye solve on the GPU (k_handeye.hip): results and view rows equal rmcv_calibrate_hand_eye_host byte for byte -- the
stage-wise call and the device-table call on every case of tests/handeye_cases.py, the degenerate, too-few and too-many ones included; the fleet
in one launch against its cameras solved one by one, with the rows of skipped views and of the camera left with two views untouched; every
refusal leaves its tables unchanged; attitudes read from a Tracker's device table give the bytes the host array gives; the chain find -> refine
-> solve -> hand-eye on five drawn frames against the four host functions, and its result through as_pnp_config() into pnp_load_cameras and
Tracker.set_stream_cameras.  Seconds in all."""
import numpy as np
import pytest

import calib_cases as CC
import handeye_cases as HC
import rmcv_amd as R
from rmcv_amd import Context, RmcvError, Tracker, abi, synth
from rmcv_amd.abi import lib

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in HC.CASES]
_host = {}


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, max_frames=5, max_width=320, max_height=256)
    yield c
    c.close()


def host(case):
    """(result bytes, row bytes, HandEyeResult) of the host form, computed once per case"""
    if case.name not in _host:
        res, rows = R.calibrate_hand_eye_host(case.views, case.attitudes, case.gripper_t, case.params)
        _host[case.name] = (np.array(res.rec).tobytes(), rows.tobytes(), res)
    return _host[case.name]


@pytest.mark.parametrize("name", NAMES)
def test_stagewise_equals_host(ctx, name):
    case = HC.BY_NAME[name]
    res, rows = ctx.calibrate_hand_eye(case.views, case.attitudes, case.gripper_t, case.params)
    want_res, want_rows, h = host(case)
    assert (res.status, res.views_used, res.pairs_used, res.pairs_skipped, res.sweeps) == (h.status, h.views_used, h.pairs_used, h.pairs_skipped, h.sweeps)
    assert np.array(res.rec).tobytes() == want_res and rows.tobytes() == want_rows


@pytest.mark.parametrize("name", NAMES)
def test_device_tables_equal_host(ctx, name):
    case = HC.BY_NAME[name]
    res, rows = ctx.calibrate_hand_eyes(case.views, case.attitudes, case.gripper_t, params=case.params)
    want_res, want_rows, h = host(case)
    assert len(res) == 1 and (res[0].status, res[0].pairs_used) == (h.status, h.pairs_used)
    assert np.array(res[0].rec).tobytes() == want_res and rows.tobytes() == want_rows


def sentinels(n_cameras, n_views):
    res, rows = np.zeros(n_cameras, abi.HANDEYE_RESULT), np.zeros(n_views, abi.HANDEYE_VIEW)
    res.view(np.uint8)[:] = 0xC3
    rows.view(np.uint8)[:] = 0x3C
    return res, rows


def counts_only(rec, h):
    """a camera without a solution: the status and the four counts; nothing else"""
    for k in ("status", "views_used", "pairs_used", "pairs_skipped", "sweeps"):
        rec[k] = getattr(h, k)


def test_fleet_in_one_launch_equals_its_cameras_alone(ctx):
    fl = HC.FLEET
    res0, rows0 = sentinels(fl.n_cameras, len(fl.views))
    res, rows = ctx.calibrate_hand_eyes(fl.views, fl.attitudes, view_camera=fl.view_camera, n_cameras=fl.n_cameras, results=res0, rows=rows0)
    want_res, want_rows = res0.copy(), rows0.copy()
    for cam in range(fl.n_cameras):
        vw, att, idx = HC.alone(fl, cam)
        h, hr = R.calibrate_hand_eye_host(vw, att)
        if cam == 2:        # left with two used views
            assert h.status == R.HANDEYE_TOO_FEW_VIEWS and h.views_used == 2 and not hr["used"].any()
            counts_only(want_res[cam:cam + 1], h)
            continue
        assert h.status == R.HANDEYE_OK
        want_res[cam] = h.rec
        used = hr["used"] == 1
        want_rows[idx[used]] = hr[used]
    assert [r.status for r in res] == [int(s) for s in want_res["status"]]
    assert np.array([r.rec for r in res], abi.HANDEYE_RESULT).tobytes() == want_res.tobytes()
    assert rows.tobytes() == want_rows.tobytes()
    skipped = np.nonzero((fl.cameras == 2) | (fl.views["used"] == 0))[0]
    assert len(skipped) == 4 and rows[skipped].tobytes() == rows0[skipped].tobytes()


def test_skipped_views_and_unsolved_cameras_leave_their_rows_untouched(ctx):
    for name in ("v9_skips", "v257_too_many", "v3_all_skipped"):
        case = HC.BY_NAME[name]
        res0, rows0 = sentinels(1, len(case.views))
        res, rows = ctx.calibrate_hand_eyes(case.views, case.attitudes, case.gripper_t, params=case.params, results=res0, rows=rows0)
        _, hr, h = host(case)
        used = np.frombuffer(hr, abi.HANDEYE_VIEW)["used"] == 1
        assert rows[used].tobytes() == np.frombuffer(hr, abi.HANDEYE_VIEW)[used].tobytes() and rows[~used].tobytes() == rows0[~used].tobytes()
        if not h.solved:
            want = res0.copy()
            counts_only(want, h)
            assert not used.any() and np.array(res[0].rec).tobytes() == want.tobytes()
    assert host(HC.BY_NAME["v9_skips"])[2].views_used == 5


def test_every_refusal_leaves_the_tables_unchanged(ctx):
    case = HC.BY_NAME["v3"]
    vw, att, _ = abi.handeye_tables(case.views, case.attitudes)
    res0, rows0 = sentinels(1, 3)
    tabs = [vw, att, res0, rows0]
    dev, offs = ctx._dev_tables(tabs)
    try:
        for o, a in zip(offs, tabs):
            ctx._dev_copy(dev, o, a, True)
        at = lambda k: (dev.value or 0) + offs[k]
        good = dict(views=at(0), attitudes=at(1), results=at(2), rows=at(3), n_views=3, n_cameras=1)
        bad = [dict(views=0), dict(attitudes=0), dict(rows=0), dict(n_views=0), dict(n_views=4097), dict(n_cameras=0), dict(n_cameras=65), dict(min_w=-0.1), dict(min_w=1.0),
               dict(min_w=float("nan")), dict(min_w=float("inf"))]
        for change in bad:
            with pytest.raises(RmcvError) as e:
                ctx.calibrate_hand_eyes(**dict(good, **change))
            assert e.value.code == abi.ERR_BAD_ARG and "hand-eye: " in str(e.value), change
        ctx.sync()
        got_res, got_rows = np.zeros_like(res0), np.zeros_like(rows0)
        ctx._dev_copy(dev, offs[2], got_res, False)
        ctx._dev_copy(dev, offs[3], got_rows, False)
        assert got_res.tobytes() == res0.tobytes() and got_rows.tobytes() == rows0.tobytes()
        ctx.calibrate_hand_eyes(**good)                 # ... and the same tables through the call that is not refused
        ctx.sync()
        ctx._dev_copy(dev, offs[2], got_res, False)
        ctx._dev_copy(dev, offs[3], got_rows, False)
        assert got_res.tobytes() == host(case)[0] and got_rows.tobytes() == host(case)[1]
    finally:
        lib().rmcv_device_free(ctx.device, dev)
    with pytest.raises(RmcvError) as e:
        ctx.calibrate_hand_eye(case.views, case.attitudes, min_w=1.0)
    assert e.value.code == abi.ERR_BAD_ARG and "rmcv_calibrate_hand_eye: hand-eye: " in str(e.value)


def test_attitudes_from_a_trackers_device_table(ctx):
    case = HC.BY_NAME["v12_noise"]
    n = len(case.views)
    trk = Tracker(device=0, n_streams=n, track_cap=1, frame_w=1, frame_h=1)
    try:
        trk.set_attitude()
        trk.set_attitudes(case.attitudes)
        assert trk.attitudes()[0].tobytes() == case.attitudes.tobytes()            # (synchronous: the table is on the device)
        res0, rows0 = abi.handeye_outputs(1, n)
        tabs = [np.ascontiguousarray(case.views), res0, rows0]
        dev, offs = ctx._dev_tables(tabs)
        try:
            for o, a in zip(offs, tabs):
                ctx._dev_copy(dev, o, a, True)
            at = lambda k: (dev.value or 0) + offs[k]
            ctx.calibrate_hand_eyes(at(0), trk.device_attitudes(), results=at(1), rows=at(2), n_views=n)
            ctx.sync()
            ctx._dev_copy(dev, offs[1], res0, False)
            ctx._dev_copy(dev, offs[2], rows0, False)
        finally:
            lib().rmcv_device_free(ctx.device, dev)
        assert res0.tobytes() == host(case)[0] and rows0.tobytes() == host(case)[1]
    finally:
        trk.close()


# the chain: five frames of 320 x 256 with a 4 x 3 board of 30-unit squares drawn from a pinhole camera that hangs on a gimbal by MOUNT;
# the board stands still in the base frame (BOARD: its pose in the camera at zero attitude), the gimbal takes the attitudes ATT
W, H, SQUARE = 320, 256, 30.0
DRAW_K = np.array([[420.0, 0, 158.3], [0, 418.0, 130.6], [0, 0, 1]])
MOUNT_R, MOUNT_T = HC.TRUE_R, HC.TRUE_T
BOARD = (0.35, -0.3, 0.1, (-60, -50, 540))
ATT = np.array([(0.0, 0.0, 0.0), (0.45, 0.07, -0.05), (-0.5, -0.06, 0.08), (0.3, -0.08, -0.07), (-0.35, 0.09, 0.04)])       # (roll, pitch, yaw)


def chain_poses():
    """board-to-camera (R, t) per frame: C_v = X^-1 B_v^-1 (X C_0)"""
    R0, t0 = CC.rotation(*BOARD[:3]), np.array(BOARD[3], np.float64)
    R_w, t_w = MOUNT_R @ R0, MOUNT_R @ t0 + MOUNT_T
    out = []
    for roll, pitch, yaw in ATT:
        B = CC.rotation(roll, pitch, yaw)
        out.append((MOUNT_R.T @ B.T @ R_w, MOUNT_R.T @ (B.T @ t_w - MOUNT_T)))
    return out


def drawn_frame(Rm, t):
    Hd = DRAW_K @ np.stack([Rm[:, 0] * SQUARE, Rm[:, 1] * SQUARE, t - SQUARE * (Rm[:, 0] + Rm[:, 1])], 1)    # unit squares, inner corner (1, 1) = object point 0
    return synth.chessboard(W, H, Hd, 5, 4)[0]


def host_chain(frames):
    n = len(frames)
    cor, cnt = np.full((n, 12, 2), np.nan, np.float32), np.zeros(n, np.int32)
    for f in range(n):
        c, _, _ = R.find_chessboard_host(frames[f], 4, 3)
        assert c is not None, f
        cor[f], cnt[f] = R.corner_subpix_host(frames[f], c, (8, 8))[0], 12
    h, hv = R.calibrate_camera_host(cor, cnt, 4, 3, SQUARE, (W, H))
    return cor, cnt, h, hv, R.calibrate_hand_eye_host(hv, ATT)


def test_chain_find_refine_solve_hand_eye_equals_the_host_functions(ctx):
    frames = np.stack([drawn_frame(Rm, t) for Rm, t in chain_poses()])
    ctx.upload(frames)
    fr = list(range(len(frames)))
    res, views, cor, cnt, st, cst, he, rows = ctx.calibrate(fr, 4, 3, SQUARE, attitudes=ATT)
    want_cor, want_cnt, h, hv, (hhe, hrows) = host_chain(frames)
    assert cnt.tolist() == [12] * len(frames) and cor.tobytes() == want_cor.tobytes()
    assert res.rec.tobytes() == h.rec.tobytes() and views.tobytes() == hv.tobytes() and res.solved and res.views_used == len(frames)
    assert np.array(he.rec).tobytes() == np.array(hhe.rec).tobytes() and rows.tobytes() == hrows.tobytes() and he.solved and he.views_used == len(frames)
    # without attitudes the call returns what it always returned
    plain = ctx.calibrate(fr, 4, 3, SQUARE)
    assert len(plain) == 6 and plain[0].rec.tobytes() == res.rec.tobytes() and plain[1].tobytes() == views.tobytes()
    # recorded, not bounded: twelve corners a view leave the poses loose
    dq = he.q - HC.TRUE_Q if he.q @ HC.TRUE_Q > 0 else he.q + HC.TRUE_Q
    print("chain: status %d, against the drawn mounting %.3f deg, %.2f units; rot_rms %.3g, trans_rms %.3g, world_rms %.3g, eig %s, pivots %s" % (
        he.status, np.degrees(2 * np.arcsin(min(1.0, np.linalg.norm(dq) / 2))), np.linalg.norm(he.t - MOUNT_T), he.rot_rms, he.trans_rms, he.world_rms, he.eig, he.pivots))
    cfg = he.as_pnp_config(res.as_pnp_config(), allow_rotation_only=True)
    assert list(cfg.gripper2camera) == he.cam2gripper.reshape(-1).tolist() and list(cfg.camera_matrix) == res.camera_matrix.reshape(-1).tolist()
    ctx.pnp_load_cameras([cfg, R.abi.default_pnp_config()])
    trk = Tracker(device=0, n_streams=2, track_cap=1, frame_w=1, frame_h=1)
    try:
        trk.set_attitude(he.as_attitude_config(allow_rotation_only=True))
        trk.set_stream_cameras([cfg, R.abi.default_pnp_config()])
    finally:
        trk.close()
