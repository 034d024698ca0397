"""The calibration solve on the GPU (k_calib.hip): results and view records equal rmcv_calibrate_camera_host byte for byte, rvec
included -- the stage-wise call and the device-table call on every case of tests/calib_cases.py; the fleet case in one launch against its
cameras solved one by one, with the rows of skipped views and of the camera left with two views untouched; every refusal leaves its tables
unchanged; the chain find -> refine -> solve on four drawn frames against the three host functions, and its result through as_pnp_config()
into pnp_load_cameras.  Seconds in all."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as CC
import rmcv_amd as R
from rmcv_amd import Context, RmcvError, abi, synth
from rmcv_amd.abi import lib

pytestmark = pytest.mark.gpu

SIZE = (CC.W, CC.H)
NAMES = [c.name for c in CC.CASES]


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, max_frames=4, max_width=320, max_height=256)
    yield c
    c.close()


def host(case):
    res, views = R.calibrate_camera_host(case.corners, case.counts, case.cols, case.rows, case.square, SIZE, case.params, case.guess)
    return res.rec.tobytes(), views.tobytes(), res


@pytest.mark.parametrize("name", NAMES)
def test_stagewise_equals_host(ctx, name):
    case = CC.BY_NAME[name]
    res, views = ctx.calibrate_camera(case.corners, case.counts, case.cols, case.rows, case.square, SIZE, case.params, case.guess)
    want_res, want_views, h = host(case)
    assert (res.status, res.iters, res.views_used) == (h.status, h.iters, h.views_used)
    assert res.rec.tobytes() == want_res and views.tobytes() == want_views


@pytest.mark.parametrize("name", NAMES)
def test_device_tables_equal_host(ctx, name):
    case = CC.BY_NAME[name]
    res, views = ctx.calibrate_cameras(case.corners, case.counts, case.cols, case.rows, case.square, SIZE, params=case.params,
                                       guesses=None if case.guess is None else [case.guess])
    want_res, want_views, h = host(case)
    assert len(res) == 1 and (res[0].status, res[0].iters) == (h.status, h.iters)
    assert res[0].rec.tobytes() == want_res and views.tobytes() == want_views


def sentinels(n_cameras, n_views):
    res, views = np.zeros(n_cameras, abi.CALIB_RESULT), np.zeros(n_views, abi.CALIB_VIEW)
    res.view(np.uint8)[:] = 0xC3
    views.view(np.uint8)[:] = 0x3C
    return res, views


def test_fleet_in_one_launch_equals_its_cameras_alone(ctx):
    fl = CC.FLEET
    res0, views0 = sentinels(fl.n_cameras, len(fl.corners))
    res, views = ctx.calibrate_cameras(fl.corners, fl.counts, fl.cols, fl.rows, fl.square, SIZE, view_camera=fl.view_camera, n_cameras=fl.n_cameras,
                                       results=res0, views=views0)
    want_res, want_views = res0.copy(), views0.copy()
    for cam in range(fl.n_cameras):
        cor, cnt, idx = CC.alone(fl, cam)
        h, hv = R.calibrate_camera_host(cor, cnt, fl.cols, fl.rows, fl.square, SIZE)
        if cam == 2:        # left with two used views: the status, the count and iters = 0; nothing else
            assert h.status == R.CALIB_TOO_FEW_VIEWS and h.views_used == 2 and not hv["used"].any()
            want_res["status"][cam], want_res["views_used"][cam], want_res["iters"][cam] = R.CALIB_TOO_FEW_VIEWS, 2, 0
            continue
        assert h.solved
        want_res[cam] = h.rec
        used = hv["used"] == 1
        want_views[idx[used]] = hv[used]
    assert [r.status for r in res] == [int(s) for s in want_res["status"]]
    assert np.array([r.rec for r in res], abi.CALIB_RESULT).tobytes() == want_res.tobytes()
    assert views.tobytes() == want_views.tobytes()
    skipped = np.nonzero((fl.cameras == 2) | (fl.counts == 0))[0]
    assert len(skipped) == 4 and views[skipped].tobytes() == views0[skipped].tobytes()


def test_skipped_views_leave_their_rows_untouched(ctx):
    case = CC.BY_NAME["s9_skips"]
    res0, views0 = sentinels(1, len(case.corners))
    res, views = ctx.calibrate_cameras(case.corners, case.counts, case.cols, case.rows, case.square, SIZE, results=res0, views=views0)
    _, hv = R.calibrate_camera_host(case.corners, case.counts, case.cols, case.rows, case.square, SIZE)
    used = hv["used"] == 1
    assert used.tolist() == [True, False, True, True, False, True, False, False, True] and res[0].views_used == 5
    assert views[used].tobytes() == hv[used].tobytes() and views[~used].tobytes() == views0[~used].tobytes()


def test_every_refusal_leaves_the_tables_unchanged(ctx):
    case = CC.BY_NAME["s3_3x3"]
    cor, cnt = abi.calib_tables(case.corners, case.counts)
    res0, views0 = sentinels(1, 3)
    tabs = [cor, cnt, res0, views0]
    dev, offs = ctx._dev_tables(tabs)
    try:
        for o, a in zip(offs, tabs):
            ctx._dev_copy(dev, o, a, True)
        at = lambda k: (dev.value or 0) + offs[k]
        good = dict(corners=at(0), counts=at(1), cols=3, rows=3, square=80.0, size=SIZE, results=at(2), views=at(3), per_frame=9, n_views=3, n_cameras=1)
        nan_guess = (np.array([np.nan, 0, 1, 0, 1, 1, 0, 0, 1.0]), np.zeros(5))
        bad = [dict(corners=0), dict(counts=0), dict(views=0), dict(n_views=0), dict(n_views=4097), dict(n_cameras=0), dict(n_cameras=65), dict(cols=1, rows=3),
               dict(cols=0, rows=9), dict(cols=33, rows=32, per_frame=1024), dict(per_frame=8), dict(per_frame=1025), dict(square=0.0), dict(square=float("inf")),
               dict(size=(0, 1024)), dict(size=(1280, 0)), dict(max_iters=0), dict(max_iters=101), dict(fix_mask=-1), dict(fix_mask=512), dict(eps=-1.0),
               dict(eps=float("nan")), dict(guesses=[nan_guess]), dict(guesses=[(np.array([100.0, 0, 1, 0, -5.0, 1, 0, 0, 1.0]), np.zeros(5))])]
        for change in bad:
            with pytest.raises(RmcvError) as e:
                ctx.calibrate_cameras(**dict(good, **change))
            assert e.value.code == abi.ERR_BAD_ARG and "calibration: " in str(e.value), change
        ctx.sync()
        got_res, got_views = np.zeros_like(res0), np.zeros_like(views0)
        ctx._dev_copy(dev, offs[2], got_res, False)
        ctx._dev_copy(dev, offs[3], got_views, False)
        assert got_res.tobytes() == res0.tobytes() and got_views.tobytes() == views0.tobytes()
        ctx.calibrate_cameras(**good)                   # ... and the same tables through the call that is not refused
        ctx.sync()
        ctx._dev_copy(dev, offs[2], got_res, False)
        assert got_res.tobytes() == host(case)[0]
    finally:
        lib().rmcv_device_free(ctx.device, dev)
    with pytest.raises(RmcvError):
        ctx.calibrate_camera(case.corners, case.counts, 3, 3, 80.0, SIZE, max_iters=0)


# the chain: four frames of 320 x 256 with a 4 x 3 board of 30-unit squares drawn from a pinhole camera
W, H, SQUARE = 320, 256, 30.0
DRAW_K = np.array([[420.0, 0, 158.3], [0, 418.0, 130.6], [0, 0, 1]])
DRAW_POSES = [(0.35, -0.25, 0.1, (-60, -50, 520)), (-0.4, 0.3, -0.15, (-75, -40, 560)), (0.25, 0.45, 0.2, (-50, -60, 500)), (-0.3, -0.45, 0.05, (-70, -35, 540))]


def drawn_frame(pose):
    Rm, t = CC.rotation(*pose[:3]), np.array(pose[3], np.float64)
    Hd = DRAW_K @ np.stack([Rm[:, 0] * SQUARE, Rm[:, 1] * SQUARE, t - SQUARE * (Rm[:, 0] + Rm[:, 1])], 1)    # unit squares, inner corner (1, 1) = object point 0
    return synth.chessboard(W, H, Hd, 5, 4)[0]


def test_chain_find_refine_solve_equals_the_host_functions(ctx):
    frames = np.stack([drawn_frame(p) for p in DRAW_POSES])
    ctx.upload(frames)
    res, views, cor, cnt, st, cst = ctx.calibrate([0, 1, 2, 3], 4, 3, SQUARE)
    want_cor, want_cnt = np.full((4, 12, 2), np.nan, np.float32), np.zeros(4, np.int32)
    for f in range(4):
        c, _, _ = R.find_chessboard_host(frames[f], 4, 3)
        assert c is not None
        want_cor[f], want_cnt[f] = R.corner_subpix_host(frames[f], c, (8, 8))[0], 12
    h, hv = R.calibrate_camera_host(want_cor, want_cnt, 4, 3, SQUARE, (W, H))
    assert cnt.tolist() == [12] * 4 and cor.tobytes() == want_cor.tobytes()
    assert res.rec.tobytes() == h.rec.tobytes() and views.tobytes() == hv.tobytes() and res.solved and res.views_used == 4
    # recorded, not bounded: it rests on the detector's and the refinement's errors on a board this small
    print("chain: rms %.4f px, fx %+.2f fy %+.2f cx %+.2f cy %+.2f against the drawing camera" % (
        res.rms, res.camera_matrix[0, 0] - DRAW_K[0, 0], res.camera_matrix[1, 1] - DRAW_K[1, 1], res.camera_matrix[0, 2] - DRAW_K[0, 2],
        res.camera_matrix[1, 2] - DRAW_K[1, 2]))
    cfg = res.as_pnp_config()
    base = R.abi.default_pnp_config()
    assert list(cfg.camera_matrix) == res.camera_matrix.reshape(-1).tolist() and list(cfg.dist) == res.dist.tolist()
    assert list(cfg.gripper2camera) == list(base.gripper2camera) and (cfg.square_w, cfg.square_h) == (base.square_w, base.square_h)
    ctx.pnp_load_cameras([cfg, base])
