"""The calibration solve on the CPU: rmcv_calibrate_camera_host against tests/calib_ref.py, the numpy restatement of the text at
the head of rmcv_amd/csrc/device_calib.h -- bit for bit on intrinsics, distortion, q, t, rms, iterations and status for every case of
tests/calib_cases.py, rvec within RVEC_ULPS of the restatement with math.atan2 in place of pm_atan2; every refusal; skipped views; the fix
mask; the fleet's cameras; rmcv_calib_to_pnp_config; and a second opinion from scipy.optimize.least_squares on the textbook model.  No GPU."""
import math

import numpy as np
import pytest

import calib_cases as CC
import calib_ref as REF
import rmcv_amd as R
from rmcv_amd import RmcvError, abi

SIZE = (CC.W, CC.H)
NAMES = [c.name for c in CC.CASES]
# rvec: the one pinned-versus-libm call.  Measured over the cases: at most 2 ulps; allowed: twice that
RVEC_ULPS = 4
# the second opinion, measured here on the CPU over CC.FREE; each bound is 8 x the largest measured value (all on s12_noise, which
# ends at max_iters; the clean sessions: 2.1e-13 px, 7.4e-7 px, 1.1e-7):
#   |the library's rms - scipy's|: at most 1.3e-11 px (the library's is the lower one in every session);
#   |fx fy cx cy| against scipy's: at most 5.3e-5 px; |k1 k2 p1 p2 k3|: at most 9.3e-5
RMS_MARGIN, PIXELS_TOL, DIST_TOL = 8 * 1.3e-11, 8 * 5.3e-5, 8 * 9.3e-5

bits = lambda x: np.asarray(x, np.float64).tobytes()
_memo = {}


def solved(name):
    """(the library's (CalibResult, views), the restatement's (Result, {view: View})) of a case, computed once"""
    if name not in _memo:
        c = CC.BY_NAME[name]
        lib = R.calibrate_camera_host(c.corners, c.counts, c.cols, c.rows, c.square, SIZE, c.params, c.guess)
        ref = REF.calibrate(c.corners, c.counts, c.cols, c.rows, c.square, CC.W, CC.H, guess=c.guess, **dict(REF.DEFAULTS, **c.params))
        _memo[name] = (lib, ref)
    return _memo[name]


def ulps(a, b):
    a, b = np.frombuffer(bits(a), np.int64), np.frombuffer(bits(b), np.int64)
    key = lambda v: np.where(v < 0, np.int64(-2 ** 63) - v, v)     # (sign-magnitude to a line)
    return int(np.max(np.abs(key(a) - key(b))))


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_restatement_bit_for_bit(name):
    (res, views), (ref, rviews) = solved(name)
    assert isinstance(ref, REF.Result)
    assert (res.status, res.iters, res.views_used) == (ref.status, ref.iters, ref.views_used)
    assert res.iters <= dict(REF.DEFAULTS, **CC.BY_NAME[name].params)["max_iters"] and res.status in (R.CALIB_CONVERGED, R.CALIB_MAX_ITERS)
    assert bits(res.camera_matrix) == bits(ref.camera_matrix) and bits(res.dist) == bits(ref.dist)
    assert bits(res.rms) == bits(ref.rms) and bits(res.rms_init) == bits(ref.rms_init)
    assert np.nonzero(views["used"])[0].tolist() == sorted(rviews)
    worst = 0
    for v, rv in rviews.items():
        assert bits(views[v]["q"]) == bits(rv.q) and bits(views[v]["tvec"]) == bits(rv.tvec) and bits(views[v]["rms"]) == bits(rv.rms), v
        worst = max(worst, ulps(views[v]["rvec"], rv.rvec))
    print("%s: rvec within %d ulps of the restatement with math.atan2" % (name, worst))
    assert worst <= RVEC_ULPS


@pytest.mark.parametrize("name", CC.FREE)
def test_free_sessions_reach_the_truth(name):
    """(indicative: the clean float32 sessions end near 2e-5 px rms; the truth lies within the figures DESIGN.md 4u records)"""
    (res, views), _ = solved(name)
    a = np.array([res.camera_matrix[0, 0], res.camera_matrix[1, 1], res.camera_matrix[0, 2], res.camera_matrix[1, 2]])
    print("%s: rms %.3g (init %.3g), iters %d, |fx fy cx cy - truth| <= %.2g px" % (name, res.rms, res.rms_init, res.iters, np.abs(a - CC.TRUE_A[:4]).max()))
    assert res.rms < res.rms_init and res.rms < (0.2 if name == "s12_noise" else 1e-4)


def test_skipped_views_and_untouched_rows():
    c = CC.BY_NAME["s9_skips"]
    (res, views), _ = solved("s9_skips")
    assert views["used"].tolist() == [1, 0, 1, 1, 0, 1, 0, 0, 1] and res.views_used == 5
    assert views[views["used"] == 0].tobytes() == bytes(4 * abi.CALIB_VIEW.itemsize)        # rows of skipped views: as the wrapper zeroed them
    keep = views["used"] == 1                                                                 # ... and the same session without them: the same bits
    alone, aviews = R.calibrate_camera_host(c.corners[keep], c.counts[keep], c.cols, c.rows, c.square, SIZE)
    assert alone.rec.tobytes() == res.rec.tobytes() and aviews.tobytes() == views[keep].tobytes()


def test_too_few_and_too_many_views_write_the_status_alone():
    c = CC.BY_NAME["s3_3x3"]
    res, views = R.calibrate_camera_host(c.corners[:2], c.counts[:2], 3, 3, c.square, SIZE)
    assert (res.status, res.views_used, res.iters, res.rms) == (R.CALIB_TOO_FEW_VIEWS, 2, 0, 0.0) and not views["used"].any() and not res.solved
    assert not res.camera_matrix.any()
    many = np.tile(c.corners, (86, 1, 1))[:257]
    res, views = R.calibrate_camera_host(many, None, 3, 3, c.square, SIZE)
    assert (res.status, res.views_used, res.iters) == (R.CALIB_TOO_MANY_VIEWS, 257, 0) and not views["used"].any()
    ref, _ = REF.calibrate(many, np.full(257, 9), 3, 3, c.square, CC.W, CC.H)
    assert ref == (REF.TOO_MANY_VIEWS, 257)
    with pytest.raises(RmcvError):
        res.as_pnp_config()


def test_bad_init_from_views_that_are_all_the_same():
    """three copies of one view: the vanishing-point equations are singular or the cost is not finite -- whatever the restatement says, bit for bit"""
    c = CC.BY_NAME["s3_3x3"]
    same = np.repeat(c.corners[:1], 3, axis=0)
    res, views = R.calibrate_camera_host(same, None, 3, 3, c.square, SIZE)
    ref, _ = REF.calibrate(same, np.full(3, 9), 3, 3, c.square, CC.W, CC.H)
    if isinstance(ref, REF.Result):
        assert (res.status, res.iters) == (ref.status, ref.iters) and bits(res.camera_matrix) == bits(ref.camera_matrix)
    else:
        assert (res.status, res.views_used) == ref and res.iters == 0 and not views["used"].any()


def test_fix_mask_leaves_fixed_parameters_bit_equal_to_their_start():
    (res, _), _ = solved("s5_11x8_fix")
    assert bits(res.dist[[2, 3, 4]]) == bits([0.0, 0.0, 0.0]) and res.dist[0] != 0.0 and res.dist[1] != 0.0
    (res, _), _ = solved("s19_4x3_guess_fix")
    K, d = CC.GUESS
    assert bits(res.dist[[1, 2, 3, 4]]) == bits(d[[1, 2, 3, 4]]) and res.dist[0] != d[0] and res.camera_matrix[0, 0] != K[0]
    c = CC.BY_NAME["s19_4x3_guess"]
    res, _ = R.calibrate_camera_host(c.corners, c.counts, c.cols, c.rows, c.square, SIZE, guess=c.guess, fix_mask=511, max_iters=5)   # everything held
    assert bits(res.camera_matrix) == bits(K) and bits(res.dist) == bits(d) and res.solved
    assert abi.calib_params(fix_mask=("k3", "p1", "p2"))["fix_mask"][0] == CC.FIX_MASK


def test_fleet_cameras_alone():
    fl = CC.FLEET
    assert sorted(set(fl.cameras.tolist())) == [0, 1, 2]
    for cam, want_used in ((0, 6), (1, 5), (2, 2)):
        cor, cnt, idx = CC.alone(fl, cam)
        res, views = R.calibrate_camera_host(cor, cnt, fl.cols, fl.rows, fl.square, SIZE)
        assert res.views_used == want_used and res.solved == (cam != 2)
        labels = fl.view_camera[idx]
        assert all((l if 0 <= l < fl.n_cameras else 0) == cam for l in labels)     # (frame_camera_eff's rule: a value outside the table is camera 0)


def test_to_pnp_config():
    (res, _), _ = solved("s5_11x8")
    base = abi.default_pnp_config()
    base.square_w, base.gripper2camera[3] = 31.0, -1.5
    cfg = res.as_pnp_config(base)
    assert list(cfg.camera_matrix) == res.camera_matrix.reshape(-1).tolist() and list(cfg.dist) == res.dist.tolist()
    assert list(cfg.gripper2camera) == list(base.gripper2camera) and (cfg.square_w, cfg.square_h) == (31.0, base.square_h)
    assert abi.lib().rmcv_calib_to_pnp_config(None, None) == abi.ERR_BAD_ARG


def test_defaults_and_every_refusal():
    assert R.calib_defaults() == dict(max_iters=30, fix_mask=0, eps=2.220446049250313e-16)
    c = CC.BY_NAME["s3_3x3"]
    good = dict(corners=c.corners, counts=c.counts, cols=3, rows=3, square=80.0, size=SIZE)
    R.calibrate_camera_host(**good)
    nan_guess = (np.array([np.nan, 0, 1, 0, 1, 1, 0, 0, 1.0]), np.zeros(5))
    neg_guess = (np.array([100.0, 0, 1, 0, -5.0, 1, 0, 0, 1.0]), np.zeros(5))
    bad = [dict(cols=1, rows=3), dict(cols=0, rows=9), dict(cols=4, rows=3), dict(square=0.0), dict(square=-1.0), dict(square=float("nan")), dict(square=float("inf")),
           dict(size=(0, 1024)), dict(size=(1280, 0)), dict(max_iters=0), dict(max_iters=101), dict(fix_mask=-1), dict(fix_mask=512), dict(eps=-1.0),
           dict(eps=float("nan")), dict(eps=float("inf")), dict(guess=nan_guess), dict(guess=neg_guess), dict(corners=np.zeros((4097, 9, 2), np.float32), counts=None),
           dict(corners=np.zeros((0, 9, 2), np.float32), counts=None), dict(corners=np.zeros((3, 1025, 2), np.float32), counts=None, cols=32, rows=32)]
    for change in bad:
        with pytest.raises(RmcvError) as e:
            R.calibrate_camera_host(**dict(good, **change))
        assert e.value.code == abi.ERR_BAD_ARG, change
    L, prm = abi.lib(), abi.calib_params()
    cor, cnt = abi.calib_tables(c.corners, c.counts)
    res, views = abi.calib_outputs(1, 3)
    p = abi.ptr
    for args in ((None, 9, p(cnt), 3, 3, 3, 80.0, 1280, 1024, p(prm), None, p(res), p(views)), (p(cor), 9, None, 3, 3, 3, 80.0, 1280, 1024, p(prm), None, p(res), p(views)),
                 (p(cor), 9, p(cnt), 3, 3, 3, 80.0, 1280, 1024, p(prm), None, None, p(views)), (p(cor), 9, p(cnt), 3, 3, 3, 80.0, 1280, 1024, p(prm), None, p(res), None)):
        assert L.rmcv_calibrate_camera_host(*args) == abi.ERR_BAD_ARG
    assert not res.view(np.uint8).any() and not views.view(np.uint8).any()
    assert L.rmcv_calibrate_camera_host(p(cor), 9, p(cnt), 3, 3, 3, 80.0, 1280, 1024, None, None, p(res), p(views)) == 0      # null parameters: the defaults


# ---- the second opinion: scipy's Levenberg-Marquardt on the textbook model with rvec parameters, started from the truth ----
def rodrigues(r):
    th = math.sqrt(float(r @ r))
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def rvec_from_matrix(Rm):
    q, _ = REF.init_pose([Rm[0, 0], Rm[0, 1], 0.0, Rm[1, 0], Rm[1, 1], 0.0, Rm[2, 0], Rm[2, 1], 1.0], [1.0, 1.0, 0.0, 0.0])
    return np.array(REF.rvec_of(q))


def scipy_opinion(name):
    from scipy.optimize import least_squares
    c = CC.BY_NAME[name]
    use = REF.used_views(c.corners, c.counts, c.cols * c.rows)
    obj = CC.object_points(c.cols, c.rows, c.square)
    obs = np.stack([c.corners[v, :c.cols * c.rows].astype(np.float64) for v in use])
    x0 = np.concatenate([CC.TRUE_A] + [np.concatenate([rvec_from_matrix(c.poses[v][0]), c.poses[v][1]]) for v in use])

    def fun(x):
        K = np.array([[x[0], 0, x[2]], [0, x[1], x[3]], [0, 0, 1.0]])
        return np.concatenate([(CC.project(K, x[4:9], rodrigues(x[9 + 6 * i:12 + 6 * i]), x[12 + 6 * i:15 + 6 * i], obj) - obs[i]).reshape(-1) for i in range(len(use))])

    sol = least_squares(fun, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac", max_nfev=200 * len(x0))
    return sol.x[:9], math.sqrt(float(sol.fun @ sol.fun) / (len(use) * c.cols * c.rows))


@pytest.mark.parametrize("name", CC.FREE)
def test_second_opinion_from_scipy(name):
    (res, _), _ = solved(name)
    a, rms = scipy_opinion(name)
    mine = np.array([res.camera_matrix[0, 0], res.camera_matrix[1, 1], res.camera_matrix[0, 2], res.camera_matrix[1, 2]] + list(res.dist))
    d_px, d_dist = np.abs(mine[:4] - a[:4]).max(), np.abs(mine[4:] - a[4:]).max()
    print("%s: rms %.6g against scipy's %.6g (difference %.3g); |fx fy cx cy| within %.3g px, distortion within %.3g" % (name, res.rms, rms, res.rms - rms, d_px, d_dist))
    assert res.rms <= rms + RMS_MARGIN
    assert d_px <= PIXELS_TOL and d_dist <= DIST_TOL
