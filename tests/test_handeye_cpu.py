"""The hand-eye solve on the CPU: rmcv_calibrate_hand_eye_host against tests/handeye_ref.py, the numpy restatement of the text at
the head of rmcv_amd/csrc/device_handeye.h -- bit for bit on every field of the result and every view row for every case of
tests/handeye_cases.py; the truth recovered; every refusal; both converters; cam2gripper and world assembled as
executable/calibration/hand_eye.cpp:165-176 does; the fleet's cameras; and a second opinion from numpy.linalg.eigh and numpy.linalg.lstsq on
the same M, N and r built in plain numpy order.  No GPU."""
import numpy as np
import pytest

import handeye_cases as HC
import handeye_ref as REF
import rmcv_amd as R
from rmcv_amd import RmcvError, abi

NAMES = [c.name for c in HC.CASES]
# The second opinion and the truth, measured here on the CPU; each bound is 8 x the largest measured value.
#   against the second opinion, over HC.CLEAN and HC.NOISY: the angle between the library's R_X and eigh's at most 1.94e-13 deg (v256; the
#       noisy session 3.37e-14), |t_X - lstsq's| at most 5.25e-13 mm (v3; the noisy session 1.84e-13)
#   against the truth, clean sessions: at most 3.61e-14 deg (v9_skips) and 7.23e-13 mm (v3)
#   against the truth, the noisy session (1 mrad, 1 mm on 12 poses): 0.0303 deg and 3.63 mm
OPINION_DEG, OPINION_MM = 8 * 1.94e-13, 8 * 5.25e-13
CLEAN_DEG, CLEAN_MM = 8 * 3.61e-14, 8 * 7.23e-13
NOISY_DEG, NOISY_MM = 8 * 0.0303, 8 * 3.63

bits = lambda x: np.asarray(x, np.float64).tobytes()
_memo = {}


def solved(name):
    """(the library's (HandEyeResult, rows), the restatement's (Result | Counts, {view: world})) of a case, computed once"""
    if name not in _memo:
        c = HC.BY_NAME[name]
        lib = R.calibrate_hand_eye_host(c.views, c.attitudes, c.gripper_t, c.params)
        ref = REF.solve(c.views, c.attitudes, c.gripper_t, **dict(REF.DEFAULTS, **c.params))
        _memo[name] = (lib, ref)
    return _memo[name]


def angle_deg(q, p):
    """the angle between the rotations of two unit quaternions"""
    d = abs(float(np.dot(q, p)))
    v = np.linalg.norm(q - p if np.dot(q, p) > 0 else q + p)       # (2 asin(|dq| / 2): exact for small angles where acos is not)
    return float(np.degrees(2 * np.arcsin(min(1.0, v / 2)))) if d <= 1.5 else float("nan")


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_restatement_bit_for_bit(name):
    (res, rows), (ref, world) = solved(name)
    c = HC.BY_NAME[name]
    if isinstance(ref, REF.Result):
        rec, rrows = REF.records(ref, world, len(c.views))
        for k in abi.HANDEYE_RESULT.names:
            assert np.asarray(res.rec[k]).tobytes() == np.asarray(rec[k][0]).tobytes(), k
        assert rows.tobytes() == rrows.tobytes()
        assert res.solved and res.pairs_used + res.pairs_skipped == res.views_used * (res.views_used - 1) // 2
    else:
        assert (res.status, res.views_used, res.pairs_used, res.pairs_skipped, res.sweeps) == tuple(ref)
        want = np.zeros(1, abi.HANDEYE_RESULT)
        for k in ref._fields:
            want[k][0] = getattr(ref, k)
        assert np.array(res.rec).reshape(1).tobytes() == want.tobytes() and not rows.view(np.uint8).any() and not res.solved


def test_the_cases_exercise_what_they_are_named_for():
    pairs = lambda name: (solved(name)[0][0].pairs_used, solved(name)[0][0].pairs_skipped)
    assert pairs("v3") == (3, 0) and pairs("v23") == (253, 0) and pairs("v24") == (276, 0) and pairs("v65") == (2080, 0) and pairs("v256") == (32640, 0)
    assert pairs("v10_turned") == (36, 9) and pairs("v10_turned_min_w0") == (45, 0)
    (res, rows), _ = solved("v257_too_many")
    assert (res.status, res.views_used) == (R.HANDEYE_TOO_MANY_VIEWS, 257) and not rows["used"].any()
    (res, rows), _ = solved("v3_all_skipped")
    assert (res.status, res.views_used, res.pairs_used, res.pairs_skipped) == (R.HANDEYE_TOO_FEW_VIEWS, 3, 0, 3)
    (res, rows), _ = solved("v9_skips")
    assert rows["used"].tolist() == [1, 0, 1, 0, 0, 1, 1, 0, 1] and res.views_used == 5
    (res, rows), _ = solved("v6_gripper_t_skip")
    assert rows["used"].tolist() == [1, 1, 0, 1, 1, 1]
    assert (HC.BY_NAME["v8_upside_down"].views["q"][:, 0] < 0).sum() >= 3                        # quaternions with negative w went in
    (res, _), _ = solved("v8_yaw_only")                                                         # degenerate: two eigenvalues at zero, the last pivot fails
    assert res.status == R.HANDEYE_T_UNOBSERVABLE and abs(res.eig[1]) < 1e-12 * res.eig[3] and not res.pivots[2] > 0.0
    c = HC.BY_NAME["v3"]
    res, rows = R.calibrate_hand_eye_host(c.views[:2], c.attitudes[:2])
    assert (res.status, res.views_used, res.pairs_used) == (R.HANDEYE_TOO_FEW_VIEWS, 2, 0) and not rows["used"].any() and not res.cam2gripper.any()


@pytest.mark.parametrize("name", HC.CLEAN + HC.NOISY)
def test_the_truth_is_recovered(name):
    (res, _), _ = solved(name)
    ang, dt = angle_deg(res.q, HC.TRUE_Q), float(np.linalg.norm(res.t - HC.TRUE_T))
    print("%s: against the truth %.3g deg, %.3g mm; rot_rms %.3g, trans_rms %.3g, world_rms %.3g" % (name, ang, dt, res.rot_rms, res.trans_rms, res.world_rms))
    assert res.status == R.HANDEYE_OK
    assert ang <= (NOISY_DEG if name in HC.NOISY else CLEAN_DEG) and dt <= (NOISY_MM if name in HC.NOISY else CLEAN_MM)


def test_skipped_views_are_as_if_absent():
    c = HC.BY_NAME["v9_skips"]
    (res, rows), _ = solved("v9_skips")
    keep = rows["used"] == 1
    alone, arows = R.calibrate_hand_eye_host(c.views[keep], c.attitudes[keep])
    assert np.array(alone.rec).tobytes() == np.array(res.rec).tobytes() and arows.tobytes() == rows[keep].tobytes()
    assert rows[~keep].tobytes() == bytes(4 * abi.HANDEYE_VIEW.itemsize)


def test_cam2gripper_and_world_as_the_reference_assembles_them():
    """hand_eye.cpp:165-176: h_gripper2camera = eye with R and t copied in; world = h_base2gripper * (h_gripper2camera * camera_position)"""
    for name in ("v5", "v9_gripper_t", "v12_noise"):
        c = HC.BY_NAME[name]
        (res, rows), _ = solved(name)
        w, x, y, z = res.q
        RX = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                       [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])
        G = R.homogeneous(RX, res.t)
        assert bits(G) == bits(res.cam2gripper) and bits(G[3]) == bits([0.0, 0.0, 0.0, 1.0])
        prod = lambda M, v: [((M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2]) + M[r][3] * v[3] for r in range(4)]     # (a 4 x 4 times a 4 x 1, left to right)
        for v in range(len(c.views)):
            att = c.attitudes[v]
            H = R.homogeneous(R.euler_to_matrix((att["roll"], att["pitch"], att["yaw"])), None if c.gripper_t is None else c.gripper_t[v])
            cam = [float(c.views["tvec"][v][0]), float(c.views["tvec"][v][1]), float(c.views["tvec"][v][2]), 1.0]
            world = prod(H.tolist(), prod(G.tolist(), cam))
            assert bits(world[:3]) == bits(rows["world"][v]) and world[3] == 1.0, (name, v)


def test_fleet_cameras_alone():
    fl = HC.FLEET
    for cam, want_used in ((0, 6), (1, 5), (2, 2)):
        vw, att, idx = HC.alone(fl, cam)
        res, rows = R.calibrate_hand_eye_host(vw, att)
        assert res.views_used == want_used and res.solved == (cam != 2)
        ref, _ = REF.solve(fl.views, fl.attitudes, None, fl.view_camera, fl.n_cameras, cam)
        assert ref.views_used == want_used
        if cam != 2:
            assert bits(ref.cam2gripper) == bits(res.cam2gripper)
            Rm, tm = HC.FLEET_MOUNTS[cam]
            assert angle_deg(res.q, HC.quat_of(Rm)) <= CLEAN_DEG and np.linalg.norm(res.t - tm) <= CLEAN_MM


def test_both_converters():
    (res, _), _ = solved("v5")
    base = abi.default_pnp_config()
    base.square_w, base.camera_matrix[0] = 31.0, 1700.0
    cfg = res.as_pnp_config(base)
    assert bits(list(cfg.gripper2camera)) == bits(res.cam2gripper)
    assert list(cfg.camera_matrix) == list(base.camera_matrix) and list(cfg.dist) == list(base.dist) and (cfg.square_w, cfg.square_h) == (31.0, base.square_h)
    abase = R.default_attitude_config(motor_angle_mode=R.ATT_MOTOR_PITCH)
    acfg = res.as_attitude_config(abase)
    assert bits(list(acfg.gripper2camera)) == bits(res.cam2gripper) and acfg.motor_angle_mode == R.ATT_MOTOR_PITCH and acfg.reserved == 0
    assert bits(list(res.as_attitude_config().gripper2camera)) == bits(res.cam2gripper)
    (deg, _), _ = solved("v8_yaw_only")                      # a rotation alone: only when asked for
    assert deg.status == R.HANDEYE_T_UNOBSERVABLE and not deg.t.any()
    for call in (deg.as_pnp_config, deg.as_attitude_config):
        with pytest.raises(RmcvError):
            call()
        assert bits(list(call(allow_rotation_only=True).gripper2camera)) == bits(deg.cam2gripper)
    (none, _), _ = solved("v257_too_many")                   # no rotation: never
    for call in (none.as_pnp_config, none.as_attitude_config):
        for allow in (False, True):
            with pytest.raises(RmcvError):
                call(allow_rotation_only=allow)
    L = abi.lib()
    assert L.rmcv_handeye_to_pnp_config(None, None, 0) == abi.ERR_BAD_ARG and L.rmcv_handeye_to_attitude_config(None, None, 1) == abi.ERR_BAD_ARG


def test_defaults_and_every_refusal():
    assert R.handeye_defaults() == dict(min_w=0.5)
    c = HC.BY_NAME["v3"]
    R.calibrate_hand_eye_host(c.views, c.attitudes)
    for min_w in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(RmcvError) as e:
            R.calibrate_hand_eye_host(c.views, c.attitudes, min_w=min_w)
        assert e.value.code == abi.ERR_BAD_ARG, min_w
    for n in (0, 4097):
        with pytest.raises(RmcvError) as e:
            R.calibrate_hand_eye_host(np.zeros(n, abi.CALIB_VIEW), np.zeros(n, abi.ATTITUDE))
        assert e.value.code == abi.ERR_BAD_ARG
    L, prm, p = abi.lib(), abi.handeye_params(), abi.ptr
    vw, att, _ = abi.handeye_tables(c.views, c.attitudes)
    res, rows = abi.handeye_outputs(1, 3)
    for args in ((None, p(att), None, 3, p(prm), p(res), p(rows)), (p(vw), None, None, 3, p(prm), p(res), p(rows)), (p(vw), p(att), None, 3, p(prm), None, p(rows)),
                 (p(vw), p(att), None, 3, p(prm), p(res), None)):
        assert L.rmcv_calibrate_hand_eye_host(*args) == abi.ERR_BAD_ARG
    assert not res.view(np.uint8).any() and not rows.view(np.uint8).any()
    assert L.rmcv_calibrate_hand_eye_host(p(vw), p(att), None, 3, None, p(res), p(rows)) == 0      # null parameters: the defaults
    assert res.tobytes() == np.array(solved("v3")[0][0].rec).reshape(1).tobytes()


# ---- the second opinion: M, N and r summed in plain numpy order, numpy.linalg.eigh for the rotation, numpy.linalg.lstsq for the translation ----
def opinion(name):
    c = HC.BY_NAME[name]
    use = REF.used_views(c.views, c.attitudes, c.gripper_t)
    min_w = dict(REF.DEFAULTS, **c.params)["min_w"]
    B = [R.euler_to_matrix((c.attitudes["roll"][v], c.attitudes["pitch"][v], c.attitudes["yaw"][v])) for v in use]
    Rc = [HC.rot_of(c.views["q"][v] / np.linalg.norm(c.views["q"][v])) for v in use]
    tc = [np.array(c.views["tvec"][v]) for v in use]
    tg = [np.zeros(3) if c.gripper_t is None else np.array(c.gripper_t[v]) for v in use]
    Lm = lambda q: np.array([[q[0], -q[1], -q[2], -q[3]], [q[1], q[0], -q[3], q[2]], [q[2], q[3], q[0], -q[1]], [q[3], -q[2], q[1], q[0]]])
    Rm = lambda q: np.array([[q[0], -q[1], -q[2], -q[3]], [q[1], q[0], q[3], -q[2]], [q[2], -q[3], q[0], q[1]], [q[3], q[2], -q[1], q[0]]])
    pairs = []
    for i in range(len(use)):
        for j in range(i + 1, len(use)):
            RA, RB = B[j].T @ B[i], Rc[j] @ Rc[i].T
            a, b = HC.quat_of(RA), HC.quat_of(RB)
            if a[0] >= min_w and b[0] >= min_w:
                pairs.append((a, b, RA, B[j].T @ (tg[i] - tg[j]), tc[j] - RB @ tc[i]))
    M = np.sum([(Lm(a) - Rm(b)).T @ (Lm(a) - Rm(b)) for a, b, *_ in pairs], 0)
    w, V = np.linalg.eigh(M)
    q = V[:, 0] / np.linalg.norm(V[:, 0])
    q = q if q[0] >= 0 else -q
    RX = HC.rot_of(q)
    C = np.concatenate([RA - np.eye(3) for _, _, RA, _, _ in pairs])
    g = np.concatenate([RX @ tB - tA for _, _, _, tA, tB in pairs])
    N, r = C.T @ C, C.T @ g
    t = np.linalg.lstsq(N, r, rcond=None)[0]
    return q, t


@pytest.mark.parametrize("name", HC.CLEAN + HC.NOISY)
def test_second_opinion_from_eigh_and_lstsq(name):
    (res, _), _ = solved(name)
    q, t = opinion(name)
    ang, dt = angle_deg(res.q, q), float(np.linalg.norm(res.t - t))
    print("%s: against eigh %.3g deg, against lstsq %.3g mm" % (name, ang, dt))
    assert ang <= OPINION_DEG and dt <= OPINION_MM
