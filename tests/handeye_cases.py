"""The hand-eye solve's cases: a seeded list of named sessions drawn from a known mounting.  The truth is the h_gripper2camera of
the reference's executable/main.cpp:15-19 as the library's default pnp config carries it, its rotation made exactly orthonormal through its
quaternion; lengths are millimetres as there.  A session's board stands still in the base frame, 1.5 m in front of the camera at zero attitude,
tilted by up to 0.3 rad; the gimbal takes attitudes uniform in +-0.4 (pitch), +-0.5 (yaw), +-0.2 (roll) rad, and each view's board-to-camera
pose follows from board, attitude and mounting.  Poses are given directly as rmcv_calib_view rows (q, tvec, used = 1; rvec and rms, which the
solve does not read, are 0).  Shared by the CPU tests, the sanitized program and the GPU tests; nothing here is changed by them.  These are the
GPU shapes too."""
from collections import namedtuple

import numpy as np

import calib_cases as CC
from rmcv_amd import abi

Case = namedtuple("Case", "name views attitudes gripper_t params")
Fleet = namedtuple("Fleet", "name views attitudes view_camera n_cameras cameras")
CASES = []


def quat_of(R):
    """(w, x, y, z) of a rotation matrix, w >= 0 (Shepperd's largest-diagonal branch), unit"""
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([1 + t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + R[2, 2] - R[0, 0] - R[1, 1]])
    q = q / np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def rot_of(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


_G = np.array(list(abi.default_pnp_config().gripper2camera), np.float64).reshape(4, 4)
TRUE_Q = quat_of(_G[:3, :3])
TRUE_R, TRUE_T = rot_of(TRUE_Q), _G[:3, 3].copy()
BOARD_OUT = 1500.0


def mounting(seed):
    """another camera's mounting: the truth turned by up to 0.2 rad and moved by up to 30 mm"""
    rng = np.random.default_rng(seed)
    R = TRUE_R @ CC.rotation(*rng.uniform(-0.2, 0.2, 3))
    return rot_of(quat_of(R)), TRUE_T + rng.uniform(-30.0, 30.0, 3)


def session(seed, n_views, noise=(0.0, 0.0), gripper_t=False, attitudes=None, flip=0.0, negate_w=False, R_X=TRUE_R, t_X=TRUE_T):
    """(views CALIB_VIEW (n,), attitudes ATTITUDE (n,), gripper_t (n, 3) | None).  noise: (rad, mm) sigma on the poses; attitudes: (n, 3)
    (roll, pitch, yaw) in place of the drawn ones; flip: the board is turned by this angle about its normal; negate_w: every second view's q is negated"""
    rng = np.random.default_rng(seed)
    R_w = R_X @ CC.rotation(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), flip + rng.uniform(-0.3, 0.3))
    t_w = R_X @ np.array([rng.uniform(-100, 100), rng.uniform(-100, 100), BOARD_OUT]) + t_X
    att = np.stack([rng.uniform(-0.2, 0.2, n_views), rng.uniform(-0.4, 0.4, n_views), rng.uniform(-0.5, 0.5, n_views)], 1)
    if attitudes is not None:
        att = np.asarray(attitudes, np.float64)
    tg = rng.uniform(-50.0, 50.0, (n_views, 3)) if gripper_t else None
    views, atts = np.zeros(n_views, abi.CALIB_VIEW), np.zeros(n_views, abi.ATTITUDE)
    atts["roll"], atts["pitch"], atts["yaw"] = att[:, 0], att[:, 1], att[:, 2]
    for v in range(n_views):
        B = CC.rotation(att[v, 0], att[v, 1], att[v, 2])
        R_c = R_X.T @ B.T @ R_w
        t_c = R_X.T @ (B.T @ (t_w - (tg[v] if gripper_t else 0.0)) - t_X)
        if noise[0] or noise[1]:
            R_c = R_c @ CC.rotation(*rng.normal(0.0, noise[0], 3))
            t_c = t_c + rng.normal(0.0, noise[1], 3)
        q = quat_of(R_c)
        views["q"][v] = -q if (negate_w and v % 2) else q
        views["tvec"][v] = t_c
        views["used"][v] = 1
    return views, atts, tg


def add(name, seed, n_views, params=None, **kw):
    CASES.append(Case(name, *session(seed, n_views, **kw), dict(params or {})))
    return CASES[-1]


add("v3", 301, 3)                                   # the minimum: 3 pairs
add("v5", 302, 5)
add("v23", 303, 23)                                 # 253 pairs: under one pair per thread
add("v24", 304, 24)                                 # 276 pairs: over it
add("v65", 305, 65)                                 # past one wavefront of views
add("v256", 306, 256)                               # the cap: 32640 pairs
add("v257_too_many", 307, 257)
add("v12_noise", 308, 12, noise=(1e-3, 1.0))        # 1 mrad, 1 mm
add("v9_gripper_t", 309, 9, gripper_t=True)
add("v8_upside_down", 310, 8, flip=np.pi, negate_w=True)


def special():
    # views that are skipped: not used, a NaN in the pose's quaternion, an infinite tvec, a NaN attitude: five of nine are used
    views, atts, _ = session(311, 9)
    views["used"][1] = 0
    views["q"][3][2] = np.nan
    views["tvec"][4][0] = np.inf
    atts["pitch"][7] = np.nan
    CASES.append(Case("v9_skips", views, atts, None, {}))
    # ... and a NaN among the gripper translations
    views, atts, tg = session(312, 6, gripper_t=True)
    tg[2, 1] = np.nan
    CASES.append(Case("v6_gripper_t_skip", views, atts, tg, {}))
    # one view turned by 170 degrees of yaw: its nine pairs are skipped
    rng = np.random.default_rng(313)
    att = np.stack([rng.uniform(-0.2, 0.2, 10), rng.uniform(-0.4, 0.4, 10), rng.uniform(-0.5, 0.5, 10)], 1)
    att[6] = (0.0, 0.0, np.radians(170.0))
    CASES.append(Case("v10_turned", *session(314, 10, attitudes=att), {}))
    # the same with min_w = 0: nothing is skipped
    CASES.append(CASES[-1]._replace(name="v10_turned_min_w0", params=dict(min_w=0.0)))
    # yaw alone: the translation along the yaw axis cannot be observed, and the rotation about it neither
    att = np.zeros((8, 3))
    att[:, 2] = np.linspace(-0.5, 0.5, 8)
    CASES.append(Case("v8_yaw_only", *session(315, 8, attitudes=att), {}))
    # every pair skipped: min_w so high that only turns under 5 degrees would pass
    CASES.append(CASES[0]._replace(name="v3_all_skipped", params=dict(min_w=0.999)))


special()
BY_NAME = {c.name: c for c in CASES}
# sessions whose result is compared with the truth and with the second opinion: clean, and the noisy one
CLEAN = ("v3", "v5", "v23", "v24", "v65", "v256", "v9_gripper_t", "v8_upside_down", "v9_skips", "v6_gripper_t_skip", "v10_turned", "v10_turned_min_w0")
NOISY = ("v12_noise",)


def fleet():
    """three cameras with mountings of their own, their views interleaved through view_camera: camera 0 has 6 used views (two of them through
    indices outside 0 .. 2, which mean camera 0), camera 1 has 5, camera 2 is left with 2 (a third has a NaN, a fourth is not used)"""
    mounts = {0: (TRUE_R, TRUE_T), 1: mounting(401), 2: mounting(402)}
    cams = {k: session(410 + k, n, R_X=mounts[k][0], t_X=mounts[k][1]) for k, n in ((0, 6), (1, 5), (2, 4))}
    order = [0, 1, 2, 0, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0]
    labels = [0, 1, 2, 7, 1, 0, 2, 1, -1, 2, 1, 0, 2, 1, 0]
    taken = {0: 0, 1: 0, 2: 0}
    views, atts = np.zeros(len(order), abi.CALIB_VIEW), np.zeros(len(order), abi.ATTITUDE)
    for v, cam in enumerate(order):
        views[v], atts[v] = cams[cam][0][taken[cam]], cams[cam][1][taken[cam]]
        taken[cam] += 1
    third, fourth = [v for v, cam in enumerate(order) if cam == 2][2:]
    views["tvec"][third][1] = np.nan
    views["used"][fourth] = 0
    return Fleet("fleet3", views, atts, np.array(labels, np.int32), 3, np.array(order, np.int32)), mounts


FLEET, FLEET_MOUNTS = fleet()


def alone(fl, cam):
    """(views, attitudes, the views' indices in the fleet's tables) of camera `cam`'s views of a fleet, as a session of its own"""
    idx = np.nonzero(fl.cameras == cam)[0]
    return fl.views[idx], fl.attitudes[idx], idx
