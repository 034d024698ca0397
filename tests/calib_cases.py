"""The calibration solve's cases: a seeded list of named sessions.  The truth is the camera and the distortion of the
reference's executable/main.cpp:8-14 (float literals, as that file writes them); a session's boards are turned by angles uniform in +-0.6 rad
about x and y and +-pi about z, stand 500 .. 1100 in front of the camera, and are kept only when every corner lies at least 8 px inside
1280 x 1024; the corners are projected with the full model and rounded to float32.  Shared by the CPU tests, the sanitized program and the
GPU tests; nothing here is changed by them.  These are the GPU shapes too."""
from collections import namedtuple

import numpy as np

W, H = 1280, 1024
f32 = lambda v: float(np.float32(v))
TRUE_K = np.array([[f32(1782.672144409928), 0.0, f32(598.8983414505224)], [0.0, f32(1783.860175007369), f32(523.4209809658056)], [0.0, 0.0, 1.0]])
TRUE_DIST = np.array([f32(-0.03436366268485048), f32(0.1953669264956857), f32(0.0001485060439399386), f32(-0.003814875777013483), f32(-0.3181808766352414)])
TRUE_A = np.array([TRUE_K[0, 0], TRUE_K[1, 1], TRUE_K[0, 2], TRUE_K[1, 2]] + list(TRUE_DIST))

# corners (n_views, per_frame, 2) float32, counts (n_views,) int32, view_camera (n_views,) int32 or None, params and guess as the entry points take them
Case = namedtuple("Case", "name corners counts cols rows square params guess poses")
Fleet = namedtuple("Fleet", "name corners counts view_camera n_cameras cols rows square params cameras")
CASES = []


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def project(K, dist, R, t, obj):
    Xc = obj @ R.T + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], 1)


def object_points(cols, rows, square):
    k = np.arange(cols * rows)
    return np.stack([(k % cols) * square, (k // cols) * square, np.zeros(cols * rows)], 1).astype(np.float64)


def session(seed, n_views, cols, rows, square, noise=0.0, per_frame=None, K=TRUE_K, dist=TRUE_DIST):
    """(corners (n_views, per_frame, 2) float32 with NaN behind a view's corners, the poses (R, t) they were drawn from)"""
    rng = np.random.default_rng(seed)
    obj = object_points(cols, rows, square)
    mid = obj.mean(0)
    P, per = cols * rows, per_frame or cols * rows
    out, poses = np.full((n_views, per, 2), np.nan, np.float32), []
    while len(poses) < n_views:
        R = rotation(rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), rng.uniform(-np.pi, np.pi))
        z = rng.uniform(500.0, 1100.0)
        t = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.25, 0.25) * z, z]) - R @ mid
        px = project(K, dist, R, t, obj)
        if px[:, 0].min() < 8 or px[:, 1].min() < 8 or px[:, 0].max() > W - 8 or px[:, 1].max() > H - 8:
            continue
        if noise:
            px = px + rng.normal(0.0, noise, px.shape)
        out[len(poses), :P] = px.astype(np.float32)
        poses.append((R, t))
    return out, poses


def add(name, seed, n_views, cols, rows, square, noise=0.0, per_frame=None, params=None, guess=None):
    c, poses = session(seed, n_views, cols, rows, square, noise, per_frame)
    CASES.append(Case(name, c, np.full(n_views, cols * rows, np.int32), cols, rows, float(square), dict(params or {}), guess, poses))
    return CASES[-1]


# the minimum set
add("s5_11x8", 101, 5, 11, 8, 30)                        # P = 88: ragged across the 64 lanes, two rounds
add("s19_4x3", 102, 19, 4, 3, 60, per_frame=16)          # P < 64, more views than a workgroup has wavefronts, a row pitch beyond P
add("s3_3x3", 103, 3, 3, 3, 80)                          # the minimum
add("s12_noise", 104, 12, 8, 6, 40, noise=0.1)           # sigma = 0.1 px
# k3 and both tangential terms held at their start (0); a guess in place of the initial intrinsics
FIX_MASK = 256 | 64 | 128
CASES.append(CASES[0]._replace(name="s5_11x8_fix", params=dict(fix_mask=FIX_MASK)))
GUESS = (np.array([1800.0, 0, 640.0, 0, 1800.0, 512.0, 0, 0, 1.0]), np.array([0.0, 0.05, 0.0, 0.0, 0.0]))
CASES.append(CASES[1]._replace(name="s19_4x3_guess", guess=GUESS))
CASES.append(CASES[1]._replace(name="s19_4x3_guess_fix", guess=GUESS, params=dict(fix_mask=FIX_MASK | 32, max_iters=12)))   # (k2 stays 0.05 too)


def with_skips():
    """s12's board again, nine views of which one has count 0, one a count short by one, one a NaN and one an infinity: five are used"""
    c, poses = session(105, 9, 8, 6, 40)
    counts = np.full(9, 48, np.int32)
    counts[1], counts[4] = 0, 47
    c[6, 17, 1] = np.nan
    c[7, 47, 0] = np.inf
    CASES.append(Case("s9_skips", c, counts, 8, 6, 40.0, {}, None, poses))


with_skips()
BY_NAME = {c.name: c for c in CASES}
# sessions whose result is compared with the truth and with scipy (clean or noisy, every parameter free, the library's own start)
FREE = ("s5_11x8", "s19_4x3", "s3_3x3", "s12_noise", "s9_skips")


def fleet():
    """three cameras of a 4 x 3 board, their views interleaved through view_camera: camera 0 has 6 used views (two of them through indices outside
    0 .. 2, which mean camera 0), camera 1 has 5, camera 2 is left with 2 (a third has a NaN, a fourth count 0)"""
    cams = {0: session(201, 6, 4, 3, 60)[0], 1: session(202, 5, 4, 3, 60)[0], 2: session(203, 4, 4, 3, 60)[0]}
    order = [0, 1, 2, 0, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0]
    labels = [0, 1, 2, 7, 1, 0, 2, 1, -1, 2, 1, 0, 2, 1, 0]
    taken = {0: 0, 1: 0, 2: 0}
    corners, counts = np.full((len(order), 12, 2), np.nan, np.float32), np.full(len(order), 12, np.int32)
    for v, cam in enumerate(order):
        corners[v] = cams[cam][taken[cam]]
        taken[cam] += 1
    third, fourth = [v for v, cam in enumerate(order) if cam == 2][2:]
    corners[third, 5, 0] = np.nan
    counts[fourth] = 0
    return Fleet("fleet3_4x3", corners, counts, np.array(labels, np.int32), 3, 4, 3, 60.0, {}, np.array(order, np.int32))


FLEET = fleet()


def alone(fl, cam):
    """(corners, counts, the views' indices in the fleet's tables) of camera `cam`'s views of a fleet, as a session of its own"""
    idx = np.nonzero(fl.cameras == cam)[0]
    return fl.corners[idx], fl.counts[idx], idx
