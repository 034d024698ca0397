"""One seeded case list for the pose stage (rm::solve_PnP = undistortPoints + IPPE for a square, then the world transform), pure numpy:
tests/test_pose_cases_cpu.py holds the oracle (oracle/rmcv_oracle_pnp.c) and the mpmath restatement (tests/pose_ref.py) against each other on
it and asserts that it reaches every counter of the oracle's pose census; tests/test_gpu_pose_cases.py sends the same list through every route
that reaches k_pnp on the device.

A case is (name, configuration name, vertices float32 [4, 2], family).  Vertices as the detector makes them: [0] top-left, [1] bottom-left,
[2] bottom-right, [3] top-right (image y grows downwards); solve_PnP feeds them in the order 1, 2, 3, 0.  configs() are the configurations by
name.  WELL_POSED are the families whose values are compared with mpmath; the others ("wild") are compared in their decisions only."""
import functools

import numpy as np

import camera_cases
from rmcv_amd import default_pnp_config
from test_oracle_pnp import project, rodrigues

SEED = 20250911
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-42))
WELL_POSED = ("projected", "detector", "roll")
SPECIAL_VALUES = [("nan", float("nan")), ("pinf", float("inf")), ("ninf", float("-inf")), ("nzero", -0.0), ("fltmax", FLT_MAX),
                  ("nfltmax", -FLT_MAX), ("denormal", DENORMAL)]
CENTRED_HALVES = (1, 2, 8, 64, 100, 256)
# the degenerate plates (square_w, square_h): the gamma2 exit (zero, tiny, inf, NaN), the gamma exit (huge), and the two that solve all the same
SQUARES = {"sq_zero": (0.0, 0.0), "sq_zero_w": (0.0, 5.0), "sq_tiny": (1e-30, 1e-30), "sq_inf": (float("inf"), float("inf")),
           "sq_nan": (float("nan"), 27.0), "sq_huge20": (1e20, 1e20), "sq_huge30": (1e30, 1e30), "sq_huge38": (3e38, 3e38),
           "sq_negative": (-27.0, -27.0), "sq_mixed": (27.0, -27.0)}
DEGENERATE_SQUARES = ("sq_zero", "sq_zero_w", "sq_tiny", "sq_inf", "sq_nan", "sq_huge20", "sq_huge30", "sq_huge38")
ICDIST_SQUARE = ((600, 500), (600, 560), (660, 560), (660, 500))


def pow2_camera():
    """no distortion, fx = fy = 1024, cx = cy = 512: pixel -> normalised is exact, a centred square is the frontal pose to the last bit"""
    cfg = default_pnp_config()
    cfg.camera_matrix[0], cfg.camera_matrix[4], cfg.camera_matrix[2], cfg.camera_matrix[5] = 1024.0, 1024.0, 512.0, 512.0
    for i in range(5):
        cfg.dist[i] = 0.0
    return cfg


def icdist_camera():
    """k1 = -0.5 alone: 1 + k1 r^2 turns negative beyond r^2 = 2, where the undistortion gives the point up"""
    cfg = default_pnp_config()
    for i, v in enumerate((-0.5, 0.0, 0.0, 0.0, 0.0)):
        cfg.dist[i] = v
    return cfg


def square_camera(name):
    cfg = default_pnp_config()
    cfg.square_w, cfg.square_h = SQUARES[name]
    return cfg


def k1_huge_camera():
    """k1 = 1e308: 1 + k1 r^2 overflows, 1 / radial is an exact +0 -- not negative, so the rounds go on (and multiply the point by zero)"""
    cfg = default_pnp_config()
    for i, v in enumerate((1e308, 0.0, 0.0, 0.0, 0.0)):
        cfg.dist[i] = v
    return cfg


def fx0_camera():
    cfg = default_pnp_config()
    cfg.camera_matrix[0] = 0.0
    return cfg


@functools.lru_cache(maxsize=None)
def configs():
    """{name: PnpConfig}, in table order (tests/test_gpu_pose_cases.py loads them as one camera table)"""
    out = {"default": default_pnp_config(), "other": camera_cases.other_camera(), "pow2": pow2_camera(), "icdist": icdist_camera()}
    for name in SQUARES:
        out[name] = square_camera(name)
    out["fx0"] = fx0_camera()
    out["k1_huge"] = k1_huge_camera()
    return out


def sq(x0, y0, x1, y1):
    """the detector's axis-aligned square: top-left, bottom-left, bottom-right, top-right"""
    return np.array([(x0, y0), (x0, y1), (x1, y1), (x1, y0)], np.float64)


def centred(s, c=512.0):
    return sq(c - s, c - s, c + s, c + s)


def ulp_neighbours(q):
    """(suffix, quad) for every coordinate moved one float32 ulp up and down"""
    q = np.asarray(q, F32)
    out = []
    for i in range(4):
        for k in range(2):
            for way, to in (("up", np.inf), ("down", -np.inf)):
                n = q.copy()
                n[i, k] = np.nextafter(q[i, k], F32(to))
                out.append(("%d%s_%s" % (i, "xy"[k], way), n))
    return out


def degenerate_quads():
    """(name, quad): coincident, collinear, three-collinear and bow-tie quadrilaterals"""
    base = sq(600, 500, 660, 560)
    out = [("coincident_all", np.tile([[640.0, 520.0]], (4, 1))),
           ("coincident_two_pairs", base[[0, 0, 2, 2]]),
           ("coincident_one_pair", base[[0, 1, 2, 2]]),
           ("collinear_horizontal", np.array([(600, 500), (620, 500), (640, 500), (660, 500)], float)),
           ("collinear_vertical", np.array([(600, 500), (600, 520), (600, 540), (600, 560)], float)),
           ("collinear_diagonal", np.array([(600, 500), (620, 520), (640, 540), (660, 560)], float)),
           ("collinear_diagonal_fractional", np.array([(600.25, 500.5), (620.25, 520.5), (640.25, 540.5), (660.25, 560.5)], float)),
           ("bow_tie_01", base[[1, 0, 2, 3]]),
           ("bow_tie_12", base[[0, 2, 1, 3]])]
    for k in range(4):                                    # vertex k on the line through its two neighbours' ... the other three stay
        q = base.copy()
        q[k] = (base[(k + 1) % 4] + base[(k + 3) % 4]) / 2
        out.append(("three_collinear_%d" % k, q))
    return out


def random_pose(rng, tilt_lo, tilt_hi, depth_lo=200.0, depth_hi=20000.0):
    """(R, t): the plate tilted by an angle in [tilt_lo, tilt_hi] degrees about a random axis in its plane, turned about its normal, at a
    log-uniform depth and a random place inside the field of view"""
    tilt = np.deg2rad(rng.uniform(tilt_lo, tilt_hi))
    a = rng.uniform(0, 2 * np.pi)
    R = rodrigues(tilt * np.array([np.cos(a), np.sin(a), 0.0])) @ rodrigues(np.array([0.0, 0.0, rng.uniform(-0.5, 0.5)]))
    z = float(np.exp(rng.uniform(np.log(depth_lo), np.log(depth_hi))))
    return R, np.array([rng.uniform(-0.25, 0.25) * z, rng.uniform(-0.2, 0.2) * z, z])


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    cfgs = configs()
    out = []

    def add(name, cfg, q, family):
        q = np.ascontiguousarray(np.asarray(q, F32).reshape(4, 2))
        q.setflags(write=False)
        out.append((name, cfg, q, family))

    # ---- the named cases
    add("icdist_all_four_give_up", "icdist", np.array(ICDIST_SQUARE, float) + 2500.0, "named")
    for cfg in ("default", "icdist"):                                           # the same pixels where the model still holds
        add("icdist_square_in_place_" + cfg, cfg, np.array(ICDIST_SQUARE, float), "named")
    for k, shift in enumerate(np.linspace(0.0, 3000.0, 41)):                    # ... and on the way out: some points give up, some do not
        add("icdist_shift_%02d" % k, "icdist", np.array(ICDIST_SQUARE, float) + shift, "icdist")
        add("icdist_shift_x_%02d" % k, "icdist", np.array(ICDIST_SQUARE, float) * (1.0, 1.0) + (shift, 0.0), "icdist")
    for name in SQUARES:
        add("plate_%s_detector" % name, name, sq(600, 500, 660, 560), "plate")
        add("plate_%s_centre" % name, name, sq(570, 495, 630, 555), "plate")
        for k in range(6):
            R, t = random_pose(rng, 0, 60, 500, 5000)
            add("plate_%s_projected_%d" % (name, k), name, project(R, t, cfgs["default"]), "plate")
    add("fx0_square", "fx0", sq(600, 500, 660, 560), "fx0")
    add("fx0_centre_column", "fx0", sq(598.8983154296875, 500, 660, 560), "fx0")
    for k in range(6):
        add("fx0_random_%d" % k, "fx0", rng.uniform(100, 900, (4, 2)), "fx0")
    add("k1_huge_square", "k1_huge", sq(600, 500, 660, 560), "k1_huge")
    add("k1_huge_centre", "k1_huge", sq(570, 495, 630, 555), "k1_huge")
    add("k1_huge_far", "k1_huge", np.array(ICDIST_SQUARE, float) + 2500.0, "k1_huge")     # r^2 > 2: k1 r^2 overflows, 1 / radial = +0 exactly
    add("k1_huge_farther", "k1_huge", np.array(ICDIST_SQUARE, float) + 3000.0, "k1_huge")
    for k in range(6):
        add("k1_huge_random_%d" % k, "k1_huge", rng.uniform(100, 900, (4, 2)), "k1_huge")
    # 1 - |column|^2 of the SECOND column rounds below zero (the first one's does in near_pi_nan_* and detector_tie_*): the b1 clamp acts on a negative
    for k, q in enumerate(([[482, 492], [482, 532], [522, 532], [522, 492]], [[354, 749], [670, 749], [670, 433], [354, 433]],
                           [[492, 542], [532, 542], [532, 502], [492, 502]], [[690, 512], [334, 512], [334, 868], [690, 868]])):
        add("b1sq_negative_%d" % k, "pow2", q, "named")
    add("huge_vertices_plus", "default", np.full((4, 2), 1e30) * [[1, 1], [1, -1], [-1, -1], [-1, 1]], "wild")
    add("huge_vertices_scaled_square", "default", sq(-1e30, -1e30, 1e30, 1e30), "wild")
    add("huge_vertices_pow2", "pow2", sq(-1e30, -1e30, 1e30, 1e30), "wild")

    # one ulp beside a rotation by pi (a centred square in reversed order): the trace falls below -1 and acos gives NaN
    add("near_pi_nan_0", "pow2", [[555.0, 469.000030517578125], [555.0, 555.0], [469.0, 555.0], [469.0, 469.000030517578125]], "named")
    add("near_pi_nan_1", "pow2", [[734.0, 290.0], [734.0, 733.99993896484375], [290.0, 733.99993896484375], [290.0, 290.0]], "named")
    for s in (1, 64):                                                           # ... and the other one-ulp neighbours of that order and of roll 2
        for suffix, n in ulp_neighbours(centred(s)[::-1]):
            add("near_reversed_%d_%s" % (s, suffix), "pow2", n, "ulp")
        for suffix, n in ulp_neighbours(np.roll(centred(s), -2, axis=0)):
            add("near_roll2_%d_%s" % (s, suffix), "pow2", n, "ulp")

    # ---- every cyclic roll, and the reversal, of a frontal square
    for s in CENTRED_HALVES:
        q = centred(s)
        for r in range(4):
            add("centred_%d_roll%d" % (s, r), "pow2", np.roll(q, -r, axis=0), "roll")
        add("centred_%d_reversed" % s, "pow2", q[::-1], "roll")
    for k in range(10):                                                         # off-centre, under the default lens: nothing is exact here
        x0, y0, side = rng.integers(50, 1100), rng.integers(50, 900), rng.integers(12, 200)
        q = sq(x0, y0, x0 + side, y0 + side)
        for r in range(4):
            add("frontal_%d_roll%d" % (k, r), "default", np.roll(q, -r, axis=0), "roll")
        add("frontal_%d_reversed" % k, "default", q[::-1], "roll")

    # ---- special values, one at a time and all four
    base = sq(600, 500, 660, 560)
    for cfg in ("default", "pow2"):
        for vname, val in SPECIAL_VALUES:
            for i in range(4):
                for k in range(2):
                    q = base.copy()
                    q[i, k] = val
                    add("%s_at_%d%s_%s" % (vname, i, "xy"[k], cfg), cfg, q, "special")
            add("%s_all_%s" % (vname, cfg), cfg, np.full((4, 2), val), "special")
            q = base.copy()
            q[:, 0] = val
            add("%s_all_x_%s" % (vname, cfg), cfg, q, "special")

    # ---- degenerate quadrilaterals with and without distortion, and their one-ulp neighbours
    for cfg in ("pow2", "default", "other"):
        for name, q in degenerate_quads():
            add("%s_%s" % (name, cfg), cfg, q, "degenerate")
    for name, q in degenerate_quads():
        if name.startswith("collinear"):
            for suffix, n in ulp_neighbours(q):
                add("near_%s_%s" % (name, suffix), "pow2", n, "ulp")
    for s in (1, 64):
        for suffix, n in ulp_neighbours(centred(s)):
            add("near_centred_%d_%s" % (s, suffix), "pow2", n, "ulp")

    # ---- projected poses: up to 80 degrees of tilt (compared with mpmath in value), and grazing ones beyond (decisions only)
    for k in range(360):
        cfg = ("default", "default", "other", "pow2")[k % 4]
        R, t = random_pose(rng, 0, 80)
        add("projected_%03d" % k, cfg, project(R, t, cfgs[cfg], distort=cfg != "pow2"), "projected")
    for k in range(120):
        cfg = ("default", "other", "pow2")[k % 3]
        R, t = random_pose(rng, 80, 89)
        add("grazing_%03d" % k, cfg, project(R, t, cfgs[cfg], distort=cfg != "pow2"), "grazing")

    # ---- the detector's shape: axis-aligned squares at integer and half-integer corners across a 1920 x 1200 frame
    for k in range(480):
        cfg = ("default", "default", "default", "other", "pow2", "sq_mixed", "sq_negative", "icdist")[k % 8]
        side = int(rng.integers(2, 400)) / 2.0
        x0, y0 = int(rng.integers(0, 2 * (1920 - 200))) / 2.0, int(rng.integers(0, 2 * (1200 - 200))) / 2.0
        add("detector_%03d" % k, cfg, sq(x0, y0, x0 + side, y0 + side), "detector" if cfg in ("default", "other", "pow2") else "detector_wild")
    for k in range(60):                                                         # around the principal point of the exact camera: ties of ea and eb
        side = int(rng.integers(1, 200))
        x0, y0 = 512 - side + int(rng.integers(-2, 3)) * side // 2, 512 - side + int(rng.integers(-2, 3)) * side // 2
        add("detector_tie_%02d" % k, "pow2", sq(x0, y0, x0 + 2 * side, y0 + 2 * side), "detector")

    # ---- random quadrilaterals
    names = list(cfgs)
    for k in range(240):
        cfg = names[k % len(names)]
        add("random_%03d" % k, cfg, rng.uniform(-200, 2200, (4, 2)) if k % 5 == 0 else rng.uniform(100, 900, (4, 2)), "random")
    assert len({c[0] for c in out}) == len(out)
    return out


def by_config():
    """{configuration name: [index into cases()]}"""
    out = {name: [] for name in configs()}
    for i, (_, cfg, _, _) in enumerate(cases()):
        out[cfg].append(i)
    return out


def vertices_of(indices):
    c = cases()
    return np.stack([c[i][2] for i in indices]) if len(indices) else np.zeros((0, 4, 2), F32)


def to_oracle_cfg(oracle, cfg):
    return camera_cases.to_oracle_cfg(oracle, cfg)


def same_bytes_but_nan(got, want):
    """the comparison rule of the device tests: raw bytes, except that a NaN matches any NaN (sign and payload of a generated NaN differ
    between x86 and the GPU; the reference promises neither).  -> (equal, number of NaN values in want)"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return False, 0
    gn, wn = np.isnan(got), np.isnan(want)
    ok = np.array_equal(gn, wn) and np.array_equal(got.view(np.uint64)[~wn], want.view(np.uint64)[~wn])
    return bool(ok), int(wn.sum())
