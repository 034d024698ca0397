"""Aiming on the CPU: the four host functions (rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance) and rmcv_aim_step_host -- the source
k_aim is compiled from (rmcv_amd/csrc/device_aim.h) -- against tests/aim_ref.c, an independently written restatement, byte for byte; a
seeded sweep against the same restatement in Python's math; the pinned reference against its host-libm build (the second opinion)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import aim_cases as K
import aim_ref as R
import track_scenarios as S
import rmcv_amd
from rmcv_amd import abi
from rmcv_amd.tracker import AimConfig, Tracker, default_aim_config, default_tracker_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, CLASSIC, NI = abi.COMPENSATE_NONE, abi.COMPENSATE_CLASSIC, abi.COMPENSATE_NI
TVECS = [(10.0, -5.0, 300.0), (0.0, 0.0, 800.0), (-40.0, 20.0, 150.0), (5.0, 5.0, 2500.0)]

# The second opinion's bound, MEASURED on this file's sweep and step cases (printed by the tests below): the largest distance
# in ulps between a double of the pinned build and of the host-libm build.  Well-conditioned outputs differ by 3 ulp at the most (yaw, the
# pitch and time of COMPENSATE_NONE); the maximum belongs to the two ill-conditioned ones of COMPENSATE_CLASSIC -- a pitch next to zero,
# where (centerAngle - normalAngle + ...) + targetAngle cancels (1048576 ulp of -2.9e-5 degrees on the sweep), and a flight time whose
# cos(angle in DEGREES) lands next to a zero of the cosine (196462 ulp of 3063 s), which a led point then inherits (3050721 ulp, a step
# case).  A different libm may round differently: x 4.
LIBM_ULPS_OBSERVED = 3050721
LIBM_ULPS_BOUND = 4 * LIBM_ULPS_OBSERVED


def bits(x):
    return np.float64(x).tobytes()


def same(a, b):
    return bits(a) == bits(b)


def ulps(a, b):
    """distance in ulps between doubles of equal sign and class (NaN against NaN: 0)"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN in one build only"
    m = ~np.isnan(a)
    d = np.zeros(a.shape, np.int64)
    ia, ib = a[m].view(np.int64), b[m].view(np.int64)
    ia, ib = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia), np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)   # sign-magnitude -> one ordered line
    d[m] = np.abs(ia - ib)
    return d


# ---------------------------------------------------------------------------------------------------------------- hand cases
def test_projectile_angle_hand_cases():
    a = rmcv_amd.projectile_angle(15, 9.8, 3, 0.2)
    assert same(a, R.projectile_angle(15, 9.8, 3, 0.2)) and 0 < a < 0.01
    z = rmcv_amd.projectile_angle(15, 9.8, 0, 0.2)                       # d = 0: delta == 0, atan(-1 * ((b / 2) * a)) = -0.0
    assert same(z, R.projectile_angle(15, 9.8, 0, 0.2)) and z == 0 and math.copysign(1, z) < 0
    n = rmcv_amd.projectile_angle(15, 9.8, 30, 5)                        # out of range
    assert math.isnan(n) and math.isnan(R.projectile_angle(15, 9.8, 30, 5))
    # the delta == 0 branch with the reference's precedence, (b / 2) * a and not b / (2 a): h = a - d^2 / (4 a) makes delta exactly 0 here
    v0, g, d = 4.0, 8.0, 4.0
    aa = g * d * d / (2 * v0 * v0)
    h = aa - d * d / (4 * aa)
    assert d * d - 4 * aa * (aa - h) == 0
    got = rmcv_amd.projectile_angle(v0, g, d, h)
    assert same(got, R.projectile_angle(v0, g, d, h)) and abs(got - math.atan(-(d / 2 * aa))) < 1e-15 and abs(got - math.atan(-d / (2 * aa))) > 1e-3


@pytest.mark.parametrize("mode", [NONE, CLASSIC])
@pytest.mark.parametrize("v0", [15.0, 28.0])
def test_solve_gea_hand_cases(mode, v0):
    for tv in TVECS:
        for off, ao in (((0.0, 0.0), 0.0), ((1.5, -2.5), 0.01)):
            t, gea = rmcv_amd.solve_gea(tv, 9.8, v0, 20.0, off, ao, mode)
            rt, rgea = R.solve_gea(tv, 9.8, v0, 20.0, off, ao, mode)
            assert same(t, rt) and gea.tobytes() == rgea.tobytes(), (tv, off)
            if mode == CLASSIC and v0 == 15.0 and tv[2] == 2500.0:          # 25 m at 15 m/s: no real root
                assert math.isnan(t) and math.isnan(gea[0]) and math.isfinite(gea[1])
            else:
                assert math.isfinite(t) and np.isfinite(gea).all()
            if mode == NONE:
                assert same(t, tv[2] / 100.0 / v0)
    # the two oddities, as written: cos() of the angle in DEGREES, and h / 100
    tv = TVECS[0]
    t, gea = rmcv_amd.solve_gea(tv, 9.8, 28.0, 20.0, mode=CLASSIC)
    target_deg = rmcv_amd.projectile_angle(28.0, 9.8, 3.0, 20.0 / 100.0) * 180.0 / math.pi
    assert abs(t - 3.0 / abs(28.0 * math.cos(target_deg))) < 1e-12 and abs(t - 3.0 / abs(28.0 * math.cos(math.radians(target_deg)))) > 1e-6


def test_solve_gea_ni_returns_nan_and_leaves_the_output():
    tv = np.array(TVECS[0])
    gea = np.array([7.0, -7.0])
    t = abi.lib().rmcv_solve_gea(abi.ptr(tv), 9.8, 15.0, 20.0, 0.0, 0.0, 0.0, NI, abi.ptr(gea))
    assert math.isnan(t) and gea.tolist() == [7.0, -7.0]
    rt, rgea = R.solve_gea(tv, 9.8, 15.0, 20.0, mode=NI, fill=7.0)
    assert math.isnan(rt) and rgea.tolist() == [7.0, 7.0]
    assert rmcv_amd.solve_gea(tv, 9.8, 15.0, 20.0, mode=NI)[1] is None


def test_delta_height_and_distance_hand_cases():
    for tv in TVECS:
        for motor, oy, ao in ((0.0, 0.0, 0.0), (0.1, -2.5, 0.01), (-0.3, 4.0, -0.02), (1.2, 0.0, 0.0)):
            assert same(rmcv_amd.delta_height(tv, motor, (0.0, oy), ao), R.delta_height(tv, motor, oy, ao))
        assert same(rmcv_amd.distance(tv), R.distance(tv))
    assert rmcv_amd.distance((3, 4, 12)) == 13.0
    # level barrel, target dead ahead and 30 cm up (camera y points down): DeltaHeight gives the 30 cm back
    assert abs(rmcv_amd.delta_height((0.0, -30.0, 400.0), 0.0) - 30.0) < 1e-12


def test_overloads_change_the_chosen_root():
    """bit 0: int abs(int) truncates both roots' angles -- both below 1 rad here -- to 0, `0 < 0` fails and x2, the steeper root, is
    taken.  (A root beyond 1 rad still truncates to 1 and loses as before: the flat shots of a fast projectile do not change.)"""
    x_fabs, x_int = R.projectile_angle(10.0, 9.8, 15.0, 6.0, 0), R.projectile_angle(10.0, 9.8, 15.0, 6.0, 1)
    assert same(x_fabs, rmcv_amd.projectile_angle(10.0, 9.8, 15.0, 6.0))
    a = 9.8 * 15.0 ** 2 / (2 * 10.0 ** 2)
    root = math.sqrt(15.0 ** 2 - 4 * a * (a - 6.0))
    r1, r2 = (-15.0 + root) / (2 * a), (-15.0 - root) / (2 * a)
    assert abs(math.atan(r1)) < abs(math.atan(r2)) < 1.0                         # both truncate to 0
    assert abs(x_fabs - math.atan(r1)) < 1e-14 and abs(x_int - math.atan(r2)) < 1e-14 and x_int < x_fabs - 0.1
    assert same(R.projectile_angle(28.0, 9.8, 4.2, 0.2, 1), R.projectile_angle(28.0, 9.8, 4.2, 0.2, 0))
    tr = np.array([K.track(500 * K.MS, (12.0, -8.0, 1500.0))], abi.TRACK)       # the same shot through the step: 15 m, 6 m up, 10 m/s
    c0 = default_aim_config(mode=CLASSIC, v0=10.0, height=600.0)
    c1 = default_aim_config(mode=CLASSIC, v0=10.0, height=600.0, overloads=1)
    a0, a1 = Tracker.aim_host(c0, K.TICK, tr, K.NOW), Tracker.aim_host(c1, K.TICK, tr, K.NOW)
    assert a0.tobytes() == R.step(c0, K.TICK, tr, K.NOW)[0].tobytes() and a1.tobytes() == R.step(c1, K.TICK, tr, K.NOW)[0].tobytes()
    assert a0["status"] == 0 and a1["status"] == 0
    assert abs((a1["pitch"] - a0["pitch"]) - math.degrees(x_int - x_fabs)) < 1e-9 and a1["pitch"] < a0["pitch"] - 5.0


# ---------------------------------------------------------------------------------------------------------------- seeded sweep
def py_projectile_angle(v0, g, d, h):
    a = (g * (d * d)) / (2.0 * (v0 * v0))
    b = d
    c = a - h
    delta = (b * b) - (4 * a * c)
    if delta > 0:
        x1 = math.atan(((-1 * b) + math.sqrt(delta)) / (2 * a))
        x2 = math.atan(((-1 * b) - math.sqrt(delta)) / (2 * a))
        return x1 if abs(x1) < abs(x2) else x2
    if delta == 0:
        return math.atan((-1) * (b / 2 * a))
    return math.nan


def py_solve_gea(tv, g, v0, h, mode):
    d = tv[2] / 100.0
    y = math.atan2(tv[0] - 0.0, tv[2]) * 180.0 / math.pi
    if mode == NONE:
        return d / v0, -(math.atan2(tv[1] - 0.0, tv[2]) * 180.0 / math.pi), y
    normal = math.atan2(h / 100.0, d) * 180.0 / math.pi
    center = -math.atan2(tv[1] - 0.0, tv[2]) * 180.0 / math.pi
    target = py_projectile_angle(v0, g, d, h / 100.0) * 180.0 / math.pi
    p = (center - normal + 0.0 * 180.0 / math.pi) + target
    c = v0 * math.cos(target) if math.isfinite(target) else math.nan
    return d / abs(c), p, y


@pytest.fixture(scope="module")
def sweep():
    rng = np.random.default_rng(2024)
    n = 200000
    tv = np.stack([rng.uniform(-200, 200, n), rng.uniform(-200, 200, n), rng.uniform(50, 3000, n)], 1)
    return tv, rng.uniform(10, 30, n), rng.uniform(-100, 100, n)


def _lib_sweep(tv, v0, h, mode):
    L, out, gea = abi.lib(), np.zeros((len(tv), 3)), np.zeros(2)
    for k in range(len(tv)):
        gea[:] = np.nan
        out[k, 0] = L.rmcv_solve_gea(abi.ptr(tv[k]), 9.8, v0[k], h[k], 0.0, 0.0, 0.0, mode, abi.ptr(gea))
        out[k, 1:] = gea
    return out


def test_seeded_sweep(sweep):
    tv, v0, h = sweep
    worst = 0
    for mode in (NONE, CLASSIC):
        got = _lib_sweep(tv, v0, h, mode)
        ref, fragile = R.solve_n(tv, v0, h, 9.8, mode)
        assert got.tobytes() == ref.tobytes()                                             # the library against tests/aim_ref.c: bytes
        py = np.array([py_solve_gea(tv[k], 9.8, v0[k], h[k], mode) for k in range(len(tv))])   # ... and against Python's math
        assert fragile.mean() <= 1e-3
        keep = ~fragile
        d = ulps(got[keep], py[keep])
        worst = max(worst, int(d.max()))
        if mode == CLASSIC:
            assert 0.05 < np.isnan(got[:, 0]).mean() < 0.6                                # both outcomes are well represented
    print("\n[aim] seeded sweep, the library against Python's math: at most %d ulp" % worst)
    assert worst <= LIBM_ULPS_BOUND


# ---------------------------------------------------------------------------------------------------------------- the step
FRAME = (1280, 1024)


def scenario_positions(k, n_obs):
    """cm, in front of the camera, moving: velocities are non-zero"""
    rng = np.random.default_rng(7000 + k)
    return np.array([[-50.0 + 40.0 * i + 0.8 * k, 10.0 - 0.3 * k, 400.0 + 150.0 * i + 2.0 * k] for i in range(n_obs)]).reshape(n_obs, 3) + rng.normal(0, 0.3, (n_obs, 3))


@pytest.fixture(scope="module")
def scenario_lists():
    """the list every step of the seven tracker scenarios leaves (rmcv_tracker_step_host), with its timestamp"""
    out = []
    for name, (over, steps) in sorted(S.scenarios().items()):
        cfg = default_tracker_config(frame_w=FRAME[0], frame_h=FRAME[1], **dict(over, win_w=0, win_h=0))
        tr, side, st, org = np.zeros(0, abi.TRACK), np.zeros((0, 4, 2), np.float32), 0, (0, 0)
        for k, (arm, ids, pos, ts) in enumerate(steps):
            tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, arm, ids, scenario_positions(k, len(arm)), (0, 0), ts)
            out.append((name, k, tr, ts))
    assert len({n for n, _, _, _ in out}) == 7
    return out


def step_cases(scenario_lists, huge=False):
    """(label, tracks, now, aim input | None); huge: the seeded lists once more with the motor angle of K.aim_inputs_huge"""
    inputs = K.aim_inputs(3)
    for name, k, tr, ts in scenario_lists:
        yield "%s[%d]" % (name, k), tr, ts + (k % 3) * 4 * K.MS, (None if k % 2 else inputs[1 + k % 2:2 + k % 2])
    for name, tr in sorted(K.lists().items()):
        for i in (None, inputs[1:2], inputs[2:3]) + ((K.aim_inputs_huge(3)[1:2],) if huge else ()):
            yield name, tr, K.NOW, i


def test_step_host_equals_the_reference_byte_for_byte(scenario_lists):
    seen = {"target": 0, "none": 0, "nosol": 0, "nan": 0, "led": 0, "huge": 0}
    cfgs = K.configs()
    for label, tr, now, inp in step_cases(scenario_lists, huge=True):
        pair = None if inp is None else (inp[0]["world2camera"], float(inp[0]["motor_angle"]))
        for cname, cfg in cfgs.items():
            got = Tracker.aim_host(cfg, K.TICK, tr, now, pair)
            ref, _ = R.step(cfg, K.TICK, tr, now, inp)
            assert got.tobytes() == ref.tobytes(), (label, cname, got, ref)
            if pair is not None and pair[1] == K.HUGE_MOTOR_ANGLE and cfg.height_mode == abi.AIM_HEIGHT_DELTA and got["track"] >= 0:
                assert np.isnan(got["pitch"]), (label, cname, got)          # the tangent of 1e12 is NaN, not a number from an undefined conversion
                seen["huge"] += 1
            seen["none"] += got["status"] == abi.AIM_NO_TARGET
            seen["target"] += got["track"] >= 0
            seen["nosol"] += got["status"] == abi.AIM_NO_SOLUTION
            seen["nan"] += bool(np.isnan(got["point"]).any())
    assert all(seen[k] > 0 for k in ("target", "none", "nosol", "nan", "huge")), seen


def test_step_corners():
    L, cfgs = K.lists(), K.configs()
    aim = lambda c, tr, inp=None: Tracker.aim_host(cfgs[c] if isinstance(c, str) else c, K.TICK, tr, K.NOW, inp)
    none = aim("defaults", L["empty"])
    assert (none["track"], none["identity"], none["lost_count"], none["status"]) == (-1, -1, 0, abi.AIM_NO_TARGET)
    assert none.tobytes()[16:] == bytes(56)                                           # every double +0.0
    assert aim("mask_nothing", L["mixed7"]).tobytes() == none.tobytes() and aim("p0_s0_h0_l1", L["one_id7"]).tobytes() == none.tobytes()
    for n in (63, 64):                                                                # ties: the lowest index, under both rules
        assert aim("defaults", L["tie%d" % n])["track"] == 0 and aim("none_nearest", L["tie%d" % n])["track"] == 0
    assert aim("max_lost_0", L["tie64"])["track"] == 0 and aim("max_lost_0", L["tie64"][1:])["track"] == 2   # lost counts 1, 2, 0, ...
    assert aim("defaults", L["tie64_last_wins"])["track"] == 63 and aim("none_nearest", L["tie64_last_wins"])["track"] == 63
    m = aim("defaults", L["mixed7"])                                                  # the newest candidate: track 4 (track 5 is beyond max_lost)
    assert m["track"] == 4 and m["identity"] == 7 and m["lost_count"] == 1
    assert aim("p0_s0_h0_l1", L["mixed7"])["track"] == 1                              # 7 masked: the NaN state is next, and comes out NaN
    nan = aim("p0_s0_h0_l1", L["mixed7"])
    assert nan["status"] == abi.AIM_NO_SOLUTION and np.isnan(nan["pitch"]) and np.isnan(nan["point"]).all()
    assert aim("p1_s0_h0_l1", L["mixed7"])["track"] == 0                              # nearest: NaN counts as +infinity
    assert aim("mask_unknown_only", L["mixed7"])["track"] == 3                        # bit 31: identities -1 and 31; the newer is 31
    u = aim("p0_s1_h0_l4", L["mixed7"][2:3])                                          # uninitialised: position, no velocity, whatever the source
    assert u["point"].tolist() == [10.0, -5.0, 300.0]
    led, unled = aim("p0_s0_h0_l1", L["one"]), aim(default_aim_config(mode=CLASSIC, v0=28.0, height=20.0, offset_x=1.5, offset_y=-2.5, angle_offset=0.01,
                                                                          lead_iterations=0, identity_mask=K.NO_7), L["one"])
    dt = (K.NOW - 500 * K.MS) / K.TICK
    assert unled["point"].tolist() == [12.0 + 30.0 * dt, -8.0 + -4.0 * dt, 420.0 + 60.0 * dt]
    lead = dt + 0.012 + aim("p0_s0_h0_l0", L["one"])["flight_time"]
    assert led["point"].tolist() == [12.0 + 30.0 * lead, -8.0 + -4.0 * lead, 420.0 + 60.0 * lead]


REVERSED_SRC = r"""
#define AIM_HOST_REVERSED 1
#include "rmcv_amd/csrc/device_aim.h"
extern "C" void aim_reversed(const rmcv_aim_config* cfg, double tick, const rmcv_track* tracks, int n, const rmcv_aim_input* in, int64_t now, rmcv_aim* out)
{
    aim_stream(cfg, tick, tracks, n, in, now, out, 0);
}
"""


def test_the_pick_does_not_depend_on_the_order_of_the_lanes(tmp_path, scenario_lists):
    """on the device the lanes run at once and the pick is a butterfly: the shared source with the lanes in the OPPOSITE order gives the same bytes"""
    src, so = tmp_path / "rev.cpp", tmp_path / "rev.so"
    src.write_text(REVERSED_SRC)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", ROOT, str(src), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    L.aim_reversed.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.aim_reversed.restype = None
    inputs = K.aim_inputs(2)
    cases = [(tr, K.NOW) for tr in K.lists().values()] + [(tr, ts) for _, k, tr, ts in scenario_lists if k % 5 == 0]
    for tr, now in cases:
        for cfg in K.configs().values():
            out = np.zeros(1, abi.AIM)
            L.aim_reversed(C.byref(cfg), K.TICK, abi.ptr(tr) if len(tr) else None, len(tr), abi.ptr(inputs[1:2]), C.c_int64(int(now)), abi.ptr(out))
            assert out[0].tobytes() == Tracker.aim_host(cfg, K.TICK, tr, now, (inputs[1]["world2camera"], float(inputs[1]["motor_angle"]))).tobytes()


# ---------------------------------------------------------------------------------------------------------------- second opinion
def test_second_opinion_the_host_libm(sweep, scenario_lists):
    """tests/aim_ref.c on pinned_math.h against the same file on the host's libm: discrete fields equal, doubles within the measured bound"""
    tv, v0, h = sweep
    worst, left_out, total = 0, 0, 0
    for mode in (NONE, CLASSIC):
        a, fa = R.solve_n(tv, v0, h, 9.8, mode)
        b, fb = R.solve_n(tv, v0, h, 9.8, mode, libm=True)
        keep = ~(fa | fb)
        left_out, total = left_out + int((~keep).sum()), total + len(keep)
        worst = max(worst, int(ulps(a[keep], b[keep]).max()))
    for label, tr, now, inp in step_cases(scenario_lists):
        for cname, cfg in K.configs().items():
            a, fa = R.step(cfg, K.TICK, tr, now, inp)
            b, fb = R.step(cfg, K.TICK, tr, now, inp, libm=True)
            total += 1
            if fa or fb:
                left_out += 1
                continue
            for f in ("track", "identity", "lost_count", "status"):
                assert a[f] == b[f], (label, cname, f)
            for f in ("pitch", "yaw", "flight_time", "distance", "point"):
                worst = max(worst, int(ulps(a[f], b[f]).max()))
    print("\n[aim] pinned_math.h against the host libm: at most %d ulp over %d cases, %d left out (a comparison decided by a hair)" % (worst, total, left_out))
    assert left_out <= 1e-3 * total
    assert worst <= LIBM_ULPS_BOUND


# ---------------------------------------------------------------------------------------------------------------- the rest
def test_rigid_inverse():
    m = K.rigid()
    inv = rmcv_amd.rigid_inverse(m)
    exp = np.eye(4)
    exp[:3, :3] = m[:3, :3].T
    for i in range(3):   # each entry of R^T t summed left to right
        exp[i, 3] = -((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3])
    assert inv.tobytes() == exp.tobytes()
    assert np.abs(inv @ m - np.eye(4)).max() < 1e-14
    assert inv[3].tolist() == [0, 0, 0, 1]
    a = np.ascontiguousarray(m)                                    # in place
    assert abi.lib().rmcv_rigid_inverse(abi.ptr(a), abi.ptr(a)) == 0 and a.tobytes() == exp.tobytes()
    assert abi.lib().rmcv_rigid_inverse(None, abi.ptr(a)) == abi.ERR_BAD_ARG


def test_struct_sizes_and_defaults():
    assert abi.AIM.itemsize == 72 and abi.AIM_INPUT.itemsize == 136 and C.sizeof(AimConfig) == 80
    c = default_aim_config()
    assert (c.g, c.v0, c.height, c.offset_x, c.offset_y, c.angle_offset, c.latency_s) == (9.8, 15.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert (c.mode, c.height_mode, c.source, c.pick, c.lead_iterations, c.max_lost, c.overloads, c.identity_mask) == (NONE, 0, 0, 0, 1, 25, 0, 0xFFFFFFFF)


@pytest.mark.parametrize("bad", [dict(g=math.nan), dict(v0=math.inf), dict(height=-math.inf), dict(offset_x=math.nan), dict(offset_y=math.inf),
                                 dict(angle_offset=math.nan), dict(latency_s=math.inf), dict(mode=NI), dict(mode=3), dict(mode=-1), dict(height_mode=2),
                                 dict(source=-1), dict(pick=2), dict(lead_iterations=5), dict(lead_iterations=-1), dict(max_lost=-1)])
def test_refusals_that_need_no_device(bad):
    """what rmcv_tracker_set_aim refuses, through the entry point that checks the same config without a device"""
    tr = K.lists()["one"]
    with pytest.raises(abi.RmcvError) as e:
        Tracker.aim_host(default_aim_config(**bad), K.TICK, tr, K.NOW)
    assert e.value.code == abi.ERR_BAD_ARG


def test_refusals_of_the_step_itself():
    tr, out, cfg = K.lists()["tie64"], np.zeros(1, abi.AIM), default_aim_config()
    L = abi.lib()
    assert L.rmcv_aim_step_host(C.byref(cfg), K.TICK, abi.ptr(tr), 65, None, C.c_int64(0), abi.ptr(out)) == abi.ERR_BAD_ARG
    assert L.rmcv_aim_step_host(C.byref(cfg), 0.0, abi.ptr(tr), 64, None, C.c_int64(0), abi.ptr(out)) == abi.ERR_BAD_ARG
    assert L.rmcv_aim_step_host(None, K.TICK, abi.ptr(tr), 64, None, C.c_int64(0), abi.ptr(out)) == abi.ERR_BAD_ARG
    assert L.rmcv_tracker_set_aim(None, C.byref(cfg)) == abi.ERR_BAD_ARG and L.rmcv_tracker_aim(None, C.c_int64(0), None) == abi.ERR_BAD_ARG
