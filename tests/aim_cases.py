"""Shared cases of the aiming tests (tests/test_aim_cpu.py, tests/test_gpu_aim.py): the configurations of the aim step, hand-made track
lists that reach its corners without pixels (ties, the NaN state, masked candidates, uninitialised tracks) and the aim inputs."""
import numpy as np

from rmcv_amd import abi
from rmcv_amd.tracker import default_aim_config

MS = 1_000_000  # ticks (tick_frequency 1e9)
TICK = 1e9
NO_7 = 0xFFFFFFFF & ~(1 << 7)   # every identity but 7


def configs():
    """name -> AimConfig: both pick rules x both sources x both height modes x lead_iterations 0, 1, 4 (CLASSIC, identity 7 masked out),
    then the single departures from the defaults"""
    out = {}
    for pick in (abi.AIM_PICK_WINDOW, abi.AIM_PICK_NEAREST):
        for source in (abi.AIM_SRC_FILTER, abi.AIM_SRC_MEASUREMENT):
            for hm in (abi.AIM_HEIGHT_FIXED, abi.AIM_HEIGHT_DELTA):
                for li in (0, 1, 4):
                    out["p%d_s%d_h%d_l%d" % (pick, source, hm, li)] = default_aim_config(
                        mode=abi.COMPENSATE_CLASSIC, v0=28.0, height=20.0, offset_x=1.5, offset_y=-2.5, angle_offset=0.01, latency_s=0.012, pick=pick,
                        source=source, height_mode=hm, lead_iterations=li, identity_mask=NO_7)
    out["defaults"] = default_aim_config()
    out["none_nearest"] = default_aim_config(pick=abi.AIM_PICK_NEAREST, latency_s=0.02, lead_iterations=2)
    out["classic_v15"] = default_aim_config(mode=abi.COMPENSATE_CLASSIC, height=20.0)   # long shots have no real root: RMCV_AIM_NO_SOLUTION
    out["max_lost_0"] = default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, max_lost=0)
    out["mask_nothing"] = default_aim_config(identity_mask=0)
    out["mask_unknown_only"] = default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, identity_mask=0x80000000)
    out["overloads"] = default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=10.0, height=600.0, overloads=1)   # slow and high: both roots below 1 rad
    return out


def track(ts, pos, vel=(0.0, 0.0, 0.0), identity=3, lost=0, initialized=1, meas=None):
    t = np.zeros(1, abi.TRACK)[0]
    t["timestamp"], t["identity"], t["lost_count"], t["initialized"] = ts, identity, lost, initialized
    t["position"] = pos
    t["state_post"] = tuple(pos) + tuple(vel)
    t["measurement"] = meas if meas is not None else (pos[0] + 0.5, pos[1] - 0.25, pos[2] + 1.0, vel[0] * 1.1, vel[1] * 0.9, vel[2] - 2.0)
    return t


def _pack(ts):
    return np.array(ts, abi.TRACK) if ts else np.zeros(0, abi.TRACK)


def lists():
    """name -> TRACK[n]"""
    T = 500 * MS
    out = {"empty": _pack([]), "one": _pack([track(T, (12.0, -8.0, 420.0), (30.0, -4.0, 60.0))]),
           "one_id7": _pack([track(T, (12.0, -8.0, 420.0), (30.0, -4.0, 60.0), identity=7)])}
    # equal timestamps and equal distances (sign flips of one point, no velocity): every rule ties, the lowest index wins
    signs = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
    for n in (63, 64):
        out["tie%d" % n] = _pack([track(T, (30.0 * signs[j % 4][0], 20.0 * signs[j % 4][1], 600.0), identity=j % 5, lost=j % 3) for j in range(n)])
    last = out["tie64"].copy()   # ... and the same list with the winner of both rules at index 63
    last[63] = track(T + MS, (3.0, 2.0, 300.0), (10.0, 0.0, -20.0), identity=2)
    out["tie64_last_wins"] = last
    nan = track(T + MS + MS // 2, (5.0, 5.0, 500.0), (1.0, 1.0, 1.0), identity=1)
    nan["state_post"] = np.nan    # what a matched update with dt = 0 leaves
    nan["measurement"][3:] = np.nan
    out["mixed7"] = _pack([
        track(T - 30 * MS, (-40.0, 20.0, 150.0), (-15.0, 2.0, 35.0), identity=2),
        nan,
        track(T, (10.0, -5.0, 300.0), (0.0, 0.0, 0.0), identity=-1, initialized=0),          # seen once: position, no velocity
        track(T + MS, (5.0, 5.0, 2500.0), (100.0, 0.0, -300.0), identity=31, lost=3),         # identity 31: the "any other" bit
        track(T + 2 * MS, (0.0, 0.0, 800.0), (20.0, 10.0, -50.0), identity=7, lost=1),        # masked out by NO_7
        track(T + 3 * MS, (60.0, -30.0, 900.0), (5.0, 5.0, 5.0), identity=4, lost=26),        # beyond max_lost
        track(T + MS, (-80.0, 15.0, 1200.0), (-60.0, 8.0, 120.0), identity=30, lost=25),
    ])
    out["five"] = out["mixed7"][[0, 2, 3, 4, 6]].copy()
    out["three"] = out["mixed7"][[1, 4, 5]].copy()
    return out


NOW = 510 * MS


def rigid(rx=0.05, ry=-0.1, t=(5.0, -3.0, 12.0)):
    cx, sx, cy, sy = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry)
    m = np.eye(4)
    m[:3, :3] = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m[:3, 3] = t
    return m


def aim_inputs(n):
    """AIM_INPUT[n]: stream 0 the defaults, the others a rigid world2camera built with rmcv_rigid_inverse and a motor angle"""
    a = np.zeros(n, abi.AIM_INPUT)
    for k in range(n):
        a[k]["world2camera"] = np.eye(4) if k == 0 else abi.rigid_inverse(rigid(0.05 * k, -0.1 + 0.03 * k, (5.0 * k, -3.0, 12.0 + k)))
        a[k]["motor_angle"] = 0.04 * k
    return a


HUGE_MOTOR_ANGLE = 1e12


def aim_inputs_huge(n):
    """aim_inputs(n) with a motor angle beyond the range of pm_rem_pio2's quadrant number (rmcv_aim_input.motor_angle is unchecked): under
    RMCV_AIM_HEIGHT_DELTA the tangent, and with it the height and the pitch, is NaN on every build"""
    a = aim_inputs(n)
    a["motor_angle"] = HUGE_MOTOR_ANGLE
    return a
