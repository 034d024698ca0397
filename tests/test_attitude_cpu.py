"""The per-stream gimbal attitude on the CPU (no device): rmcv_crc8, rmcv_serial_encode / _decode, rmcv_euler_to_matrix, rmcv_homogeneous and
rmcv_attitude_step_host -- the source k_attitude is compiled from -- against tests/attitude_ref.c, byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest

import aim_cases as AK
import attitude_cases as K
import attitude_ref as R
import rmcv_amd
from rmcv_amd import CAMP_BLUE, CAMP_RED, AttitudeConfig, RmcvError, Tracker, abi, default_attitude_config, default_pnp_config

PI = 3.141592653589793


# ---------------------------------------------------------------- crc8
def test_crc8_known_values_and_empty():
    assert [rmcv_amd.crc8(bytes([b])) for b in (1, 2, 3, 4, 8, 255)] == [0x31, 0x62, 0x53, 0xC4, 0xB9, 0xAC]
    assert rmcv_amd.crc8(b"") == 0
    assert abi.lib().rmcv_crc8(None, 5) == 0


def test_crc8_equals_a_bitwise_crc_on_random_strings():
    rng = np.random.default_rng(31)
    for _ in range(1000):
        s = rng.integers(0, 256, 23, dtype=np.uint8).tobytes()
        assert rmcv_amd.crc8(s) == K.py_crc8(s) == R.crc(s)


# ---------------------------------------------------------------- serial_encode / serial_decode
def test_encode_decode_round_trip_and_rejections():
    for camp in (CAMP_RED, CAMP_BLUE):
        p = rmcv_amd.serial_encode(camp, 12.5, -3.25, 0.75)
        assert p == K.py_packet(1 if camp == CAMP_RED else 0, 12.5, -3.25, 0.75)
        got_camp, att = rmcv_amd.serial_decode(p)
        assert got_camp == camp
        assert (att["yaw"], att["pitch"], att["roll"]) == (12.5 * PI / 180.0, -3.25 * PI / 180.0, 0.75 * PI / 180.0)
        for at in (0, 5, 23):                                               # a flipped header, payload and CRC byte
            bad = bytearray(p)
            bad[at] ^= 0x04
            assert rmcv_amd.serial_decode(bytes(bad)) is None and R.decode(bytes(bad)) is None
    with pytest.raises(RmcvError):
        rmcv_amd.serial_encode(abi.CAMP_NEUTRAL, 0, 0, 0)
    assert rmcv_amd.serial_decode(K.py_packet(0xFE, 1, 2, 3))[0] == CAMP_BLUE   # byte 1: bit 0 only
    assert rmcv_amd.serial_decode(K.py_packet(0xFF, 1, 2, 3))[0] == CAMP_RED


def test_decode_radians_equal_the_reference_bytes():
    rng = np.random.default_rng(32)
    vals = np.concatenate([rng.uniform(-720, 720, 600), rng.standard_normal(200) * 1e-3, [0.0, -0.0, 180.0, 90.0, 1e30, math.inf, math.nan]]).astype(np.float32)
    for k in range(0, len(vals) - 2):
        yaw, pitch, roll = (float(v) for v in vals[k:k + 3])
        p = K.py_packet(k & 1, yaw, pitch, roll)
        camp, att = rmcv_amd.serial_decode(p)
        rcamp, xyz = R.decode(p)
        assert camp == rcamp == (CAMP_RED if k & 1 else CAMP_BLUE)
        assert np.array([att["roll"], att["pitch"], att["yaw"]]).tobytes() == xyz.tobytes()


# ---------------------------------------------------------------- euler_to_matrix / homogeneous
SPECIAL = [0.0, -0.0, math.pi / 2, -math.pi / 2, math.pi, 1e4 * math.pi / 180, 2.0 ** -30, math.nan]


def angle_triples():
    rng = np.random.default_rng(33)
    out = [(a, b, c) for a in SPECIAL for b in SPECIAL for c in SPECIAL]
    out += [tuple(t) for t in rng.uniform(-4, 4, (2000, 3))]
    return out


def test_euler_to_matrix_and_homogeneous_equal_the_reference_bytes():
    rng = np.random.default_rng(34)
    for roll, pitch, yaw in angle_triples():
        got, want = rmcv_amd.euler_to_matrix((roll, pitch, yaw)), R.to_matrix(roll, pitch, yaw)
        assert got.tobytes() == want.tobytes(), (roll, pitch, yaw, got, want)
        if all(math.isfinite(v) for v in (roll, pitch, yaw)):
            # three rounded products of unit-size terms: a bound on the arithmetic, not a parity claim
            assert np.abs(got @ got.T - np.eye(3)).max() < 1e-14
        else:
            assert np.isnan(got).any()
        t = rng.uniform(-100, 100, 3)
        for tr in (None, t):
            h = rmcv_amd.homogeneous(got, tr)
            assert h.tobytes() == R.homogeneous(want, tr).tobytes()
            assert h[3].tolist() == [0, 0, 0, 1] and h[:3, 3].tolist() == ([0, 0, 0] if tr is None else t.tolist())


def test_angles_beyond_the_quadrant_number_come_out_nan():
    """a CRC-valid packet may carry any float: from 1.93e11 degrees on the pinned sine and cosine are NaN (pinned_math.h, the conversion's
    edge), on every build -- not the 7e121 an undefined conversion to int gave on x86"""
    for deg in (1e12, -1e12, 3.4028234663852886e38, -3.4028234663852886e38):
        _, att = rmcv_amd.serial_decode(K.py_packet(1, deg, 0.25, -0.5))
        assert att["yaw"] == float(np.float32(deg)) * PI / 180.0 and math.isfinite(att["yaw"])
        got = rmcv_amd.euler_to_matrix(att)
        assert got.tobytes() == R.to_matrix(att["roll"], att["pitch"], att["yaw"]).tobytes()
        assert np.isnan(got[:2]).all() and not np.isnan(got[2]).any()             # rows 0 and 1 carry cos / sin of the yaw, row 2 does not
    below = 3.3e9                                                                   # ... and just below the edge both are numbers in [-1, 1]
    m = rmcv_amd.euler_to_matrix((0.0, 0.0, below))
    assert np.isfinite(m).all() and np.abs(m).max() <= 1.0 and m.tobytes() == R.to_matrix(0.0, 0.0, below).tobytes()


def test_signed_zeros_are_a_general_product_s():
    m = rmcv_amd.euler_to_matrix((0.0, 0.0, 0.0))
    assert m.tobytes() == R.to_matrix(0.0, 0.0, 0.0).tobytes() == np.eye(3).tobytes()      # every zero +0: (x * 0 + -0 * 1) + ... sums to +0
    assert rmcv_amd.euler_to_matrix((-0.0, -0.0, -0.0)).tobytes() == R.to_matrix(-0.0, -0.0, -0.0).tobytes()


# ---------------------------------------------------------------- the step
def configs():
    out = []
    for mode in (abi.ATT_MOTOR_KEEP, abi.ATT_MOTOR_PITCH):
        out.append(default_attitude_config(motor_angle_mode=mode))
        out.append(default_attitude_config(motor_angle_mode=mode, gripper2camera=K.gripper2camera(35)))
    return out


def test_default_config():
    c = default_attitude_config()
    assert C.sizeof(AttitudeConfig) == 136 and abi.ATTITUDE.itemsize == 24
    assert list(c.gripper2camera) == list(default_pnp_config().gripper2camera) and c.motor_angle_mode == abi.ATT_MOTOR_KEEP and c.reserved == 0


def test_step_host_equals_the_reference_every_case():
    n = 130
    for cfg in configs():
        for camps_on in (False, True):
            att, camps, inp = K.start_tables(n, 36)
            err = np.zeros(n, np.int32)
            for rnd, pk in enumerate((K.packets(n, 37)[0], K.packets(n, 38, shift=3)[0], None)):
                want = R.tables(cfg, pk, att, camps if camps_on else None, err, inp)
                for f in range(n):
                    a, c, e, b, i = Tracker.attitude_host(cfg, None if pk is None else pk[f].tobytes(), att[f:f + 1], int(camps[f]) if camps_on else None,
                                                          int(err[f]), inp[f:f + 1])
                    assert a.tobytes() == want[0][f].tobytes() and e == want[2][f] and b.tobytes() == want[3][f].tobytes(), (rnd, f)
                    assert i.tobytes() == want[4][f].tobytes(), (rnd, f, i, want[4][f])
                    assert c == (int(want[1][f]) if camps_on else None)
                att, err, inp = want[0], want[2], want[4]
                if camps_on:
                    camps = want[1]
            kinds = [K.packets(n, 37)[1], K.packets(n, 38, shift=3)[1]]
            rejected = np.array([sum(not k[f].startswith("valid") for k in kinds) for f in range(n)])
            assert err.tolist() == rejected.tolist() and 0 < rejected.sum() < 2 * n      # packet_errors counts the rejections
            if cfg.motor_angle_mode == abi.ATT_MOTOR_PITCH:
                assert inp["motor_angle"].tobytes() == att["pitch"].tobytes()
            else:
                assert inp["motor_angle"].tobytes() == K.start_tables(n, 36)[2]["motor_angle"].tobytes()
            assert np.isnan(inp["world2camera"]).any() and np.isfinite(inp["world2camera"]).any()   # the NaN angle ran through; the others are finite


def test_step_host_is_what_the_host_functions_say():
    # (a gripper2camera orthonormal to double precision: the default's entries are float literals, whose transpose is an inverse to 6e-8 only)
    cfg = default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH, gripper2camera=K.gripper2camera(35))
    p = rmcv_amd.serial_encode(CAMP_RED, 30.0, -10.0, 5.0)
    a, camp, err, b, inp = Tracker.attitude_host(cfg, p, (0.0, 0.0, 0.0), CAMP_BLUE)
    assert camp == CAMP_RED and err == 0 and a.tobytes() == rmcv_amd.serial_decode(p)[1].tobytes()
    B = rmcv_amd.homogeneous(rmcv_amd.euler_to_matrix(a))
    assert b.tobytes() == B.tobytes()
    G = np.array(cfg.gripper2camera).reshape(4, 4)
    assert np.abs(inp["world2camera"] @ (B @ G) - np.eye(4)).max() < 1e-12 and inp["motor_angle"] == a["pitch"]
    a2, camp2, err2, b2, inp2 = Tracker.attitude_host(cfg, None, a, CAMP_RED, 0, inp.reshape(1))          # no packet: the table as it stands
    assert (a2.tobytes(), camp2, err2, b2.tobytes(), inp2.tobytes()) == (a.tobytes(), CAMP_RED, 0, b.tobytes(), inp.tobytes())
    _, _, _, none, _ = Tracker.attitude_host(cfg, p, (0.0, 0.0, 0.0), base2gripper=False)                  # no pose tables
    assert none is None


def test_first_ever_rejected_packet_leaves_zero_attitude_and_initial_camp():
    cfg = default_attitude_config()
    bad = bytearray(rmcv_amd.serial_encode(CAMP_RED, 30.0, -10.0, 5.0))
    bad[0] = 0x39
    a, camp, err, b, inp = Tracker.attitude_host(cfg, bytes(bad), (0.0, 0.0, 0.0), CAMP_BLUE)
    assert a.tobytes() == bytes(24) and camp == CAMP_BLUE and err == 1
    assert b.tobytes() == np.eye(4).tobytes()
    assert inp["world2camera"].tobytes() == rmcv_amd.rigid_inverse(np.array(cfg.gripper2camera).reshape(4, 4)).tobytes()   # today's loop_inputs


def test_rigid_inverse_unchanged():
    m = AK.rigid()                                                          # the inputs of tests/test_aim_cpu.py::test_rigid_inverse
    exp = np.eye(4)
    exp[:3, :3] = m[:3, :3].T
    for i in range(3):
        exp[i, 3] = -((m[0, i] * m[0, 3] + m[1, i] * m[1, 3]) + m[2, i] * m[2, 3])
    assert rmcv_amd.rigid_inverse(m).tobytes() == exp.tobytes()
    g = np.array(default_pnp_config().gripper2camera).reshape(4, 4)
    junk = g.copy()
    junk[3] = [5, 6, 7, 8]                                                  # row 3 of the input is not read
    assert rmcv_amd.rigid_inverse(junk).tobytes() == rmcv_amd.rigid_inverse(g).tobytes()


def test_bad_arguments():
    L = abi.lib()
    a, r9, h16, p24 = np.zeros(1, abi.ATTITUDE), np.zeros(9), np.zeros(16), np.zeros(24, np.uint8)
    camp, err, inp = C.c_int32(0), C.c_int32(0), np.zeros(1, abi.AIM_INPUT)
    cfg = default_attitude_config()
    B = abi.ERR_BAD_ARG
    assert L.rmcv_euler_to_matrix(None, abi.ptr(r9)) == B and L.rmcv_euler_to_matrix(abi.ptr(a), None) == B
    assert L.rmcv_homogeneous(None, None, abi.ptr(h16)) == B and L.rmcv_homogeneous(abi.ptr(r9), None, None) == B
    assert L.rmcv_serial_decode(None, C.byref(camp), abi.ptr(a)) == B and L.rmcv_serial_decode(abi.ptr(p24), None, abi.ptr(a)) == B
    assert L.rmcv_serial_decode(abi.ptr(p24), C.byref(camp), None) == B
    assert L.rmcv_serial_encode(CAMP_RED, 0.0, 0.0, 0.0, None) == B and L.rmcv_serial_encode(7, 0.0, 0.0, 0.0, abi.ptr(p24)) == B
    args = [C.byref(cfg), None, abi.ptr(a), None, C.byref(err), None, abi.ptr(inp)]
    assert L.rmcv_attitude_step_host(*args) == 0
    for k in (0, 2, 4, 6):
        bad = list(args)
        bad[k] = None
        assert L.rmcv_attitude_step_host(*bad) == B
    for broken in (default_attitude_config(motor_angle_mode=2), default_attitude_config(motor_angle_mode=-1),
                   default_attitude_config(gripper2camera=np.full(16, math.nan)), default_attitude_config(gripper2camera=[math.inf] + [0.0] * 15)):
        assert L.rmcv_attitude_step_host(C.byref(broken), None, abi.ptr(a), None, C.byref(err), None, abi.ptr(inp)) == B
