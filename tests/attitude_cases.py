"""The case list of the attitude tests (TEST INFRASTRUCTURE), shared by tests/test_attitude_cpu.py and tests/test_gpu_attitude.py: serial
packets of every kind the step tells apart, built here in Python (struct + a bit-by-bit CRC), cycled over any number of streams."""
import struct

import numpy as np

from rmcv_amd import CAMP_BLUE, CAMP_RED, abi

KINDS = ("valid_red", "valid_blue", "bad_header", "bad_payload", "bad_crc", "valid_upper_bits", "valid_nan", "valid_large", "valid_huge")
VALID = {"valid_red": CAMP_RED, "valid_blue": CAMP_BLUE, "valid_upper_bits": CAMP_BLUE, "valid_nan": CAMP_RED, "valid_large": CAMP_BLUE, "valid_huge": CAMP_RED}


def py_crc8(data):
    """polynomial 0x31, MSB first, init 0, no reflection, no final xor -- one bit at a time"""
    crc = 0
    for byte in bytes(data):
        for bit in range(7, -1, -1):
            top = (crc >> 7) & 1
            crc = (crc << 1) & 0xFF
            if top ^ ((byte >> bit) & 1):
                crc ^= 0x31
    return crc


def py_packet(byte1, yaw, pitch, roll, filler=0):
    """24 bytes: header, byte 1, yaw / pitch / roll as little-endian f32 at 3 / 11 / 15, `filler` elsewhere, the CRC"""
    b = bytearray([filler & 0xFF] * 24)
    b[0], b[1] = 0x38, byte1 & 0xFF
    b[3:7], b[11:15], b[15:19] = struct.pack("<f", yaw), struct.pack("<f", pitch), struct.pack("<f", roll)
    b[23] = py_crc8(b[:23])
    return bytes(b)


def packet(kind, rng):
    yaw, pitch, roll = (float(np.float32(rng.uniform(-180, 180))), float(np.float32(rng.uniform(-60, 60))), float(np.float32(rng.uniform(-30, 30))))
    filler = int(rng.integers(0, 256))
    if kind == "valid_red":
        return py_packet(1, yaw, pitch, roll, filler)
    if kind == "valid_blue":
        return py_packet(0, yaw, pitch, roll, filler)
    if kind == "valid_upper_bits":
        return py_packet(0xFE, yaw, pitch, roll, filler)           # bit 0 clear under seven set bits: still blue
    if kind == "valid_nan":
        return py_packet(0x81, yaw, float("nan"), roll, filler)    # a valid packet with a non-finite angle runs through
    if kind == "valid_large":
        return py_packet(0, 1e4, -1e4, 720.0, filler)
    if kind == "valid_huge":
        # radians beyond the range of pm_rem_pio2's quadrant number (an int): the sines and cosines are NaN on every build (pinned_math.h)
        return py_packet(1, 1e12, -1e12, 3.4028234663852886e38, filler)
    good = bytearray(py_packet(1, yaw, pitch, roll, filler))
    if kind == "bad_header":
        good[0] ^= 0x10
        good[23] = py_crc8(good[:23])                              # (the CRC is right: the header alone rejects it)
    elif kind == "bad_payload":
        good[int(rng.integers(1, 23))] ^= 1 << int(rng.integers(0, 8))
    elif kind == "bad_crc":
        good[23] ^= 1 << int(rng.integers(0, 8))
    else:
        raise KeyError(kind)
    return bytes(good)


def packets(n, seed, shift=0):
    """((n, 24) uint8, the kind of every stream): KINDS cycled over the streams, starting at `shift`"""
    rng = np.random.default_rng(seed)
    kinds = [KINDS[(f + shift) % len(KINDS)] for f in range(n)]
    return np.frombuffer(b"".join(packet(k, rng) for k in kinds), np.uint8).reshape(n, 24).copy(), kinds


def start_tables(n, seed):
    """what a tracker may hold when the step arrives: (attitudes ATTITUDE[n], camps int32[n], aim inputs AIM_INPUT[n])"""
    rng = np.random.default_rng(seed)
    att = np.zeros(n, abi.ATTITUDE)
    att["roll"], att["pitch"], att["yaw"] = rng.uniform(-0.5, 0.5, n), rng.uniform(-1, 1, n), rng.uniform(-3, 3, n)
    camps = rng.integers(0, 2, n).astype(np.int32)
    inp = np.zeros(n, abi.AIM_INPUT)
    inp["world2camera"] = rng.uniform(-2, 2, (n, 4, 4))
    inp["motor_angle"] = rng.uniform(-1, 1, n)
    return att, camps, inp


def gripper2camera(seed):
    """a rigid transform other than the default's: a rotation (the reference's own Euler product, in numpy) and a translation in cm"""
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(-1, 1, 3)
    rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    m = np.eye(4)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = rng.uniform(-80, 80, 3)
    return m
