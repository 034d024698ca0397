"""The reference of the attitude tests (TEST INFRASTRUCTURE): tests/attitude_ref.c -- an independently written plain-C restatement of
include/core.h:66-84, src/core.cpp:406-416, hardware/src/serialport.cpp:9-18, executable/main.cpp:120-143 and of the attitude step of
include/rmcv_abi.h -- built the way tests/aim_ref.py builds its library (gcc -O2 -ffp-contract=off, into tests/_build/).  It shares only
pinned_math.h's pm_sin / pm_cos with the library."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from rmcv_amd import abi

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_SRC = os.path.join(_TESTS, "attitude_ref.c")
_DEPS = [_SRC, os.path.join(_ROOT, "include", "rmcv_abi.h"), os.path.join(_ROOT, "rmcv_amd", "csrc", "pinned_math.h")]
_FLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fexcess-precision=standard", "-fno-tree-vectorize"]

ATTITUDE, AIM_INPUT = abi.ATTITUDE, abi.AIM_INPUT


def build():
    so = os.path.join(_TESTS, "_build", "libattitude_ref.so")
    if os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(s) for s in _DEPS):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(so))
    os.close(fd)
    try:
        subprocess.run(["gcc"] + _FLAGS + ["-shared", "-o", tmp, _SRC, "-lm"], check=True)
        os.replace(tmp, so)  # (atomic: two test processes may build at once)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.att_ref_to_matrix.restype = None
        L.att_ref_to_matrix.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
        L.att_ref_homogeneous.restype = None
        L.att_ref_homogeneous.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.att_ref_crc.restype = C.c_uint8
        L.att_ref_crc.argtypes = [C.c_void_p, C.c_int]
        L.att_ref_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.att_ref_step.restype = None
        L.att_ref_step.argtypes = [C.c_void_p] * 7
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def to_matrix(roll, pitch, yaw):
    out = np.zeros((3, 3))
    lib().att_ref_to_matrix(float(roll), float(pitch), float(yaw), _p(out))
    return out


def homogeneous(rotation, translation=None):
    r, out = np.ascontiguousarray(rotation, np.float64).reshape(3, 3), np.zeros((4, 4))
    t = None if translation is None else np.ascontiguousarray(translation, np.float64).reshape(3)
    lib().att_ref_homogeneous(_p(r), _p(t), _p(out))
    return out


def crc(data):
    b = np.frombuffer(bytes(data), np.uint8)
    return int(lib().att_ref_crc(_p(b) if len(b) else None, len(b)))


def decode(packet):
    """(camp, (roll, pitch, yaw) float64[3]) | None"""
    b = np.frombuffer(bytes(packet), np.uint8)
    assert len(b) == 24
    camp, xyz = C.c_int32(0), np.zeros(3)
    return (camp.value, xyz) if lib().att_ref_decode(_p(b), C.byref(camp), _p(xyz)) else None


def step(config, packet, attitude, camp, packet_errors, aim_input, base2gripper=True):
    """one stream: config an rmcv_amd.AttitudeConfig, packet 24 bytes | None, attitude a 1-element ATTITUDE array, camp an int | None,
    aim_input a 1-element AIM_INPUT array -> (ATTITUDE record, camp | None, packet_errors, base2gripper (4, 4) | None, AIM_INPUT record);
    nothing handed in is changed"""
    a = np.ascontiguousarray(attitude, ATTITUDE).reshape(1).copy()
    inp = np.ascontiguousarray(aim_input, AIM_INPUT).reshape(1).copy()
    pk = None if packet is None else np.frombuffer(bytes(packet), np.uint8)
    cm, err = C.c_int32(0 if camp is None else int(camp)), C.c_int32(int(packet_errors))
    b = np.zeros((4, 4)) if base2gripper else None
    lib().att_ref_step(C.cast(C.byref(config), C.c_void_p), _p(pk), _p(a), None if camp is None else C.cast(C.byref(cm), C.c_void_p),
                       C.cast(C.byref(err), C.c_void_p), _p(b), _p(inp))
    return a[0], (None if camp is None else cm.value), err.value, b, inp[0]


def tables(config, packets, attitudes, camps, errors, inputs, base2gripper=True):
    """the step over n streams: packets (n, 24) uint8 | None, attitudes ATTITUDE[n], camps int32[n] | None, errors int32[n], inputs
    AIM_INPUT[n] -> new (attitudes, camps | None, errors, base2gripper (n, 4, 4) | None, inputs)"""
    n = len(attitudes)
    att, err, inp = attitudes.copy(), errors.copy(), inputs.copy()
    cm = None if camps is None else camps.copy()
    b2g = np.zeros((n, 4, 4)) if base2gripper else None
    for f in range(n):
        a, c, e, b, i = step(config, None if packets is None else packets[f].tobytes(), att[f:f + 1], None if cm is None else cm[f], err[f], inp[f:f + 1],
                             base2gripper)
        att[f], err[f], inp[f] = a, e, i
        if cm is not None:
            cm[f] = c
        if b2g is not None:
            b2g[f] = b
    return att, cm, err, b2g, inp
