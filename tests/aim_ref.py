"""The reference of the aiming tests (TEST INFRASTRUCTURE): tests/aim_ref.c -- an independently written plain-C restatement of
src/mobility.cpp:36-82,127-164 and of the aim step of include/rmcv_abi.h -- built the way tests/track_ref.py builds its library (the oracle
Makefile's flags, into tests/_build/).  lib(): the transcendentals of pinned_math.h (the parity contract); lib(libm=True): the host libm's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from rmcv_amd import abi

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_SRC = os.path.join(_TESTS, "aim_ref.c")
_DEPS = [_SRC, os.path.join(_ROOT, "include", "rmcv_abi.h"), os.path.join(_ROOT, "rmcv_amd", "csrc", "pinned_math.h")]
# the oracle Makefile's flags for its scalar restatements
_FLAGS = ["-O2", "-std=c11", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fexcess-precision=standard", "-fno-tree-vectorize"]

AIM, AIM_INPUT, TRACK = abi.AIM, abi.AIM_INPUT, abi.TRACK


def build(libm=False):
    so = os.path.join(_TESTS, "_build", "libaim_ref_libm.so" if libm else "libaim_ref.so")
    if os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(s) for s in _DEPS):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(so))
    os.close(fd)
    try:
        subprocess.run(["cc"] + _FLAGS + (["-DAIM_REF_LIBM"] if libm else []) + ["-shared", "-o", tmp, _SRC, "-lm"], check=True)
        os.replace(tmp, so)  # (atomic: two test processes may build at once)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return so


_libs = {}


def lib(libm=False):
    if libm not in _libs:
        L = C.CDLL(build(libm))
        L.aim_ref_projectile_angle.restype = C.c_double
        L.aim_ref_projectile_angle.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]
        L.aim_ref_solve_gea.restype = C.c_double
        L.aim_ref_solve_gea.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float, C.c_double, C.c_int, C.c_int, C.c_void_p]
        L.aim_ref_delta_height.restype = C.c_double
        L.aim_ref_delta_height.argtypes = [C.c_void_p, C.c_double, C.c_float, C.c_double]
        L.aim_ref_distance.restype = C.c_double
        L.aim_ref_distance.argtypes = [C.c_void_p]
        L.aim_ref_solve_n.restype = None
        L.aim_ref_solve_n.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.aim_ref_step.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.aim_ref_fragile_reset.restype = None
        _libs[libm] = L
    return _libs[libm]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _t(tvec):
    return np.ascontiguousarray(tvec, np.float64).reshape(3)


def projectile_angle(v0, g, d, h, overloads=0, libm=False):
    return lib(libm).aim_ref_projectile_angle(v0, g, d, h, overloads)


def solve_gea(tvec, g, v0, h, offset=(0.0, 0.0), angle_offset=0.0, mode=0, overloads=0, libm=False, fill=np.nan):
    """(time, [pitch, yaw]); the output starts as `fill`, so an untouched one shows"""
    t, gea = _t(tvec), np.full(2, fill)
    time = lib(libm).aim_ref_solve_gea(_p(t), g, v0, h, offset[0], offset[1], angle_offset, mode, overloads, _p(gea))
    return time, gea


def delta_height(tvec, motor_angle, offset_y=0.0, angle_offset=0.0, libm=False):
    t = _t(tvec)
    return lib(libm).aim_ref_delta_height(_p(t), motor_angle, offset_y, angle_offset)


def distance(tvec, libm=False):
    t = _t(tvec)
    return lib(libm).aim_ref_distance(_p(t))


def solve_n(tvecs, v0, h, g, mode, overloads=0, libm=False):
    """(out (n, 3): time, pitch, yaw; fragile bool[n])"""
    tv, v0, h = np.ascontiguousarray(tvecs, np.float64).reshape(-1, 3), np.ascontiguousarray(v0, np.float64), np.ascontiguousarray(h, np.float64)
    out, frag = np.zeros((len(tv), 3)), np.zeros(len(tv), np.uint8)
    lib(libm).aim_ref_solve_n(len(tv), _p(tv), _p(v0), _p(h), g, mode, overloads, _p(out), _p(frag))
    return out, frag.astype(bool)


def step(config, tick_frequency, tracks, now, aim_input=None, libm=False):
    """one stream's aim step: config an rmcv_amd.AimConfig, tracks TRACK[n], aim_input a 1-element AIM_INPUT array | None
    -> (the AIM record, whether a comparison on the way was decided by a hair)"""
    tr = np.ascontiguousarray(tracks, TRACK)
    out = np.zeros(1, AIM)
    L = lib(libm)
    L.aim_ref_fragile_reset()
    rc = L.aim_ref_step(C.byref(config), tick_frequency, _p(tr) if len(tr) else None, len(tr), None if aim_input is None else _p(aim_input), C.c_int64(int(now)), _p(out))
    assert rc == 0
    return out[0], L.aim_ref_fragile() > 0
