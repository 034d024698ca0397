"""rm::utils::homogeneous and rm::lookup_CRC of include/rmcv_shim.hpp: a caller that sees only the reference's declarations
(tests/shim_attitude/attitude_contract.hpp: include/core.h:188 and hardware/include/serialport.h:49 with their default arguments) links
against a backend unit that is the shim, and gets what the ABI's host functions return.  Needs no GPU."""
import os
import subprocess

import numpy as np

import rmcv_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS = ("shim_attitude/backend_attitude", "shim/core_stub", "shim_attitude/caller_attitude")


def build(tmp):
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_attitude"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_attitude_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_shim_defines_homogeneous_and_lookup_crc_and_returns_what_the_abi_returns(tmp_path):
    objs, exe = build(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_attitude/backend_attitude"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_attitude/caller_attitude"]], check=True, capture_output=True, text=True).stdout
    for name in ("rm::utils::homogeneous(", "rm::lookup_CRC("):
        assert name in defined and name in undefined, name
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {line.split()[0]: line.split()[1:] for line in out.splitlines()}
    rotation = (0.125 * (np.arange(9) + 1) - 0.5).reshape(3, 3)
    translation = 10.5 * (np.arange(3) + 1)

    def matrix(row):
        assert row[:6] == ["rows", "4", "cols", "4", "type", "6"]                                     # 4 x 4, CV_64F
        return np.array([float.fromhex(v) for v in row[6:]]).reshape(4, 4)

    assert matrix(rows["default"]).tobytes() == rmcv_amd.homogeneous(rotation).tobytes()             # the default translation: zeros
    assert matrix(rows["full"]).tobytes() == rmcv_amd.homogeneous(rotation, translation).tobytes()
    assert rows["bad_rotation"][:4] == rows["bad_translation"][:4] == ["rows", "0", "cols", "0"]     # the reference's `return {}`
    buffer = bytes([0x38] + [(7 * i + 3) & 0xFF for i in range(1, 23)])
    assert int(rows["crc"][0]) == rmcv_amd.crc8(buffer)
    assert int(rows["crc_one"][0]) == 0xAC and int(rows["crc_none"][0]) == 0
