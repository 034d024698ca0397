"""rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance of include/rmcv_shim.hpp: a caller that sees only the reference's declarations
(tests/shim_aim/aim_contract.hpp: include/mobility.h's signatures and default arguments) links against a backend unit that is the shim, and
gets what the ABI's host functions return.  Needs no GPU."""
import math
import os
import subprocess

import rmcv_amd
from rmcv_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS = ("shim_aim/backend_aim", "shim/core_stub", "shim_aim/caller_aim")
TVEC = (10.0, -5.0, 300.0)


def build(tmp):
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_aim"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_aim_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_shim_defines_the_aiming_functions_and_returns_what_the_abi_returns(tmp_path):
    objs, exe = build(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_aim/backend_aim"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_aim/caller_aim"]], check=True, capture_output=True, text=True).stdout
    for name in ("rm::ProjectileAngle(", "rm::SolveGEA(", "rm::DeltaHeight(", "rm::Distance("):
        assert name in defined and name in undefined, name
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {line.split()[0]: line.split()[1:] for line in out.splitlines()}
    val = float.fromhex

    def same(text, x):
        return (math.isnan(val(text)) and math.isnan(x)) or val(text).hex() == float(x).hex()

    assert same(rows["angle"][0], rmcv_amd.projectile_angle(15, 9.8, 3, 0.2))
    assert same(rows["distance"][0], rmcv_amd.distance(TVEC))
    assert same(rows["height_default"][0], rmcv_amd.delta_height(TVEC, 0.1))                        # offset {0, 0}, angleOffset 0
    assert same(rows["height_full"][0], rmcv_amd.delta_height(TVEC, 0.1, (1.5, -2.5), 0.01))
    t, gea = rmcv_amd.solve_gea(TVEC, 9.8, 28.0, 20.0)                                               # the defaults: COMPENSATE_NONE
    assert same(rows["gea_default"][0], t) and same(rows["gea_default"][1], gea[0]) and same(rows["gea_default"][2], gea[1])
    assert rows["gea_default"][3:] == ["rows", "2", "cols", "1", "type", "6"]                        # 2 x 1, CV_64F
    t, gea = rmcv_amd.solve_gea(TVEC, 9.8, 28.0, 20.0, (1.5, -2.5), 0.01, abi.COMPENSATE_CLASSIC)
    assert same(rows["gea_classic"][0], t) and same(rows["gea_classic"][1], gea[0]) and same(rows["gea_classic"][2], gea[1])
    assert math.isnan(val(rows["gea_ni"][0])) and rows["gea_ni"][1:] == ["created", "0"]             # NAN, the output never created
    assert all(math.isnan(val(v)) for v in rows["not_mat"][:3]) and rows["not_mat"][3:] == ["created", "0"]
