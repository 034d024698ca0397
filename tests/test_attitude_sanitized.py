"""The host path of rmcv_amd/csrc/device_attitude.h under AddressSanitizer and UndefinedBehaviorSanitizer: tests/attitude_san_main.cpp, a
stand-alone program with its own main, is compiled with -fsanitize=address,undefined and fed the CPU case list -- the 130-stream tables
included -- and what it writes equals tests/attitude_ref.c byte for byte.  A CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import attitude_cases as K
import attitude_ref as R
from rmcv_amd import abi, default_attitude_config

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attitude_san") / "attitude_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "attitude_san_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("n", [1, 5, 64, 65, 130])
def test_host_path_under_sanitizers_equals_the_reference(program, tmp_path, n):
    rounds = [K.packets(n, 51)[0], K.packets(n, 52, shift=3)[0], None, K.packets(n, 53, shift=5)[0]]
    for camps_on, pose, mode in ((0, 1, abi.ATT_MOTOR_KEEP), (1, 1, abi.ATT_MOTOR_PITCH), (1, 0, abi.ATT_MOTOR_KEEP)):
        cfg = default_attitude_config(motor_angle_mode=mode, gripper2camera=K.gripper2camera(54))
        att, camps, inp = K.start_tables(n, 55)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<4i", n, len(rounds), camps_on, pose) + bytes(cfg) + att.tobytes() + camps.tobytes() + inp.tobytes())
            for pk in rounds:
                f.write(struct.pack("<i", 0 if pk is None else 1) + (b"" if pk is None else pk.tobytes()))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        done = subprocess.run([program, src, dst], capture_output=True, text=True, env=env)
        assert done.returncode == 0, done.stderr
        got = open(dst, "rb").read()
        err, at = np.zeros(n, np.int32), 0
        for pk in rounds:
            att, new_camps, err, b2g, inp = R.tables(cfg, pk, att, camps if camps_on else None, err, inp, base2gripper=bool(pose))
            if camps_on:
                camps = new_camps
            want = att.tobytes() + camps.tobytes() + err.tobytes() + (b2g.tobytes() if pose else b"") + inp.tobytes()
            assert got[at:at + len(want)] == want
            at += len(want)
        assert at == len(got) and err.sum() > 0
