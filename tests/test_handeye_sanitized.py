"""rmcv_amd/csrc/device_handeye.h's host form under AddressSanitizer and UndefinedBehaviorSanitizer: tests/handeye_san_main.cpp, a stand-alone
program with its own main whose every table is a heap block of exactly its size, is compiled with -fsanitize=address,undefined and fed every
case of tests/handeye_cases.py and the fleet in one call (one of its cameras with too few views); what it writes equals tests/handeye_ref.py
byte for byte.  A CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np

import handeye_cases as HC
import handeye_ref as REF
from rmcv_amd.abi import HANDEYE_RESULT, HANDEYE_VIEW

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def sessions():
    """(views, attitudes, gripper_t, view_camera, n_cameras, min_w)"""
    out = [(c.views, c.attitudes, c.gripper_t, None, 1, dict(REF.DEFAULTS, **c.params)["min_w"]) for c in HC.CASES]
    fl = HC.FLEET
    return out + [(fl.views, fl.attitudes, None, fl.view_camera, fl.n_cameras, REF.DEFAULTS["min_w"])]


def restated(views, attitudes, gripper_t, view_camera, n_cameras, min_w):
    """the records the program writes, from the restatement -> (bytes, cameras with a rotation)"""
    res, rows, solved = np.zeros(n_cameras, HANDEYE_RESULT), np.zeros(len(views), HANDEYE_VIEW), 0
    for cam in range(n_cameras):
        r, world = REF.solve(views, attitudes, gripper_t, view_camera, n_cameras, cam, min_w)
        for k in r._fields:
            res[k][cam] = getattr(r, k)
        for v, w in world.items():
            rows["world"][v], rows["used"][v] = w, 1
        solved += isinstance(r, REF.Result)
    return res.tobytes() + rows.tobytes(), solved


def test_handeye_host_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "handeye_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "handeye_san_main.cpp"), "-o", exe], check=True)
    todo = sessions()
    blob, want, solved = [struct.pack("<i", len(todo))], [], 0
    for views, attitudes, gripper_t, view_camera, n_cameras, min_w in todo:
        blob.append(struct.pack("<4id", len(views), n_cameras, gripper_t is not None, view_camera is not None, min_w))
        blob.append(np.ascontiguousarray(views).tobytes() + np.ascontiguousarray(attitudes).tobytes())
        if gripper_t is not None:
            blob.append(np.ascontiguousarray(gripper_t, np.float64).tobytes())
        if view_camera is not None:
            blob.append(np.ascontiguousarray(view_camera, np.int32).tobytes())
        w, s = restated(views, attitudes, gripper_t, view_camera, n_cameras, min_w)
        want.append(w)
        solved += s
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["cases %d solved %d" % (len(todo), solved)] and solved == len(HC.CASES) - 2 + 2
    assert open(dst, "rb").read() == b"".join(want)
