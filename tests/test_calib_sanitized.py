"""rmcv_amd/csrc/device_calib.h's host form under AddressSanitizer and UndefinedBehaviorSanitizer: tests/calib_san_main.cpp, a stand-alone program
with its own main whose every table and workspace is a heap block of exactly its size, is compiled with -fsanitize=address,undefined and fed
every case of tests/calib_cases.py (and the fleet's cameras, one of them with too few views); what it writes equals tests/calib_ref.py, rvec
apart, which is compared in ulps.  A CPU test: nothing here touches a GPU or loads into python."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import calib_cases as CC
import calib_ref as REF
from rmcv_amd.abi import CALIB_RESULT, CALIB_VIEW

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def sessions():
    out = [(c.corners, c.counts, c.cols, c.rows, c.square, c.params, c.guess) for c in CC.CASES]
    fl = CC.FLEET
    return out + [CC.alone(fl, cam)[:2] + (fl.cols, fl.rows, fl.square, {}, None) for cam in range(fl.n_cameras)]


def restated(corners, counts, cols, rows, square, params, guess):
    """the records the program writes, from the restatement; rvec zeroed (it is compared apart)"""
    res, views = np.zeros(1, CALIB_RESULT), np.zeros(len(corners), CALIB_VIEW)
    r, rv = REF.calibrate(corners, counts, cols, rows, square, CC.W, CC.H, guess=guess, **dict(REF.DEFAULTS, **params))
    if isinstance(r, REF.Result):
        for k in ("camera_matrix", "dist", "rms", "rms_init", "views_used", "iters", "status"):
            res[k][0] = getattr(r, k)
        for v, o in rv.items():
            views["tvec"][v], views["q"][v], views["rms"][v], views["used"][v] = o.tvec, o.q, o.rms, 1
    else:
        res["status"][0], res["views_used"][0] = r
    return res, views, {v: o.rvec for v, o in rv.items()}


def test_calib_host_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "calib_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "calib_san_main.cpp"), "-o", exe], check=True)
    todo = sessions()
    blob, want, rvecs, solved = [struct.pack("<i", len(todo))], [], [], 0
    for corners, counts, cols, rows, square, params, guess in todo:
        p = dict(REF.DEFAULTS, **params)
        corners = np.ascontiguousarray(corners, np.float32)
        blob.append(struct.pack("<9i2d", len(corners), corners.shape[1], cols, rows, CC.W, CC.H, p["max_iters"], p["fix_mask"], guess is not None, square, p["eps"]))
        if guess is not None:
            blob.append(np.concatenate([guess[0], guess[1]]).astype("<f8").tobytes())
        blob.append(corners.tobytes() + np.ascontiguousarray(counts, np.int32).tobytes())
        res, views, rv = restated(corners, counts, cols, rows, square, params, guess)
        want.append(res.tobytes() + views.tobytes())
        rvecs.append(rv)
        solved += int(res["status"][0]) & 7 != 0
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["cases %d solved %d" % (len(todo), solved)] and solved == len(todo) - 1
    got, at, plain = open(dst, "rb").read(), 0, []
    for (corners, *_), rv in zip(todo, rvecs):          # rvec out of the program's records: within 4 ulps of the restatement's, then zeroed
        n = len(corners)
        res = np.frombuffer(got, CALIB_RESULT, 1, at).copy()
        views = np.frombuffer(got, CALIB_VIEW, n, at + CALIB_RESULT.itemsize).copy()
        at += CALIB_RESULT.itemsize + n * CALIB_VIEW.itemsize
        for v, r in rv.items():
            a, b = views["rvec"][v].view(np.int64), np.array(r, np.float64).view(np.int64)
            assert np.all(np.sign(views["rvec"][v]) == np.sign(r)) and np.abs(a - b).max() <= 4, v
        views["rvec"] = 0.0
        plain.append(res.tobytes() + views.tobytes())
    assert at == len(got)
    assert hashlib.sha256(b"".join(plain)).hexdigest() == hashlib.sha256(b"".join(want)).hexdigest()
