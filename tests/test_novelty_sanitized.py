"""The host path of rmcv_amd/csrc/device_novelty.h under AddressSanitizer and UndefinedBehaviorSanitizer: tests/novelty_san_main.cpp, a
stand-alone program with its own main whose every table is a heap block of exactly its size, is compiled with -fsanitize=address,undefined
and fed every append of tests/novelty_cases.py with the state tests/novelty_ref.py says it meets; what it writes equals the restatement.  A
CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np

import novelty_cases as K
import novelty_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def calls():
    """(n_streams, R, T, rows, n_rows, labels, state before, state after, keep, min_sad) of every append of every case"""
    out = []
    for c in K.cases():
        e = K.expected(c)
        before = R.State(c.cap, c.R)
        for (rows, n, lb, _), keep, dist, after in zip(c.appends, e["keeps"], e["sads"], e["states"]):
            out.append((len(n), c.R, c.T, rows, n, lb, before, after, keep, dist))
            before = after
    return out


def test_host_rule_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "novelty_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "novelty_san_main.cpp"), "-o", exe], check=True)
    cs = calls()
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(cs)))
        for s, depth, T, rows, n, lb, before, _, _, _ in cs:
            f.write(struct.pack("<4i", s, depth, T, len(rows)))
            f.write(n.astype("<i4").tobytes() + lb.astype("<i4").tobytes() + rows.tobytes())
            f.write(before.rings[:s].tobytes() + before.pushed[:s].astype("<i8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    got = open(dst, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        v = np.frombuffer(got, dtype, count, at)
        at += v.nbytes
        return v

    for s, depth, T, rows, n, lb, before, after, keep, dist in cs:
        total = len(rows)
        assert np.array_equal(take(np.uint8, total).astype(bool), keep)
        assert np.array_equal(take("<i4", total).astype(np.int64), dist)
        assert int(take("<i8", 1)[0]) == after.near - before.near
        assert np.array_equal(take(np.uint8, s * depth * R.ROW).reshape(s, depth, R.ROW), after.rings[:s])
        assert np.array_equal(take("<i8", s), after.pushed[:s])
        assert int(take("<i4", 1)[0]) == (R.sad(rows[0], rows[1]) if total >= 2 else -1)
    assert at == len(got)
