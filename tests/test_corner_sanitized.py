"""rmcv_amd/csrc/device_corner.h's host form under AddressSanitizer and UndefinedBehaviorSanitizer: tests/corner_san_main.cpp, a stand-alone
program with its own main whose every image and table is a heap block of exactly its size (images with packed rows and with padded rows whose
last one ends with its pixels), is compiled with -fsanitize=address,undefined and fed every case of tests/corner_cases.py; what it writes equals
restatement (a) of tests/corner_ref.py.  A CPU test: nothing here touches a GPU or loads into python."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import corner_cases as CC
import corner_ref as REF

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_corner_host_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "corner_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "corner_san_main.cpp"), "-o", exe], check=True)
    blob, want, corners = [struct.pack("<i", len(CC.CASES))], [], 0
    for c in CC.CASES:
        img = CC.IMAGES[c.image]
        h, w = img.shape[:2]
        blob.append(struct.pack("<8id", w, h, len(c.corners), c.win[0], c.win[1], c.zero[0], c.zero[1], c.max_iters, c.eps) + img.tobytes() + c.corners.tobytes())
        ref, st = REF.subpix(img, c.corners, c.win, c.zero, c.max_iters, c.eps, pinned=True)
        want += [ref.tobytes() + st.tobytes()] * 2 + [REF.mask(c.win[0], c.win[1], c.zero).tobytes(), REF.gray(img).tobytes()]
        corners += 2 * len(c.corners)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["cases %d corners %d" % (len(CC.CASES), corners)]
    assert hashlib.sha256(open(dst, "rb").read()).hexdigest() == hashlib.sha256(b"".join(want)).hexdigest()
