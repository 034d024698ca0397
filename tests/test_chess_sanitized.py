"""rmcv_amd/csrc/device_chess.h's host form under AddressSanitizer and UndefinedBehaviorSanitizer: tests/chess_san_main.cpp, a stand-alone program
with its own main whose every image and table is a heap block of exactly its size (images with packed rows and with padded rows whose last one
ends with its pixels), is compiled with -fsanitize=address,undefined and fed every case of tests/chess_cases.py; what it writes equals
tests/chess_ref.py.  A CPU test: nothing here touches a GPU or loads into python."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import chess_cases as CC
import chess_ref as REF

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_chess_host_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "chess_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "chess_san_main.cpp"), "-o", exe], check=True)
    blob, want, boards = [struct.pack("<i", len(CC.CASES))], [], 0
    for c in CC.CASES:
        img = CC.IMAGES[c.image]
        h, w = img.shape[:2]
        p = dict(REF.DEFAULTS, **c.params)
        blob.append(struct.pack("<9i", w, h, c.cols, c.rows, p["threshold"], p["contrast"], p["nms"], p["dist_min"], p["dist_max"]) + img.tobytes())
        cor, st, cand = REF.find(img, c.cols, c.rows, **c.params)
        cor = np.full((c.cols * c.rows, 2), np.nan, np.float32) if cor is None else cor
        want += [struct.pack("<2i", st, len(cand)) + cand.tobytes() + cor.tobytes()] * 2
        boards += 2 * (st & REF.FOUND != 0)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["cases %d boards %d" % (len(CC.CASES), boards)]
    assert hashlib.sha256(open(dst, "rb").read()).hexdigest() == hashlib.sha256(b"".join(want)).hexdigest()
