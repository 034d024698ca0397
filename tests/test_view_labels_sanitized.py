"""The host-side view-label functions (rmcv_amd/csrc/rmcv_labels.hip over device_text.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/labels_san_main.cpp, a stand-alone program with its own main, is compiled with -fsanitize=address,undefined
and fed the numbers and the blit cases of tests/label_cases.py at every scale, every buffer a heap block of exactly its size and every
string first asked for with a cap one short.  What it prints equals Python's "%f" and the library's own lines, what it writes equals
tests/label_ref.py byte for byte.  A CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np

import label_cases as K
import label_ref as LR
import rmcv_amd
from rmcv_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_host_functions_under_sanitizers(tmp_path):
    exe = str(tmp_path / "labels_san_main")
    subprocess.run(["g++"] + FLAGS + ["-x", "c++", os.path.join(HERE, "labels_san_main.cpp"), "-o", exe], check=True)
    numbers = K.F6_FIXED + K.f6_neighbours() + K.f6_ties() + K.f6_seeded(2000) + [v for v, _ in K.F6_PINNED]
    lines = ["%f" % v for v in numbers[:-len(K.F6_PINNED)]] + [t for _, t in K.F6_PINNED]
    for ch in range(256):
        if chr(ch) in abi.LABEL_CHARSET:
            lines.append(" ".join(str(int(v)) for v in [ch] + list(rmcv_amd.view_glyph(chr(ch)))))
    blob = struct.pack("<4i", K.VW, K.VH, K.W, K.H) + struct.pack("<i", len(numbers)) + np.array(numbers, np.float64).tobytes()
    cases = K.cases()
    blob += struct.pack("<i", len(cases) * len(K.SCALES))
    want = b""
    for case in cases:
        at, tt = LR.texts_of(case)
        for scale in K.SCALES:
            n = len(case["armours"])
            ids, pos = case["identities"], case["positions"]
            blob += struct.pack("<8i", case["stride"], scale, n, ids is not None, pos is not None, len(case["tracks"]), *case["origin"])
            blob += K.background(case["stride"]).tobytes() + case["armours"].tobytes()
            blob += (ids.tobytes() if ids is not None else b"") + (pos.tobytes() if pos is not None else b"")
            blob += case["tracks"].tobytes() + case["side"].tobytes()
            lines += at + tt
            want += LR.expected(case, scale)[0].tobytes()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == lines
    assert open(fout, "rb").read() == want
