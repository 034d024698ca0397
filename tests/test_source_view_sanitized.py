"""The host path of the source view (rmcv_amd/csrc/device_view.h: source_view_host) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/source_view_san_main.cpp, a stand-alone program with its own main, is compiled with -fsanitize=address,undefined and fed the CPU case
list of tests/view_cases.py over the frames of tests/source_view_cases.py at every size there, the rows padded by 5 bytes and the image
block ending with its last pixel; what it writes equals tests/source_view_ref.py byte for byte.  A CPU test: nothing here touches a GPU or
loads into python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import source_view_cases as SK
import source_view_ref as SR
import view_cases as K
from rmcv_amd.abi import POINT, VIEW_ALL

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
PAD = 5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("source_view_san") / "source_view_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "source_view_san_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("src,dst", SK.SIZES, ids=["%dx%d-%dx%d" % (s + d) for s, d in SK.SIZES])
def test_host_path_under_sanitizers_equals_the_reference(program, tmp_path, src, dst):
    w, h = src
    frame = SK.frame(w, h)
    stride = 3 * w + PAD
    padded = np.full((h, stride), 0xA5, np.uint8)
    padded[:, :3 * w] = frame.reshape(h, 3 * w)
    image = padded.tobytes()[:stride * (h - 1) + 3 * w]
    cases = K.cases(w, h)
    blob = struct.pack("<i", len(cases))
    want = b""
    for case in cases:
        neg = case["negatives"]
        offs = np.concatenate([[0], np.cumsum([len(c) for c in neg])]).astype(np.int32)
        pts = np.zeros(int(offs[-1]), POINT)
        if len(pts):
            allp = np.concatenate(neg)
            pts["x"], pts["y"] = allp[:, 0], allp[:, 1]
        blob += struct.pack("<10i", w, h, stride, len(case["blobs"]), len(neg), len(pts), len(case["armours"]), VIEW_ALL, dst[0], dst[1])
        blob += image + case["blobs"].tobytes() + offs.tobytes() + pts.tobytes() + case["armours"].tobytes()
        want += SR.view(frame, case["blobs"], neg, case["armours"], dst).tobytes()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, fin, fout], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert open(fout, "rb").read() == want
