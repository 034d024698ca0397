"""rmcv_amd/csrc/icon_host.h under AddressSanitizer and UndefinedBehaviorSanitizer: tests/icon_strip_san_main.cpp, a stand-alone program with
its own main whose every image, list and output is a heap block of exactly its size (images with packed rows and with padded rows whose last
one ends with its pixels), is compiled with -fsanitize=address,undefined and fed tests/icon_strip_cases.py at every side and both rectangular
sizes, strips with fewer, as many and more slots than armours, and sheets; what it writes equals the numpy restatements.  A CPU test: nothing
here touches a GPU or loads into python."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import icon_cases as K
import icon_strip_cases as S
import view_cases as VK
from rmcv_amd.abi import ICON_STRIP_CAP_MAX, VIEW_ALL, VIEW_ARMOURS

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SIZES = [(s, s) for s in S.SIDES] + list(S.RECT_SIZES)
STRIPS = [(9, 7, 4), (9, 20, 9), (3, 33, 5), (0, 20, 2), (2, 80, 2), (1, 1, 3)]             # (armours, side, cap)
SHEETS = [(5, 50, 34, 33, VIEW_ALL), (2, 100, 68, 20, VIEW_ARMOURS), (0, 40, 30, 80, 0), (6, 160, 120, 128, VIEW_ALL)]  # (armours, vw, vh, side, flags)


def sheet_armours(n):
    return VK.armours(*[VK.armour(K.box(5 + k, 5, 30 + k, 30), K.box(10 + 9 * k, 8 + 5 * k, 60 + 9 * k, 50 + 5 * k)) for k in range(n)])


def test_icon_host_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "icon_strip_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "icon_strip_san_main.cpp"), "-o", exe], check=True)
    img, binary = K.frame(), VK.binary(S.W, S.H)
    blob = [struct.pack("<ii", S.W, S.H), img.tobytes(), binary.tobytes()]
    want = []
    n_icons = sum(len(S.list_for(*size)) for size in SIZES)
    blob.append(struct.pack("<i", n_icons))
    degenerate = 0
    for ow, oh in SIZES:
        for (_, q), (out, clamped, deg) in zip(S.list_for(ow, oh), S.expected(ow, oh)):
            blob.append(np.asarray(q, np.float32).tobytes() + struct.pack("<ii", ow, oh))
            want.append(clamped.tobytes() + struct.pack("<i", deg) + out.tobytes())
            degenerate += deg
    icons = [q for _, q in S.cases(20)[:9]]
    blob.append(struct.pack("<i", len(STRIPS)))
    for n, side, cap in STRIPS:
        blob.append(struct.pack("<iii", n, side, cap) + b"".join(np.asarray(q, np.float32).tobytes() for q in icons[:n]))
        want.append(S.strip_ref(img, icons[:n], side, cap).tobytes())
    blob.append(struct.pack("<i", len(SHEETS)))
    for n, vw, vh, side, flags in SHEETS:
        arm = sheet_armours(n)
        blob.append(struct.pack("<iiiii", n, vw, vh, side, flags) + b"".join(a["vertices"].tobytes() + a["icon"].tobytes() for a in arm))
        want.append(S.sheet_ref(img, binary, VK.blobs(), [], arm, (vw, vh), side, flags, ICON_STRIP_CAP_MAX).tobytes())
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["icons %d degenerate %d strips %d sheets %d" % (n_icons, degenerate, len(STRIPS), len(SHEETS))]
    assert hashlib.sha256(open(dst, "rb").read()).hexdigest() == hashlib.sha256(b"".join(want)).hexdigest()
