"""rm::affine_correction on the shim (include/rmcv_shim.hpp): the link contract of tests/shim_icon/ -- a backend unit that
DEFINES it from the declaration of the reference's include/imgproc.h:17, a caller that saw the declaration only and makes the call of
executable/main.cpp:180 -- built like tests/shim_view/; and what the caller's program gets: the vertices clamped in place and the reference's
bytes, at 20 x 20 (the oracle's) and at the labeler's 80 x 80.  The function runs on the CPU: no GPU."""
import os
import struct
import subprocess

import numpy as np

import icon_cases as K
import icon_strip_cases as S
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS = ("shim_icon/backend_icon", "shim/core_stub", "shim_icon/caller_icon")
SIZES = ((20, 20), (80, 80), (33, 7))


def build_shim_icon(tmp):
    """compile the three units and link them against librmcv_hip.so -> (objects by unit, executable)"""
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_icon"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_icon_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_shim_defines_affine_correction_and_returns_the_reference_bytes(tmp_path):
    objs, exe = build_shim_icon(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_icon/backend_icon"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_icon/caller_icon"]], check=True, capture_output=True, text=True).stdout
    assert any("rm::affine_correction(cv::Mat const&, cv::Point2f*, cv::Size)" in ln and " T " in ln for ln in defined.splitlines())
    assert any("rm::affine_correction(" in ln for ln in undefined.splitlines())
    assert "rmcv_affine_correction_host" not in undefined                              # the caller reaches the C-ABI only through rm::
    plain = os.path.join(str(tmp_path), "backend_plain.o")                             # cv:: headers without cv::Size: the shim compiles, without it
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "cv_mock"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "shim"),
                    "-c", os.path.join(HERE, "shim", "backend.cpp"), "-o", plain], check=True)
    assert "affine_correction" not in subprocess.run(["nm", "-C", "--defined-only", plain], check=True, capture_output=True, text=True).stdout
    img = K.frame()
    blob, want, n = [struct.pack("<ii", S.W, S.H), img.tobytes()], [], 0
    records = []
    for ow, oh in SIZES:
        for (name, q), (out, clamped, _) in zip(S.list_for(ow, oh), S.expected(ow, oh)):
            records.append(np.asarray(q, np.float32).tobytes() + struct.pack("<ii", ow, oh))
            want.append(clamped.tobytes() + out.tobytes())
            if (ow, oh) == (20, 20):                                                    # main.cpp:180's size: the oracle's bytes
                ref, ric, _ = O.affine_correction(img, q)
                assert ric.tobytes() + ref.tobytes() == want[-1], name
            n += 1
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(blob + [struct.pack("<i", n)] + records))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert done.stdout.splitlines() == ["records %d refused 1" % n]
    assert open(dst, "rb").read() == b"".join(want)
