"""rm::debug::device_view, the shim's one addition for the operator's view (include/rmcv_shim.hpp): the link contract of
tests/shim_view/ -- a backend unit that DEFINES it from a declaration with a default argument, a caller that saw the declaration only --
built like tests/shim_window/, and, on the GPU, what the caller's program gets against the library's own view of the same batch."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS = ("shim_view/backend_view", "shim/core_stub", "shim_view/caller_view")


def build_shim_view(tmp):
    """compile the three units and link them against librmcv_hip.so -> (objects by unit, executable)"""
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_view"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_view_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_shim_defines_device_view(tmp_path):
    objs, exe = build_shim_view(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_view/backend_view"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_view/caller_view"]], check=True, capture_output=True, text=True).stdout
    assert any("rm::debug::device_view(rmcv_ctx*, int, cv::Size const&)" in ln and " T " in ln for ln in defined.splitlines())
    assert not any("rm::debug::draw_" in ln for ln in defined.splitlines())      # draw_lightblobs / draw_armours stay the reference's own
    assert any("rm::debug::device_view(" in ln for ln in undefined.splitlines())
    assert "rmcv_batch_get_debug_view" not in undefined and os.path.exists(exe)   # the caller reaches the view only through rm::
    plain = os.path.join(str(tmp_path), "backend_plain.o")                          # cv:: headers without cv::Size: the shim compiles, without it
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "cv_mock"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "shim"),
                    "-c", os.path.join(HERE, "shim", "backend.cpp"), "-o", plain], check=True)
    assert "device_view" not in subprocess.run(["nm", "-C", "--defined-only", plain], check=True, capture_output=True, text=True).stdout


def fnv(a):
    h = 1469598103934665603
    for b in a.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.gpu
def test_shim_device_view_equals_the_library(tmp_path):
    from rmcv_amd import CAMP_BLUE, STAGE_ALL, Context, default_params, synth
    _, exe = build_shim_view(str(tmp_path))
    w, h, vw, vh = 200, 136, 160, 102
    out = subprocess.run([exe, str(w), str(h), str(vw), str(vh)], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    c = Context(device=0, max_frames=4)
    try:
        c.upload(np.stack([synth.frame(3 + f, w, h, CAMP_BLUE, 0) for f in range(4)]))
        c.run(default_params(tilt_max=10.0), STAGE_ALL)
        large, view = c.debug_view(1, (1024, 768)), c.debug_view(1, (vw, vh))
    finally:
        c.close()
    assert view.any() and (view != view[0, 0]).any()
    assert out[:4] == ["default", "1024", "768", "%016x" % fnv(large)]
    assert out[4:8] == ["view", str(vw), str(vh), "%016x" % fnv(view)]
    assert out[8:] == ["refused", "2"]
