"""Windowed detection, the parts that need no GPU: rm::utils::GetROI (rmcv_get_roi) against the independent restatement of
tests/window_ref.py and against hand-computed cases, rmcv_window_origin, rmcv_armours_to_frame, and the argument checks of the new
batch and pipeline entry points on a host without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import window_ref as R

from rmcv_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM_UNITS = ("shim_window/backend_window", "shim/core_stub", "shim_window/caller_window")


def build_shim_window(tmp):
    """compile the three units of the tracked-ROI link test and link them against librmcv_hip.so -> (objects by unit, executable)"""
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in SHIM_UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_window"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_window_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_new_entry_points_are_exported():
    L = abi.lib()
    for name in ("rmcv_batch_set_windows", "rmcv_batch_set_device_windows", "rmcv_batch_get_windows", "rmcv_batch_device_windows",
                 "rmcv_pipeline_submit_windows", "rmcv_get_roi", "rmcv_window_origin", "rmcv_armours_to_frame"):
        assert name in abi.EXPORTS and hasattr(L, name), name


def test_get_roi_matches_the_restatement_on_random_inputs():
    rng = np.random.default_rng(20261017)
    n_cases = 4000
    for i in range(n_cases):
        n = int(rng.integers(1, 9))
        fw, fh = int(rng.integers(16, 2049)), int(rng.integers(16, 1537))
        if i % 7 == 0:    # points well outside the frame, negative included
            pts = rng.uniform(-600.0, 2600.0, size=(n, 2)).astype(np.float32)
        else:             # a cluster somewhere around the frame
            c = rng.uniform(-40.0, [fw + 40.0, fh + 40.0])
            pts = (c + rng.uniform(-120.0, 120.0, size=(n, 2))).astype(np.float32)
        if i % 5 == 0:    # whole-number coordinates: floor() on exact integers, +1 on widths
            pts = np.rint(pts).astype(np.float32)
        kind = i % 4
        scale = (1.0, 1.0) if kind == 0 else (float(np.float32(rng.uniform(0.2, 4.0))),) * 2 if kind == 1 else \
            (float(np.float32(rng.uniform(0.2, 4.0))), float(np.float32(rng.uniform(0.2, 4.0))))
        if i % 11 == 0:
            scale = (1.0, 2.5)                                            # only one of the two differs from 1: the branch is taken
        prev = (0, 0, 0, 0) if i % 3 == 0 else tuple(int(v) for v in rng.integers(-200, 1200, size=4))
        fs = (-1, -1) if i % 97 == 0 else (fw, fh)                        # the reference's default frame size
        got = abi.get_roi(pts, scale, fs, prev)
        want = R.get_roi(pts, scale, fs, prev)
        assert got == want, (i, pts.tolist(), scale, fs, prev, got, want)
    # the scalar overload of include/core.h:143 is the pair (s, s)
    pts = np.array([[100, 200], [139, 259]], np.float32)
    assert abi.get_roi(pts, 2.0, (1280, 1024)) == abi.get_roi(pts, (2.0, 2.0), (1280, 1024)) == R.get_roi(pts, (2.0, 2.0), (1280, 1024))


def test_get_roi_hand_computed_cases():
    f = (1280, 1024)
    # scale 1 leaves the bounding rect as it is: floor(10.5) = 10, floor(30.7) - 10 + 1 = 21; floor(20.2) = 20, floor(40.9) - 20 + 1 = 21
    assert abi.get_roi([[10.5, 20.2], [30.7, 40.9]], 1.0, f) == (10, 20, 21, 21)
    # ... plus previous.x / .y (a rect found inside an earlier ROI)
    assert abi.get_roi([[10.5, 20.2], [30.7, 40.9]], 1.0, f, (100, 50, 7, 9)) == (110, 70, 21, 21)
    # scale (2, 3) on the 40 x 60 rect at (100, 200): margins (int)(40 * 2 / 2) = 40 and (int)(60 * 3 / 2) = 90; x = 60, y = 110, w = 40 + 80 = 120
    # and h = 60 + 2 * 40 = 140 -- the WIDTH's margin, as the reference writes it (a "fixed" version would give 60 + 180 = 240)
    assert abi.get_roi([[100, 200], [139, 259]], (2.0, 3.0), f) == (60, 110, 120, 140)
    # truncation of the margin: w = 21, scale 1.5 -> (int)(15.75) = 15
    assert abi.get_roi([[10.5, 20.2], [30.7, 40.9]], (1.5, 1.5), f, (100, 100, 0, 0)) == (110 - 15, 120 - 15, 21 + 30, 21 + 30)
    # crossing the left edge: x = 5 - 40 < 0 -> 0, the size stays what the margins made it
    assert abi.get_roi([[5, 300], [44, 339]], 2.0, f) == (0, 260, 120, 120)
    # crossing the top edge
    assert abi.get_roi([[300, 5], [339, 44]], 2.0, f) == (260, 0, 120, 120)
    # touching the right edge: x + w = 1250 + 30 = 1280 >= 1280 -> w = 1280 - 1250 - 1 = 29
    assert abi.get_roi([[1250, 300], [1279, 329]], 1.0, f) == (1250, 300, 29, 30)
    # one short of it: x + w = 1279 < 1280 -> untouched
    assert abi.get_roi([[1249, 300], [1278, 329]], 1.0, f) == (1249, 300, 30, 30)
    # touching the bottom edge: y + h = 1000 + 24 = 1024 >= 1024 -> h = 1024 - 1000 - 1 = 23
    assert abi.get_roi([[100, 1000], [129, 1023]], 1.0, f) == (100, 1000, 30, 23)
    # a rect beyond the frame: w = 1280 - 2000 - 1 < 0 -> {0, 0, 0, 0}
    assert abi.get_roi([[2000, 2000], [2010, 2010]], 1.0, f) == (0, 0, 0, 0)
    # the default frame size {-1, -1}: every size comes out negative -> {0, 0, 0, 0}
    assert abi.get_roi([[10, 10], [20, 20]]) == (0, 0, 0, 0)
    # no points: the empty rect at `previous`, then the edge rules
    assert abi.get_roi(np.zeros((0, 2), np.float32), 1.0, f, (30, 40, 0, 0)) == (30, 40, 0, 0)


def test_window_origin_and_effective_origin_rule():
    assert abi.window_origin((60, 110, 120, 140), 512, 384) == (60 + 60 - 256, 110 + 70 - 192) == (-136, -12)
    assert abi.window_origin((600, 500, 41, 33), 512, 384) == (600 + 20 - 256, 500 + 16 - 192)
    assert abi.window_origin((0, 0, 0, 0), 1, 1) == (0, 0)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        rect = tuple(int(v) for v in rng.integers(0, 2000, size=4))
        ww, wh = int(rng.integers(1, 1921)), int(rng.integers(1, 1201))
        assert abi.window_origin(rect, ww, wh) == R.window_origin(rect, ww, wh)
    # the restatement of the effective-origin rule, on hand-computed cases (the GPU tests compare the device's table with it)
    assert R.effective_origin(-136, -12, 1280, 1024, 512, 384) == (0, 0)
    assert R.effective_origin(389, 300, 1280, 1024, 512, 384) == (384, 300)      # 389 & ~15
    assert R.effective_origin(5000, 5000, 1280, 1024, 512, 384) == (768, 640)    # 1280 - 512 = 768 is a multiple of 16
    assert R.effective_origin(5000, 0, 1280, 1024, 200, 150) == (1072, 0)        # 1080 & ~15
    assert R.effective_origin(7, 9, 1280, 1024, 1280, 1024) == (0, 0)            # window == frame
    L = abi.lib()
    out = (C.c_int32 * 2)()
    rect = (C.c_int32 * 4)(1, 2, 3, 4)
    assert L.rmcv_window_origin(None, 8, 8, out) == abi.ERR_BAD_ARG and L.rmcv_window_origin(rect, 8, 8, None) == abi.ERR_BAD_ARG
    assert L.rmcv_window_origin(rect, 0, 8, out) == abi.ERR_BAD_ARG and L.rmcv_window_origin(rect, 8, -1, out) == abi.ERR_BAD_ARG


def test_armours_to_frame_is_one_f32_add_per_coordinate():
    rng = np.random.default_rng(9)
    a = np.zeros(5, abi.ARMOUR)
    a["icon"] = rng.uniform(-30, 600, size=(5, 4, 2)).astype(np.float32)
    a["vertices"] = rng.uniform(-30, 600, size=(5, 4, 2)).astype(np.float32)
    a["bbox"] = rng.uniform(0, 600, size=(5, 4)).astype(np.float32)
    a["blob_i"], a["blob_j"] = np.arange(5), np.arange(5) + 1
    x, y = 16777217, -333                                     # (float)16777217 = 16777216: the offset is converted first, as mobility.cpp:172 does
    b = abi.armours_to_frame(a, x, y)
    off = np.array([np.float32(x), np.float32(y)], np.float32)
    assert off[0] == np.float32(16777216.0)
    assert np.array_equal(b["icon"], a["icon"] + off) and np.array_equal(b["vertices"], a["vertices"] + off)
    assert np.array_equal(b["bbox"][:, :2], a["bbox"][:, :2] + off) and np.array_equal(b["bbox"][:, 2:], a["bbox"][:, 2:])
    assert np.array_equal(b["blob_i"], a["blob_i"]) and np.array_equal(b["blob_j"], a["blob_j"])
    assert len(abi.armours_to_frame(np.zeros(0, abi.ARMOUR), 3, 4)) == 0
    L = abi.lib()
    assert L.rmcv_armours_to_frame(None, 1, 0, 0) == abi.ERR_BAD_ARG and L.rmcv_armours_to_frame(None, -1, 0, 0) == abi.ERR_BAD_ARG
    assert L.rmcv_armours_to_frame(None, 0, 0, 0) == abi.OK


def test_window_entry_points_check_their_arguments_without_a_gpu():
    import torch
    L = abi.lib()
    pt = (C.c_int32 * 2)(0, 0)
    w, h = C.c_int32(-1), C.c_int32(-1)
    assert L.rmcv_batch_set_windows(None, pt, 64, 32) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_set_windows(None, None, 0, 0) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_set_device_windows(None, pt, 64, 32) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_get_windows(None, pt, 1, C.byref(w), C.byref(h)) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_device_windows(None, None, None, None) == abi.ERR_BAD_ARG
    t = C.c_uint64(7)
    p = abi.default_params()
    assert L.rmcv_pipeline_submit_windows(None, pt, 1, 64, 64, 192, 192 * 64, pt, 64, 32, C.addressof(p), 15, C.addressof(t)) == abi.ERR_BAD_ARG
    assert t.value == 7
    out = (C.c_int32 * 4)()
    pts = (C.c_float * 4)(1, 2, 3, 4)
    assert L.rmcv_get_roi(pts, 2, 1.0, 1.0, 100, 100, None, None) == abi.ERR_BAD_ARG        # no output
    assert L.rmcv_get_roi(None, 2, 1.0, 1.0, 100, 100, None, out) == abi.ERR_BAD_ARG        # points missing
    assert L.rmcv_get_roi(pts, -1, 1.0, 1.0, 100, 100, None, out) == abi.ERR_BAD_ARG
    assert L.rmcv_get_roi(pts, 2, 1.0, 1.0, 100, 100, None, out) == abi.OK and list(out) == [1, 2, 3, 3]   # previous == NULL: zeros
    if not torch.cuda.is_available():
        from rmcv_amd import Context, RmcvError
        with pytest.raises(RmcvError) as e:
            Context(device=0, max_frames=2)
        assert e.value.code == abi.ERR_NO_DEVICE                                               # windows have no CPU path either


def test_shim_defines_get_roi(tmp_path):
    """the backend object (declarations of include/core.h:142-147 + the shim) DEFINES both overloads of rm::utils::GetROI next to the
    functions it defined before; a caller that saw declarations only links against it.  Where the cv:: headers have no cv::Size
    (tests/cv_mock alone) the shim still compiles, without them."""
    objs, exe = build_shim_window(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_window/backend_window"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_window/caller_window"]], check=True, capture_output=True, text=True).stdout
    roi = [ln for ln in defined.splitlines() if "rm::utils::GetROI(" in ln and " T " in ln]
    assert len(roi) == 2 and any("float, cv::Size const&" in ln for ln in roi) and any("cv::Size2f const&, cv::Size const&" in ln for ln in roi), roi
    for sym in ("rm::extract_color(", "rm::filter_armours(", "rm::solve_PnP("):
        assert any(sym in ln and " T " in ln for ln in defined.splitlines()), sym
    for sym in ("rm::utils::GetROI(", "rm::extract_color(", "rm::solve_PnP("):
        assert any(sym in ln for ln in undefined.splitlines()), sym
    assert "rmcv_get_roi" not in undefined and os.path.exists(exe)      # the caller reaches the helper only through rm::
    plain = os.path.join(str(tmp_path), "backend_plain.o")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "cv_mock"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "shim"),
                    "-c", os.path.join(HERE, "shim", "backend.cpp"), "-o", plain], check=True)
    assert "GetROI" not in subprocess.run(["nm", "-C", "--defined-only", plain], check=True, capture_output=True, text=True).stdout
