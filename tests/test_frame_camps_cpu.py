"""Per-frame detection keys, the host side (no GPU): rmcv_frame_key -- the function the device's prologue kernel runs, compiled for the
host -- against a restatement written here from the reference's text: the channel choice of rm::extract_color (src/imgproc.cpp:56-65) and
cv::inRange(gray, lb, 255) on a saturated u8 difference.  Then the key checked for what it MEANS: the image numpy computes from it equals
the CPU oracle's extract_binary with the raw camp and bound."""
import ctypes as C

import numpy as np
import pytest

import rmcv_amd
from rmcv_amd import MORPH_NONE, abi

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
CAMPS = (-7, -1, 0, 1, 2, 3, I32_MIN, I32_MAX)
BOUNDS = (I32_MIN, -1, 0, 1, 80, 255, 256, 257, I32_MAX)


def key_restated(camp, lb):
    """imgproc.cpp:56-65 in BGR byte order (split() gives B = 0, G = 1, R = 2): GUIDELIGHT (2) subtracts R from G, BLUE (1) R from B, every
    other value B from R.  inRange(gray, lb, 255) on gray = saturate(a - b) in 0 .. 255: lb <= 0 admits every pixel; lb > 255 none -- as a
    bound on a - b that is any value above 255, the key says 256; otherwise gray >= lb is a - b >= lb (lb >= 1: saturation at 0 changes
    nothing)."""
    a, b = (1, 2) if camp == 2 else (0, 2) if camp == 1 else (2, 0)
    if lb <= 0:
        return a, b, 1, 1
    return a, b, min(lb, 256), 0


def test_new_entry_points_are_exported():
    names = ("rmcv_frame_key", "rmcv_batch_set_frame_camps", "rmcv_batch_set_device_frame_camps", "rmcv_batch_get_frame_keys",
             "rmcv_pipeline_submit_camps", "rmcv_tracker_set_camps", "rmcv_tracker_device_camps")
    L = abi.lib()
    for n in names:
        assert n in abi.EXPORTS and hasattr(L, n), n
    assert L.rmcv_abi_version() == 1            # additive
    assert rmcv_amd.frame_key is abi.frame_key and rmcv_amd.Context.frame_key(1, 80) == abi.frame_key(1, 80)


@pytest.mark.parametrize("camp", CAMPS)
def test_frame_key_matches_the_restatement(camp):
    for lb in BOUNDS:
        assert abi.frame_key(camp, lb) == key_restated(camp, lb), (camp, lb)


def test_frame_key_checks_its_argument():
    assert abi.lib().rmcv_frame_key(C.c_int32(1), C.c_int32(80), None) == abi.ERR_BAD_ARG


def test_frame_key_means_what_the_oracle_computes(oracle):
    frame = np.random.default_rng(20261017).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    seen = set()
    for camp in CAMPS:
        for lb in BOUNDS:
            a, b, bound, all_pass = abi.frame_key(camp, lb)
            diff = frame[:, :, a].astype(np.int32) - frame[:, :, b].astype(np.int32)
            img = np.where((diff >= bound) | bool(all_pass), 255, 0).astype(np.uint8)
            ref = oracle.extract_binary(frame, camp, lb, MORPH_NONE)
            assert np.array_equal(img, ref), (camp, lb)
            seen.add(ref.tobytes())
    assert len(seen) >= 3 * 2 + 2               # three pairs at bounds 1 and 80, the all-set and the empty image: the cases differ


def test_context_entry_points_check_their_arguments_without_a_gpu():
    L = abi.lib()
    one = np.zeros(1, np.int32)
    assert L.rmcv_batch_set_frame_camps(None, abi.ptr(one), None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_set_device_frame_camps(None, abi.ptr(one), None) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_get_frame_keys(None, abi.ptr(np.zeros(4, np.int32)), 1) == abi.ERR_BAD_ARG
    assert L.rmcv_tracker_set_camps(None, abi.ptr(one), None) == abi.ERR_BAD_ARG
    assert L.rmcv_tracker_device_camps(None, None, None) == abi.ERR_BAD_ARG
    assert L.rmcv_pipeline_submit_camps(None, None, 1, 64, 64, 192, 192 * 64, None, None, None, 0, 0, None, abi.STAGE_ALL, None) == abi.ERR_BAD_ARG
