"""T(r), the oriented 8-bit mosaic a delivered sensor buffer r is read as (include/rmcv_abi.h: RMCV_OPT_INPUT_SAMPLE_BITS /
_VALID_BIT / _ORIENT), the pattern derived for it, and the way back, restated in plain numpy for the tests.  No product code.

  n(s)        = s for 1-byte samples, (s >> valid_bit) & 0xFF for 2-byte samples (the bits above the window are dropped)
  T(r)(x, y)  = n(r(mirror ? w-1-x : x, flip ? h-1-y : y))
  pattern     the caller names that of r as delivered; T(r)'s R site has column parity (w-1-rx) & 1 under mirror, row parity
              (h-1-ry) & 1 under flip
"""
import numpy as np

import bayer_ref as BR

ORIENTATIONS = [(False, False), (True, False), (False, True), (True, True)]  # (mirror, flip)


def narrow(r, valid_bit=0):
    """n of every sample: uint8 as it is, uint16 -> bits valid_bit .. valid_bit + 7"""
    r = np.asarray(r)
    if r.dtype == np.uint8:
        return r
    assert r.dtype.itemsize == 2 and 0 <= valid_bit <= 4
    return ((r.astype(np.uint32) >> valid_bit) & 0xFF).astype(np.uint8)


def orient_bgr(bgr, mirror, flip):
    """mirror (left-right) and / or flip (top-bottom) BGR frames [..., h, w, 3]; its own inverse"""
    return np.ascontiguousarray(_orient_axes(np.asarray(bgr), mirror, flip, -2))


def _orient_axes(a, mirror, flip, ax_w):
    if mirror:
        a = np.flip(a, ax_w)
    if flip:
        a = np.flip(a, ax_w - 1)
    return a


def T(r, valid_bit=0, mirror=False, flip=False):
    """the oriented 8-bit mosaic of one delivered buffer (h, w) or a stack (n, h, w)"""
    return np.ascontiguousarray(_orient_axes(narrow(r, valid_bit), mirror, flip, -1))


def derived_pattern(pattern, w, h, mirror=False, flip=False):
    """the pattern of T(r) for a buffer of pattern `pattern` as delivered"""
    rx, ry = BR.r_site(pattern)
    if mirror:
        rx = (w - 1 - rx) & 1
    if flip:
        ry = (h - 1 - ry) & 1
    return {(0, 0): BR.RG, (0, 1): BR.GB, (1, 0): BR.GR, (1, 1): BR.BG}[(rx, ry)]


def delivered_pattern(oriented_pattern, w, h, mirror=False, flip=False):
    """the pattern a sensor reports for the buffer whose T has `oriented_pattern` (the derivation is its own inverse)"""
    return derived_pattern(oriented_pattern, w, h, mirror, flip)


def delivered(mosaic, sample_bits=8, valid_bit=0, mirror=False, flip=False, rng=None):
    """a delivered buffer r with T(r) = mosaic ([..., h, w] uint8): oriented back, and with 16-bit samples the pixel at bits
    valid_bit .. valid_bit + 7 with random bits below and above the window"""
    m = _orient_axes(np.asarray(mosaic, np.uint8), mirror, flip, -1)
    if sample_bits == 8:
        return np.ascontiguousarray(m)
    assert sample_bits == 16 and 0 <= valid_bit <= 4
    rng = rng or np.random.default_rng(1)
    keep = np.uint16(0xFF << valid_bit)
    noise = rng.integers(0, 1 << 16, m.shape, dtype=np.uint16) & np.uint16(~keep & 0xFFFF)
    return np.ascontiguousarray((m.astype(np.uint16) << np.uint16(valid_bit)) | noise)
