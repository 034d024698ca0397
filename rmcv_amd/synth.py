"""Synthetic camera stream: deterministic, integer-only frames from csrc/synth.c."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .abi import CAMP_BLUE, lib, ptr


def frame(index, w=1280, h=1024, camp=CAMP_BLUE, variant=0, out=None):
    """one BGR uint8 frame [h, w, 3]; seed = 20241008 + index"""
    if out is None:
        out = np.empty((h, w, 3), np.uint8)
    rc = lib().rmcv_synth_frame(ptr(out), w, h, 3 * w, C.c_uint64(int(index)), int(camp), int(variant))
    if rc != 0:
        raise ValueError("rmcv_synth_frame failed: %d" % rc)
    return out


def batch(first, n, w=1280, h=1024, camp=CAMP_BLUE, variant=0, threads=8):
    """frames first .. first+n-1 as uint8 [n, h, w, 3] (ctypes releases the GIL, so threads scale)"""
    out = np.empty((n, h, w, 3), np.uint8)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(lambda i: frame(first + i, w, h, camp, variant, out[i]), range(n)))
    return out


def mosaic(bgr, pattern):
    """the colour filter array of `pattern` (abi.BAYER_RG .. BAYER_BG: the top-left 2x2 block) sampled from synthetic BGR frames
    [..., h, w, 3] -> raw 8-bit mosaics [..., h, w]: each pixel keeps the one channel its filter passes"""
    from .abi import BAYER_BG, BAYER_GB, BAYER_GR, BAYER_RG
    if pattern not in (BAYER_RG, BAYER_GB, BAYER_GR, BAYER_BG):
        raise ValueError("unknown Bayer pattern %r" % (pattern,))
    bgr = np.asarray(bgr, np.uint8)
    rx = 1 if pattern in (BAYER_GR, BAYER_BG) else 0  # the R site of the 2x2 block
    ry = 1 if pattern in (BAYER_GB, BAYER_BG) else 0
    h, w = bgr.shape[-3], bgr.shape[-2]
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    px, py = (x ^ rx) & 1, (y ^ ry) & 1
    ch = np.where((px == 0) & (py == 0), 2, np.where((px == 1) & (py == 1), 0, 1))  # R site, B site, else G (BGR channel index)
    return np.take_along_axis(bgr, np.broadcast_to(ch[..., None], bgr.shape[:-1] + (1,)), axis=-1)[..., 0].copy()


def raw_frame(mosaic, sample_bits=8, valid_bit=0, mirror=False, flip=False, rng=None):
    """a buffer as a sensor delivers it whose oriented 8-bit reading is `mosaic` [..., h, w] (include/rmcv_abi.h: T(r) = mosaic): the
    pixels mirrored / flipped back into the sensor's order and, with 16-bit samples, placed at bits valid_bit .. valid_bit + 7 of
    little-endian uint16 samples whose bits below AND above that window hold random data (a reader has to drop both)"""
    m = np.asarray(mosaic, np.uint8)
    if mirror:
        m = m[..., ::-1]
    if flip:
        m = m[..., ::-1, :]
    if sample_bits == 8:
        return np.ascontiguousarray(m)
    if sample_bits != 16 or not 0 <= valid_bit <= 4:
        raise ValueError("sample_bits is 8 or 16, valid_bit 0 .. 4")
    rng = rng or np.random.default_rng(20241008)
    window = np.uint16(0xFF << valid_bit)
    noise = rng.integers(0, 1 << 16, m.shape, dtype=np.uint16) & ~window
    return np.ascontiguousarray((m.astype(np.uint16) << np.uint16(valid_bit)) | noise).astype("<u2")


def checksum(img):
    h, w, _ = img.shape
    img = np.ascontiguousarray(img)
    return int(lib().rmcv_synth_checksum(ptr(img), w, h, 3 * w))


def svm_weights(seed=20241008, n_class=7):
    """stand-in for the reference's svm.xml, which is not in its repository (.gitignore:40-43): seeded weights with
    the trained model's shape (executable/svm/optimizer.cpp:9,16-19 -- 7 classes, linear C_SVC, 20*20*3 features):
    (weights f32 [21, 1200], rho f64 [21], labels i32 [7])"""
    rng = np.random.default_rng(seed)
    n_df = n_class * (n_class - 1) // 2
    w = (rng.standard_normal((n_df, 1200)) * 1e-3).astype(np.float32)
    rho = (rng.standard_normal(n_df) * 0.05).astype(np.float64)
    return w, rho, np.arange(n_class, dtype=np.int32)


def chessboard(w, h, H, nx, ny, ss=4, lo=40, hi=215):
    """a chessboard of nx x ny unit squares under the homography H (3 x 3: board coordinates -> pixels, pixel centres at integers), every
    pixel the mean of ss x ss samples; dark squares `lo`, light squares and everything off the board `hi` -> (bgr (h, w, 3) uint8 with equal
    channels, the (nx - 1)(ny - 1) analytic inner corners (row-major, (x, y)) float64).  Plain numpy: what the corner refinement's tests
    and tools/corner_bench.py draw"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    Hi = np.linalg.inv(H)
    off = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(w)[:, None] + off[None, :]).reshape(-1)          # sample centres, w ss of them
    ys = (np.arange(h)[:, None] + off[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    den = Hi[2, 0] * X + Hi[2, 1] * Y + Hi[2, 2]
    u = (Hi[0, 0] * X + Hi[0, 1] * Y + Hi[0, 2]) / den
    v = (Hi[1, 0] * X + Hi[1, 1] * Y + Hi[1, 2]) / den
    inside = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)
    dark = inside & (((np.floor(u) + np.floor(v)).astype(np.int64) & 1) == 0)
    val = np.where(dark, float(lo), float(hi)).reshape(h, ss, w, ss).mean(axis=(1, 3))
    gray = np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
    bgr = np.repeat(gray[:, :, None], 3, axis=2)
    ij = np.array([(i, j, 1.0) for j in range(1, ny) for i in range(1, nx)], np.float64)
    p = ij @ H.T
    return np.ascontiguousarray(bgr), p[:, :2] / p[:, 2:3]
