"""D(m), the library's demosaic of a raw 8-bit Bayer mosaic (include/rmcv_abi.h: RMCV_OPT_INPUT_FORMAT), restated in plain numpy
for the tests.  The product has no CPU path; this is the yardstick its GPU kernels are held to.

For an interior site (1 <= x <= w-2, 1 <= y <= h-2):
  own colour                            m(x, y)
  G at an R or B site                   (left + right + up + down + 2) >> 2
  at a G site: the colour of its row    (left + right + 1) >> 1;  the colour of its column  (up + down + 1) >> 1
  B at an R site / R at a B site        (four diagonal neighbours + 2) >> 2
Border: D(m)(x, y) = D(m)(clamp(x, 1, w-2), clamp(y, 1, h-2)).
Patterns name the top-left 2x2 block: 1 RG (R G / G B), 2 GB (G B / R G), 3 GR (G R / B G), 4 BG (B G / G R).
"""
import numpy as np

RG, GB, GR, BG = 1, 2, 3, 4
PATTERNS = (RG, GB, GR, BG)


def r_site(pattern):
    """(x, y) parity of the R site in the top-left 2x2 block"""
    if pattern not in PATTERNS:
        raise ValueError("unknown Bayer pattern %r" % (pattern,))
    return (1 if pattern in (GR, BG) else 0), (1 if pattern in (GB, BG) else 0)


def mosaic(bgr, pattern):
    """sample the colour filter array of `pattern` from BGR frames [..., h, w, 3] -> [..., h, w]"""
    rx, ry = r_site(pattern)
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[-3], bgr.shape[-2]
    px = (np.arange(w)[None, :] ^ rx) & 1
    py = (np.arange(h)[:, None] ^ ry) & 1
    ch = np.where((px == 0) & (py == 0), 2, np.where((px == 1) & (py == 1), 0, 1))
    out = np.empty(bgr.shape[:-1], np.uint8)
    for c in range(3):
        sel = np.broadcast_to(ch == c, out.shape)
        out[sel] = bgr[..., c][sel]
    return out


def demosaic(m, pattern):
    """D(m): (h, w) uint8 mosaic -> (h, w, 3) uint8 BGR"""
    m = np.asarray(m)
    assert m.ndim == 2 and m.shape[0] >= 3 and m.shape[1] >= 3
    rx, ry = r_site(pattern)
    h, w = m.shape
    a = m.astype(np.int32)
    own = a[1:-1, 1:-1]
    hs = a[1:-1, :-2] + a[1:-1, 2:]
    vs = a[:-2, 1:-1] + a[2:, 1:-1]
    ds = a[:-2, :-2] + a[:-2, 2:] + a[2:, :-2] + a[2:, 2:]
    px = (np.arange(1, w - 1)[None, :] ^ rx) & 1
    py = (np.arange(1, h - 1)[:, None] ^ ry) & 1
    px, py = np.broadcast_to(px, own.shape), np.broadcast_to(py, own.shape)
    cross, diag = (hs + vs + 2) >> 2, (ds + 2) >> 2
    hm, vm = (hs + 1) >> 1, (vs + 1) >> 1
    r_at, b_at = (px == 0) & (py == 0), (px == 1) & (py == 1)
    g_rrow, g_brow = (px == 1) & (py == 0), (px == 0) & (py == 1)
    B = np.select([r_at, b_at, g_rrow, g_brow], [diag, own, vm, hm])
    G = np.select([r_at, b_at], [cross, cross], own)
    R = np.select([r_at, b_at, g_rrow, g_brow], [own, diag, hm, vm])
    inner = np.stack([B, G, R], axis=-1).astype(np.uint8)
    yi = np.clip(np.arange(h), 1, h - 2) - 1
    xi = np.clip(np.arange(w), 1, w - 2) - 1
    return np.ascontiguousarray(inner[yi][:, xi])
