"""The session recorder's packed format, restated in numpy from its specification (include/rmcv_abi.h) -- not from
rmcv_amd/csrc/device_pack.h.

A plane is h rows of w_bytes bytes with a byte lag of 1 .. 4.  Each row is cut into segments of 256 bytes, S = ceil(w_bytes / 256); the last
one is extended with virtual bytes of raw value 0 and residual 0.  Per segment: b_raw = bit length of the greatest byte; for byte i of the row
r = (v[i] - (v[i - lag] if i >= lag else 0)) mod 256, z = ((s << 1) ^ (s >> 7)) & 0xFF with s = r as int8; b_pred = bit length of the greatest
z; raw mode if b_raw <= b_pred, else predicted; header byte b | mode_predicted << 4; payload: for j < b (outermost), k < 4, one little-endian
u64 whose bit L is bit j of the coded value of the segment's byte 4 L + k.  Frame: h S header bytes padded with zeros to 8 | h + 1 u32 row
offsets into the payload area (entry h its size) padded to 8 | the payloads in segment order.
"""
import numpy as np

SEG = 256


def align8(x):
    return (x + 7) & ~7


def segments(w_bytes):
    return -(-w_bytes // SEG)


def head_bytes(w_bytes, h):
    return align8(h * segments(w_bytes)) + align8(4 * (h + 1))


def bound(w_bytes, h):
    return head_bytes(w_bytes, h) + 32 * 8 * h * segments(w_bytes)


def bitlen(x):
    return int(x).bit_length()


def zigzag(r):
    s = r.astype(np.uint8).view(np.int8).astype(np.int32)
    return ((s << 1) ^ (s >> 7)) & 0xFF


def unzigzag(z):
    z = z.astype(np.int32)
    return ((z >> 1) ^ -(z & 1)) & 0xFF


def _row_codes(row, lag):
    """(raw, z) of a row, each padded with virtual zeros to whole segments"""
    w = len(row)
    v = row.astype(np.int32)
    pred = np.zeros(w, np.int32)
    pred[lag:] = v[:w - lag] if w > lag else []
    z = zigzag((v - pred) & 0xFF)
    pad = segments(w) * SEG - w
    return np.concatenate([v, np.zeros(pad, np.int32)]), np.concatenate([z, np.zeros(pad, np.int32)])


def _words(coded, b):
    """the 4 b little-endian u64 words of a segment's 256 coded values"""
    out = np.zeros(4 * b, np.uint64)
    lanes = coded.reshape(64, 4)                       # [L][k] = byte 4 L + k
    for j in range(b):
        for k in range(4):
            bits = ((lanes[:, k] >> j) & 1).astype(np.uint64)
            out[4 * j + k] = np.bitwise_or.reduce(bits << np.arange(64, dtype=np.uint64))
    return out.astype("<u8").view(np.uint8)


def pack(plane, lag):
    """plane (h, w_bytes) uint8 -> the packed frame as uint8[size]"""
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    S = segments(w)
    header = np.zeros(align8(h * S), np.uint8)
    table = np.zeros(align8(4 * (h + 1)) // 4, "<u4")
    payload = []
    total = 0
    for y in range(h):
        table[y] = total
        raw, z = _row_codes(plane[y], lag)
        for s in range(S):
            sv, sz = raw[s * SEG:(s + 1) * SEG], z[s * SEG:(s + 1) * SEG]
            b_raw, b_pred = bitlen(sv.max()), bitlen(sz.max())
            pred = not b_raw <= b_pred
            b = b_pred if pred else b_raw
            header[y * S + s] = b | (int(pred) << 4)
            payload.append(_words(sz if pred else sv, b))
            total += 32 * b
    table[h] = total
    return np.concatenate([header, table.view(np.uint8)] + payload)


def unpack(packed, w_bytes, h, lag):
    """the inverse, for round trips of the restatement itself"""
    packed = np.asarray(packed, np.uint8)
    S = segments(w_bytes)
    H = align8(h * S)
    at = head_bytes(w_bytes, h)
    out = np.zeros((h, S * SEG), np.int32)
    for y in range(h):
        for s in range(S):
            hb = int(packed[y * S + s])
            b, pred = hb & 15, hb >> 4
            words = packed[at:at + 32 * b].view("<u8").astype(np.uint64)
            at += 32 * b
            coded = np.zeros((64, 4), np.int32)
            for j in range(b):
                for k in range(4):
                    coded[:, k] |= (((words[4 * j + k] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.int32)) << j
            coded = coded.reshape(SEG)
            if pred:
                r = unzigzag(coded)
                for t in range(SEG):
                    i = s * SEG + t
                    out[y, i] = (r[t] + (out[y, i - lag] if i >= lag else 0)) & 0xFF
            else:
                out[y, s * SEG:(s + 1) * SEG] = coded
    assert H + align8(4 * (h + 1)) <= at == len(packed)
    return out[:, :w_bytes].astype(np.uint8)


# ---- the case list: shapes and inputs the CPU, sanitizer and GPU tests share ----
WIDTHS = (1, 3, 255, 256, 257, 480, 600)
HEIGHTS = (1, 2, 17)
KINDS = ("zero", "constant", "noise", "ramp", "bright", "poisson")


def plane(kind, w_bytes, h, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * w_bytes + h)
    if kind == "zero":
        return np.zeros((h, w_bytes), np.uint8)
    if kind == "constant":
        return np.full((h, w_bytes), 0x5A, np.uint8)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w_bytes), dtype=np.uint8)
        return a
    if kind == "ramp":                                     # wraps 255 -> 0 inside the rows
        return ((np.arange(w_bytes)[None, :] * 3 + np.arange(h)[:, None] * 251 + 250) & 0xFF).astype(np.uint8)
    if kind == "bright":                                   # one bright byte in a dark segment
        a = rng.integers(0, 4, (h, w_bytes), dtype=np.uint8)
        a[h // 2, w_bytes // 2] = 0xF3
        return a
    if kind == "poisson":
        return np.minimum(rng.poisson(6.0, (h, w_bytes)), 255).astype(np.uint8)
    raise ValueError(kind)


def cases():
    """(kind, w_bytes, h, lag): every width and height, every lag (w_bytes < lag included), every kind of input"""
    return [(kind, w, h, lag) for w in WIDTHS for h in HEIGHTS for kind in KINDS for lag in (1, 2, 3, 4)]


_packed = {}


def packed(kind, w_bytes, h, lag, seed=0):
    """pack(plane(...)) of a case, computed once for all the tests that compare against it (read-only)"""
    key = (kind, w_bytes, h, lag, seed)
    if key not in _packed:
        p = pack(plane(kind, w_bytes, h, seed), lag)
        p.setflags(write=False)
        _packed[key] = p
    return _packed[key]
