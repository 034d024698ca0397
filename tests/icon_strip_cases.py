"""One seeded case list for the icon at any output size (rm::affine_correction(frame, tmp, icon, {side, side}), the labeler's
strip and sheet), pure numpy on tests/icon_cases.py's 160 x 120 scene: tests/test_icon_strip_cpu.py holds rmcv_affine_correction_host,
rmcv_icon_strip_host and the sheet against the second opinion (tests/independent_icon.py) on it, tests/test_gpu_icon_strip.py sends the same
list through k_icon_strip, tests/test_icon_strip_sanitized.py through the stand-alone program.

cases(side): icon_cases.named_icons(160, 120); the exact-double box box(12, 9, 12 + 2 side - 1, 9 + 2 side - 1) -- the 2:1 area branch of the
resize -- where it fits the frame (sides 80 and 128 do not: "double_80", "double_128" are left out); a side x side box (a resize that is a
copy; at side 128 the frame is 120 rows high, so that box is 128 x 120 at the frame's top); 40 icons of each of random_icon's six kinds,
seeded per side."""
import functools

import numpy as np

import icon_cases as K

W, H = K.W, K.H
SIDES = (1, 7, 20, 33, 80, 128)
RECT_SIZES = ((33, 7), (7, 33))      # ow != oh: only the host function and the shim take them
LEFT_OUT = ("double_80", "double_128")


def double_box(side):
    """the exact 2 side x 2 side box, or None where it does not fit the frame"""
    x1, y1 = 12 + 2 * side - 1, 9 + 2 * side - 1
    return K.box(12, 9, x1, y1) if x1 <= W - 1 and y1 <= H - 1 else None


def square_box(side):
    y0 = 9 if 9 + side - 1 <= H - 1 else 0
    return K.box(12, y0, 12 + side - 1, min(y0 + side - 1, H - 1))


@functools.lru_cache(maxsize=None)
def cases(side):
    """[(name, icon float32 [4, 2])] for output side `side` on the 160 x 120 scene"""
    out = list(K.named_icons(W, H))
    d = double_box(side)
    if d is not None:
        out.append(("double_%d" % side, np.array(d, np.float32)))
    out.append(("square_%d_for_side" % side, np.array(square_box(side), np.float32)))
    rng = np.random.default_rng(K.SEED + 77 * side)
    for kind in range(6):
        for i in range(K.FAMILY):
            out.append(("side%d_family%d_%02d" % (side, kind, i), K.random_icon(rng, H, W, kind)))
    for _, q in out:
        q.setflags(write=False)
    names = [n for n, _ in out]
    assert len(set(names)) == len(names) and not set(names) & set(LEFT_OUT)
    return out


def box_of(icon, w=W, h=H):
    """(bx, by, bw, bh, degenerate) of an icon on a w x h image: imgproc.cpp:11-17 by the second opinion's clamp"""
    import independent_icon as ind
    q = np.array(icon, np.float32).reshape(4, 2)
    x = ind.clamp_coordinates(q[:, 0], np.float32(w) - np.float32(1))
    y = ind.clamp_coordinates(q[:, 1], np.float32(h) - np.float32(1))
    px, py = np.rint(x.astype(np.float64)).astype(np.int64), np.rint(y.astype(np.float64)).astype(np.int64)
    bx, by = int(px.min()), int(py.min())
    bw, bh = int(px.max()) - bx + 1, int(py.max()) - by + 1
    return bx, by, bw, bh, bool(bw <= 0 or bh <= 0 or bx < 0 or by < 0 or bx + bw > w or by + bh > h)


def affine_any(img, icon, ow, oh):
    """the expected picture at (ow, oh): the second opinion's own pieces, warp of the box, then resize_to -- for ow == oh exactly
    independent_icon.affine_correction(img, icon, ow) -> (out uint8 [oh, ow, 3], clamped icon, degenerate)"""
    import independent_icon as ind
    h, w, _ = img.shape
    q = np.array(icon, np.float32).reshape(4, 2).copy()
    q[:, 0] = ind.clamp_coordinates(q[:, 0], np.float32(w) - np.float32(1))
    q[:, 1] = ind.clamp_coordinates(q[:, 1], np.float32(h) - np.float32(1))
    bx, by, bw, bh, deg = box_of(q, w, h)
    if deg:
        return np.zeros((oh, ow, 3), np.uint8), q, 1
    f32 = np.float32
    src = [(q[1, 0] - f32(bx), q[1, 1] - f32(by)), (q[2, 0] - f32(bx), q[2, 1] - f32(by)), (q[0, 0] - f32(bx), q[0, 1] - f32(by))]
    m = ind.get_affine_transform([(float(a), float(b)) for a, b in src], [(0.0, 0.0), (float(bw), 0.0), (0.0, float(bh))])
    warped = ind.warp_affine_same_size(img[by:by + bh, bx:bx + bw], m)
    return ind.resize_to(warped, ow, oh), q, 0


def list_for(ow, oh):
    """the case list an output size is checked on: cases(ow) (the rectangular sizes take their width's list)"""
    return cases(ow)


@functools.lru_cache(maxsize=None)
def expected(ow, oh):
    """[(out, clamped icon, degenerate)] of list_for(ow, oh) on the scene, by the second opinion: computed once, shared, left unchanged"""
    out = [affine_any(K.frame(), q, ow, oh) for _, q in list_for(ow, oh)]
    for o, q, _ in out:
        o.setflags(write=False)
        q.setflags(write=False)
    return out


def strip_ref(img, icons, side, cap, strip_w=None):
    """the strip restated: `side` rows of strip_w (default cap side) pixels; icon j < min(n, cap) at columns [j side, (j + 1) side), zeros elsewhere"""
    strip_w = cap * side if strip_w is None else strip_w
    out = np.zeros((side, strip_w, 3), np.uint8)
    for j, q in enumerate(icons[:cap]):
        out[:, j * side:(j + 1) * side] = affine_any(img, q, side, side)[0]
    return out


def armours_of(icons):
    """an ARMOUR table whose icons are `icons` (everything else zero: the strip reads nothing else)"""
    from rmcv_amd import ARMOUR
    arm = np.zeros(len(icons), ARMOUR)
    for j, q in enumerate(icons):
        arm["icon"][j] = q
    return arm


def sheet_ref(img, binary, blobs, negatives, armours, size, side, flags, max_armours):
    """the sheet restated: source_view_ref.view | view_ref.view at flags 0, over the strip of cap = min(2 vw // side, max_armours)"""
    import source_view_ref as SR
    import view_ref as VR
    vw, vh = size
    out = np.zeros((vh + side, 2 * vw, 3), np.uint8)
    out[:vh, :vw] = SR.view(img, blobs, negatives, armours, size, flags)
    out[:vh, vw:] = VR.view(binary, [], [], [], size, 0)
    cap = min(2 * vw // side, max_armours)
    out[vh:] = strip_ref(img, [a for a in np.asarray(armours)["icon"]] if len(armours) else [], side, cap, 2 * vw)
    return out
