"""Geometry for the debug-view tests: images, light blobs, negative contours and armours chosen so that every branch of the
line rasteriser, the clip and the resize is walked.  Shared by tests/test_view_cpu.py, tests/test_view_sanitized.py and tests/test_gpu_view.py;
tests/view_ref.py draws them independently of the library."""
import numpy as np

from rmcv_amd.abi import ARMOUR, CAMP_BLUE, CAMP_RED, LIGHTBLOB

# (w, h) -> (vw, vh): general downscale (four plane words per row, the last 8 pixels wide), the exact-2x area path, the copy, an upscale,
# an odd width (row tails that are no whole dword), and a view of one pixel (a source span no tile can stage)
SIZES = [((200, 136), (160, 102)), ((128, 96), (64, 48)), ((96, 64), (96, 64)), ((96, 64), (160, 96)), ((200, 136), (150, 101)), ((70, 40), (1, 1))]


def binary(w, h, seed=7):
    """a 0 / 255 image with fine and coarse structure: noise, bars and a filled block"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    b = (rng.random((h, w)) < 0.2).astype(np.uint8) * 255
    b[h // 4:h // 2, w // 8:w // 3] = 255
    b[:, w // 2::7] = 255
    b[h - 1, :] = 255
    b[:, w - 1] = 255
    return b


def blob(vertices, target=CAMP_BLUE):
    r = np.zeros(1, LIGHTBLOB)
    r["vertices"][0] = np.asarray(vertices, np.float32).reshape(4, 2)
    r["target"][0] = target
    return r


def blobs(*rows):
    return np.concatenate(rows) if rows else np.zeros(0, LIGHTBLOB)


def armour(vertices, icon):
    r = np.zeros(1, ARMOUR)
    r["vertices"][0] = np.asarray(vertices, np.float32).reshape(4, 2)
    r["icon"][0] = np.asarray(icon, np.float32).reshape(4, 2)
    return r


def armours(*rows):
    return np.concatenate(rows) if rows else np.zeros(0, ARMOUR)


def _case(name, b=None, n=None, a=None):
    return dict(name=name, blobs=b if b is not None else blobs(), negatives=[np.asarray(c, np.int32).reshape(-1, 2) for c in (n or [])],
                armours=a if a is not None else armours())


def cases(w, h):
    """the case list for a w x h image"""
    cx, cy = w // 2, h // 2
    r = min(w, h) // 3
    out = []
    # every octant, both directions: two-point contours are drawn there and back (dx < 0 on the way back)
    star = []
    for dx, dy in [(r, r // 3), (r // 3, r), (-r // 3, r), (-r, r // 3), (-r, -r // 3), (-r // 3, -r), (r // 3, -r), (r, -r // 3), (r, 0), (0, r), (r, r), (-r, r)]:
        star.append([(cx, cy), (cx + dx, cy + dy)])
    out.append(_case("octants", n=star))
    # a blob per octant pair as a thin 4-gon, both colours
    out.append(_case("blob_octants", b=blobs(blob([(cx - r, cy - 2), (cx - 3, cy - r), (cx + r, cy + 1), (cx + 2, cy + r)], CAMP_RED),
                                             blob([(5, 5), (w - 6, 9), (w - 9, h - 6), (8, h - 9)], CAMP_BLUE))))
    # dx < 0 with clipping: endpoints outside each border, outside two at once, and edges wholly outside
    out.append(_case("clipped", n=[[(w + 20, cy - 7), (-15, cy + 9)], [(cx + 9, -30), (cx - 11, h + 25)], [(-w, -h // 2), (w // 3, h + 40)],
                                   [(w + 33, -21), (-9, h + 13)], [(-40, h + 30), (w + 17, -25)], [(-5, 3), (4, -6)], [(w - 3, h + 4), (w + 6, h - 5)]],
                     b=blobs(blob([(-20.0, -10.0), (w + 30.0, 12.0), (w + 8.0, h + 19.0), (-31.0, h - 4.0)], CAMP_RED))))
    out.append(_case("outside", n=[[(-50, -50), (-10, -3)], [(w + 5, 0), (w + 90, h)], [(0, h), (w, h + 1)], [(-1, 0), (-1, h - 1)], [(w, 5), (w, 9)]],
                     b=blobs(blob([(-90, 10), (-10, 10), (-10, 60), (-90, 60)])),
                     a=armours(armour([(w + 1, 1), (w + 50, 1), (w + 50, 30), (w + 1, 30)], [(0, -9), (w, -9), (w, -1), (0, -1)]))))
    # a point polygon: one contour point, and a blob whose four vertices coincide; also at the corners
    out.append(_case("points", n=[[(cx, cy)], [(0, 0)], [(w - 1, h - 1)], [(w, h)], [(cx + 3, cy)], [(cx + 3, cy)]],
                     b=blobs(blob([(7, 9)] * 4, CAMP_RED), blob([(w - 1, 0)] * 4))))
    # half-integer vertices: round half to even -- 10.5 -> 10, 11.5 -> 12, -0.5 -> -0, 0.5 -> 0, 1.5 -> 2
    out.append(_case("half_even", b=blobs(blob([(10.5, 11.5), (30.5, 12.5), (31.5, 40.5), (9.5, 39.5)], CAMP_RED), blob([(-0.5, 0.5), (1.5, 2.5), (2.5, 3.5), (0.5, 1.5)])),
                     a=armours(armour([(20.5, 20.5), (50.5, 21.5), (49.5, 33.5), (21.5, 32.5)], [(24.5, 10.5), (44.5, 10.5), (44.5, 44.5), (24.5, 44.5)]))))
    # both blob colours overlapping, in both orders: the later one wins where they cross
    a_, b_ = [(cx - r, cy - 5), (cx + r, cy - 5), (cx + r, cy + 5), (cx - r, cy + 5)], [(cx - 5, cy - r), (cx + 5, cy - r), (cx + 5, cy + r), (cx - 5, cy + r)]
    out.append(_case("red_then_blue", b=blobs(blob(a_, CAMP_RED), blob(b_, CAMP_BLUE))))
    out.append(_case("blue_then_red", b=blobs(blob(a_, CAMP_BLUE), blob(b_, CAMP_RED), blob(a_, 7))))
    # negatives crossing blob edges and armours over both
    ring = [(cx - r + i, cy - r // 2) for i in range(2 * r)] + [(cx + r, cy - r // 2 + i) for i in range(r)] + [(cx + r - i, cy + r // 2) for i in range(2 * r)] + \
           [(cx - r, cy + r // 2 - i) for i in range(r)]
    out.append(_case("crossing", b=blobs(blob(a_, CAMP_BLUE), blob(b_, CAMP_BLUE)), n=[ring, [(cx - r - 3, cy - r), (cx + r + 2, cy + r)]],
                     a=armours(armour([(cx - r // 2, cy - r // 2), (cx + r // 2, cy - r // 3), (cx + r // 2, cy + r // 2), (cx - r // 2, cy + r // 3)],
                                      [(cx - 4, cy - r), (cx + 4, cy - r), (cx + 4, cy + r), (cx - 4, cy + r)]))))
    out.append(_case("empty"))
    # segments with an endpoint that is not finite, or too large: skipped, the polygon's other edges drawn
    out.append(_case("skipped", b=blobs(blob([(10, 10), (np.nan, 20), (40, 30), (15, 35)]), blob([(np.inf, 1), (60, 8), (70, 30), (50, 20)], CAMP_RED),
                                         blob([(5, 5), (2.0 ** 30, 9), (30, 50), (-2.0 ** 31, 4)])),
                     n=[[(3, 3), (2 ** 30, 10), (20, 25)], [(w - 4, 4), (-2 ** 31, h), (cx, cy)]]))
    # seeded random polygons with vertices up to +-3x the image
    rng = np.random.default_rng(20240611 + w * 131 + h)
    def quad(): return np.stack([rng.integers(-3 * w, 3 * w, 4), rng.integers(-3 * h, 3 * h, 4)], 1) + rng.choice([0.0, 0.5, 0.25], (4, 2))
    rb = blobs(*[blob(quad(), int(rng.integers(0, 2))) for _ in range(6)])
    rn = [np.stack([rng.integers(-3 * w, 3 * w, k), rng.integers(-3 * h, 3 * h, k)], 1) for k in (2, 3, 5, 9)]
    ra = armours(*[armour(quad(), quad()) for _ in range(4)])
    out.append(_case("random", b=rb, n=rn, a=ra))
    return out
