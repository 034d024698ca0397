"""Inputs of the view-label tests: the numbers the f6 format is checked on, and the blit cases -- a 96 x 40 view of a 64 x 48
geometry (ratios 1.5 and 0.8333: neither is an integer) at scales 1, 2 and 8.  Shared by tests/test_view_labels_cpu.py,
tests/test_view_labels_sanitized.py and tests/test_gpu_view_labels.py; the expected pictures are tests/label_ref.py's."""
import math
import random

import numpy as np

from rmcv_amd.abi import ARMOUR, TRACK

W, H, VW, VH = 64, 48, 96, 40
SCALES = (1, 2, 8)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# ---- the numbers -------------------------------------------------------------------------------------------------------------------------
F6_FIXED = [0.0, -0.0, 5e-324, 0.5e-6, 1.5e-6, 2.5e-6, 0.9999995, 9.9999995, 123456.7890125, 999999999999999.875, -1e-9]
F6_PINNED = [(float("nan"), "nan"), (-float("nan"), "nan"), (float("inf"), "inf"), (-float("inf"), "-inf"), (1e15, "big"), (-1e15, "-big"),
             (1.7e308, "big"), (-1.7e308, "-big"), (math.nextafter(1e15, 0), "999999999999999.875000"),
             (-math.nextafter(1e15, 0), "-999999999999999.875000")]


def f6_neighbours():
    """the doubles adjacent to each fixed value, both signs (the one above 999999999999999.875 is 1e15 itself, where "%f" no longer is the
    rule: it is pinned as "big" in F6_PINNED)"""
    out = []
    for v in F6_FIXED:
        out += [v, -v, math.nextafter(v, math.inf), math.nextafter(v, -math.inf), math.nextafter(-v, math.inf), math.nextafter(-v, -math.inf)]
    return [v for v in out if abs(v) < 1e15]


def f6_ties():
    """the values on which round-half-even decides.  A six-decimal tie is v 10^6 = q + 1/2 exactly, i.e. v = (2 q + 1) / (2^7 5^6); a
    double is k / 2^j, so 5^6 must divide 2 q + 1 and the ties are exactly the k / 2^7 with k odd (0.0078125 -> 0.007812, 0.0234375 ->
    0.023438).  Here: every odd k below 2^10 and some large ones, both signs, with their neighbours one ulp either side (no ties: the
    ordinary rule); then k / 2^j for every other j up to 29, exact binary values with up to 29 decimals that are NOT ties."""
    out = []
    for k in list(range(1, 2 ** 10, 2)) + [2 ** 20 + 1, 2 ** 30 + 3, 2 ** 40 + 5, 2 ** 50 + 7, 2 ** 53 - 1]:
        v = k / 2 ** 7
        if v < 1e15:
            out += [v, -v, math.nextafter(v, 0), math.nextafter(v, math.inf)]
    # k / 2^j for every j: ties only at j = 7, but each is an exact binary value with many decimals
    for j in range(1, 30):
        for k in (1, 3, 5, 2 ** j - 1, 2 ** j + 1, 12345 * 2 + 1):
            out += [k / 2 ** j, -k / 2 ** j]
    return out


def f6_seeded(n=20000, seed=20261020):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        v = math.ldexp(1 + rng.random(), rng.randint(-1080, 49)) * rng.choice((1, -1))
        if abs(v) < 1e15:
            out.append(v)
    return out


# ---- the blit cases ----------------------------------------------------------------------------------------------------------------------
def armours(*anchors):
    """ARMOUR records whose vertices[0] is the anchor (the other fields are never read by the label pass: filled with a recognisable slope)"""
    a = np.zeros(len(anchors), ARMOUR)
    for i, (x, y) in enumerate(anchors):
        a[i]["vertices"] = [[x, y], [x + 9, y], [x + 9, y + 5], [x, y + 5]]
        a[i]["icon"] = a[i]["vertices"] + 1
        a[i]["bbox"] = [x, y, 9, 5]
    return a


def tracks(rows):
    """TRACK records from (identity, lost_count, initialized, position, state_post[0:3]) rows"""
    t = np.zeros(len(rows), TRACK)
    for i, (identity, lost, init, pos, post) in enumerate(rows):
        t[i]["identity"], t[i]["lost_count"], t[i]["initialized"] = identity, lost, init
        t[i]["position"] = pos
        t[i]["state_post"][:3] = post
        t[i]["state_post"][3:] = [7.5, -7.5, 0.25]   # (velocities: never printed)
        t[i]["timestamp"] = 1000 + i
    return t


def quad(x, y, w=12, h=7):
    return np.array([[x, y], [x + w, y + 1], [x + w - 1, y + h], [x - 1, y + h - 1]], np.float32)


def case(name, arm=(), ids=None, pos=None, trk=(), side=(), origin=(0, 0), stride=3 * VW, geometry=(W, H)):
    a = armours(*arm)
    return dict(name=name, armours=a, identities=None if ids is None else np.array(ids, np.int32),
                positions=None if pos is None else np.array(pos, np.float64).reshape(-1, 3), tracks=tracks(list(trk)),
                side=np.array(side, np.float32).reshape(-1, 4, 2), origin=origin, stride=stride, geometry=geometry)


NAN = float("nan")


def cases():
    """every case is run at every scale of SCALES"""
    return [
        case("plain", arm=[(10, 30)], ids=[3], pos=[[1.5, -2.25, 300.125]]),
        case("defaults", arm=[(4, 20)]),                                               # identities / positions NULL: -1: 0.000000, ...
        case("none", arm=[]),                                                          # n_armours == 0
        case("clip_left", arm=[(-6, 24)], ids=[12], pos=[[0.5, 0.25, 0.125]]),         # negative anchor: the floor (-6 * 96 / 64 = -9)
        case("floor_not_trunc", arm=[(-1, 20)], ids=[8], pos=[[1, 2, 3]]),             # -1 * 96 / 64 = -1.5 -> -2, truncation gives -1
        case("clip_right", arm=[(58, 24)], ids=[7], pos=[[9, 8, 7]]),
        case("clip_top", arm=[(8, 3)], ids=[1], pos=[[1, 1, 1]]),
        case("clip_bottom", arm=[(8, 47)], ids=[2], pos=[[2, 2, 2]]),
        case("below", arm=[(8, 300)], ids=[2], pos=[[2, 2, 2]]),                       # entirely outside, four ways
        case("above", arm=[(8, -300)], ids=[2], pos=[[2, 2, 2]]),
        case("left", arm=[(-3000, 20)], ids=[2], pos=[[2, 2, 2]]),
        case("right", arm=[(3000, 20)], ids=[2], pos=[[2, 2, 2]]),
        case("half_even", arm=[(10.5, 21.5), (11.5, 35.5)], ids=[4, 5], pos=[[0, 0, 0], [1, 1, 1]]),   # 10.5 -> 10, 21.5 -> 22; 11.5 -> 12, 35.5 -> 36
        case("nan_vertex", arm=[(NAN, 20), (12, NAN), (2.0 ** 30, 20), (6, 44)], ids=[1, 2, 3, 4], pos=[[1, 1, 1]] * 4),   # three skipped, one drawn
        case("overlap", arm=[(10, 30), (11, 31)], ids=[3, 4], pos=[[1.5, -2.25, 300.125], [NAN, float("inf"), -1e300]]),
        case("specials", arm=[(0, 16), (0, 30), (0, 44)], ids=[INT32_MIN, INT32_MAX, 0],
             pos=[[NAN, float("inf"), -float("inf")], [1e15, -1e15, -0.0], [999999999999999.875, -1e-9, 2.5e-6]]),
        case("track", trk=[(5, 3, 1, [1, 2, 3], [10.5, -20.25, 30.125])], side=[quad(12, 10)]),
        case("track_uninitialised", trk=[(6, 0, 0, [1.25, 2.5, 3.75], [10.5, -20.25, 30.125])], side=[quad(20, 14)]),   # position, not state_post
        case("track_under_armour", arm=[(12, 24)], ids=[5], pos=[[10.5, -20.25, 30.125]],
             trk=[(5, 26, 1, [0, 0, 0], [10.5, -20.25, 30.125])], side=[quad(12, 24)]),                                # yellow wins
        case("track_window", arm=[(12, 24)], trk=[(1, 0, 1, [0, 0, 0], [1, 2, 3]), (2, 1, 1, [0, 0, 0], [4, 5, 6])],
             side=[quad(112, 224), quad(140, 230)], origin=(96, 200)),                                                 # (x_eff, y_eff) != (0, 0)
        case("track_clipped", trk=[(9, 9, 1, [0, 0, 0], [9, 9, 9]), (10, 0, 1, [0, 0, 0], [1, 1, 1])],
             side=[quad(-8, 40, 30, 20), quad(50, -4, 40, 9)]),                                                        # quads across the edges
        case("track_far", trk=[(9, 9, 1, [0, 0, 0], [9, 9, 9])], side=[[[5, 5], [2.0 ** 29, 9], [2.0 ** 29, 2.0 ** 29], [5, 30]]]),   # far outside: the clip on 64-bit positions
        case("track_nan_vertex", trk=[(3, 0, 1, [0, 0, 0], [3, 3, 3]), (4, 0, 1, [0, 0, 0], [4, 4, 4])],
             side=[[[10, 20], [30, NAN], [30, 30], [10, 30]], [[NAN, 20], [50, 20], [50, 30], [40, 30]]]),  # no quad but a line; neither
        case("five_tracks", trk=[(i, i, i & 1, [i, i, i], [-i, -i, -i]) for i in range(5)], side=[quad(4 + 10 * i, 6 + 8 * i) for i in range(5)]),
        case("odd_stride", arm=[(10, 30), (58, 24)], ids=[3, 7], pos=[[1.5, -2.25, 300.125], [9, 8, 7]],
             trk=[(5, 3, 1, [1, 2, 3], [10.5, -20.25, 30.125])], side=[quad(12, 10)], stride=3 * VW + 7),              # not a multiple of 4; the tail bytes stay
    ]


def background(stride, seed=5):
    """a finished view to draw over, as a flat buffer of rows `stride` bytes apart (the last row ends with its last pixel): noise, so
    that a pixel written that should not be, or left that should be written, shows -- except where it would equal an overlay colour"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(1, 255, stride * (VH - 1) + 3 * VW, dtype=np.uint8)   # never 0 or 255: no pixel is yellow or magenta by chance
    return buf


def rows_of(buf, stride):
    """(VH, stride) view of a flat buffer's rows, the last one padded virtually: use [:, :3 * VW] for the pixels"""
    return np.lib.stride_tricks.as_strided(buf, (VH, 3 * VW), (stride, 1))
