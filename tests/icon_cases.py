"""One seeded case list for the icon path (rm::affine_correction + the one-vs-one vote), pure numpy: tests/test_icon_cases_cpu.py holds the
oracle and the second opinion against each other on it and asserts that it reaches every branch of the oracle's census;
tests/test_gpu_icon_cases.py sends the same list through every instantiation and every consumer of icon_row and of the vote on the device.

Scenes: a 160 x 120 BGR frame (noise + ramp + checkerboard; even dimensions, so the same bytes serve as a mosaic) and 96 x 64 windows of
it whose origin x is a multiple of 16.  icon_cases(w, h) is the list for an image of that extent; vote_cases() the list of models and rows.
Icon vertices: [0] bottom-left, [1] top-left, [2] top-right, [3] bottom-right; the affine map is fixed by [1], [2], [0]."""
import functools
import itertools

import numpy as np

W, H = 160, 120
WIN_W, WIN_H = 96, 64
WIN_ORIGINS = [(32, 40), (0, 0), (64, 56), (16, 8), (48, 24), (64, 0), (0, 56), (32, 17)]   # effective as they are: x % 16 == 0, inside the frame
SEED = 20250607
ROW = 1200
F32 = np.float32


def scene(rng, h, w):
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[..., 1] = (np.arange(w)[None, :] * 255 // max(1, w - 1)).astype(np.uint8)      # a ramp: interpolation errors cannot hide in noise
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 2] = ((xx // 7 + yy // 5) % 2 * 200 + 20).astype(np.uint8)                # and a checkerboard: every tap matters
    return img


def random_icon(rng, h, w, kind=None):
    drawn = rng.integers(0, 6)
    kind = drawn if kind is None else kind
    cx, cy = rng.uniform(0, w), rng.uniform(0, h)
    if kind == 0:                                             # exact 40 x 40 box: the 2:1 area branch of resize
        x0, y0 = int(rng.integers(0, w - 41)), int(rng.integers(0, h - 41))
        return np.array([[x0, y0 + 39], [x0, y0], [x0 + 39, y0], [x0 + 39, y0 + 39]], np.float32)
    if kind == 1:                                             # tiny: 1..4 px boxes (every column clamped in resize)
        s = rng.uniform(0.3, 3.5)
        q = np.array([[-s, s], [-s, -s], [s, -s], [s, s]]) * 0.5 + (cx, cy)
        return q.astype(np.float32)
    sx, sy = rng.uniform(4, 160), rng.uniform(4, 160)
    ang = rng.uniform(-0.6, 0.6)
    base = np.array([[-sx, sy], [-sx, -sy], [sx, -sy], [sx, sy]]) * 0.5        # [0] bottom-left, [1] top-left, [2] top-right, [3] bottom-right
    if kind >= 4:
        base += rng.normal(0, 0.08 * min(sx, sy), base.shape)                  # a sheared / perspective-looking quad
    r = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    q = base @ r.T + (cx, cy)
    if kind == 3:
        q += rng.uniform(-0.4, 0.4) * np.array([w, h])                          # partly (or wholly) outside: the clamp of imgproc.cpp:11-15
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def frame():
    f = scene(np.random.default_rng(SEED), H, W)
    f.setflags(write=False)
    return f


def window(k):
    x, y = WIN_ORIGINS[k]
    return np.ascontiguousarray(frame()[y:y + WIN_H, x:x + WIN_W])


def box(x0, y0, x1, y1):
    """the upright icon whose vertices are the corners (x0, y0) .. (x1, y1): an (x1 - x0 + 1) x (y1 - y0 + 1) box for integers"""
    return [[x0, y1], [x0, y0], [x1, y0], [x1, y1]]


QUAD = [[20, 50], [28, 12], [80, 20], [72, 58]]               # a tilted rectangle-like quadrilateral, no two coordinates equal
RECT = box(22, 14, 75, 49)
PROBE = [[np.nan, 50], [30, np.inf], [-np.inf, 10], [60, 60]]


# Two of the three defining vertices share their x exactly and the third lies left of them (a fourth, far left, sets the box's origin): two
# rows of the 6 x 6 system tie for the pivot of a column.  The search takes the FIRST maximum; on frame() taking the last one instead
# changes bytes of these icons (found by a seeded search with the second opinion; tests/test_icon_cases_cpu.py asserts it).
PIVOT_TIES = [
    [[35.34575271606445, 6.766864776611328], [35.31424331665039, 36.868438720703125], [35.34575271606445, 100.0252685546875], [0.786440372467041, 4.245222568511963]],
    [[85.01763153076172, 34.985626220703125], [28.030275344848633, 95.34272003173828], [85.01763153076172, 90.23444366455078], [1.3884226083755493, 1.2851303815841675]],
    [[91.98729705810547, 84.64155578613281], [91.98729705810547, 99.82141876220703], [24.383508682250977, 63.99353790283203], [2.6445224285125732, 2.5963406562805176]],
    [[35.79475784301758, 30.507532119750977], [28.569805145263672, 93.23027038574219], [35.79475784301758, 86.37278747558594], [2.8978142738342285, 2.1970207691192627]],
    [[108.15150451660156, 36.720096588134766], [45.558509826660156, 54.99853515625], [108.15150451660156, 18.954570770263672], [0.15495239198207855, 1.1521066427230835]],
    [[126.40721130371094, 104.39445495605469], [75.04612731933594, 91.7577896118164], [126.40721130371094, 85.76275634765625], [2.4136996269226074, 3.8347432613372803]],
]


def named_icons(w, h):
    """[(name, icon float32 [4, 2])] for a w x h image"""
    out = []

    def add(name, q):
        out.append((name, np.array(q, np.float32).reshape(4, 2)))
    for k, q in enumerate(PIVOT_TIES):                                        # first: they land in frame 0 of a batch, the scene itself
        add("pivot_tie_%d" % k, q)
    add("upright_integer_41", box(20, 10, 60, 50))                            # fx = fy = 0 at the origin: the saturated w00 tap
    add("area_40x40", box(30, 20, 69, 59))
    for s in (1, 2, 19, 20, 21, 41):
        add("w%d_tall" % s, box(40, 4, 40 + s - 1, 60))
        add("h%d_wide" % s, box(8, 20, 84, 20 + s - 1))
        add("square_%d" % s, box(12, 9, 12 + s - 1, 9 + s - 1))
    for name, q in (("left", box(0, 20, 25, 45)), ("right", box(w - 26, 20, w - 1, 45)), ("top", box(30, 0, 55, 25)), ("bottom", box(30, h - 26, 55, h - 1)),
                    ("top_left", box(0, 0, 25, 25)), ("top_right", box(w - 26, 0, w - 1, 25)), ("bottom_left", box(0, h - 26, 25, h - 1)),
                    ("bottom_right", box(w - 26, h - 26, w - 1, h - 1))):
        add("touches_" + name, q)
    for name, q in (("left", box(-60, 20, -20, 45)), ("right", box(w + 20, 20, w + 60, 45)), ("above", box(30, -50, 55, -10)), ("below", box(30, h + 10, 55, h + 50)),
                    ("beyond_corner", box(w + 5, h + 5, w + 40, h + 40))):
        add("outside_" + name, q)
    add("larger_than_the_image", box(-50, -30, w + 50, h + 30))
    add("straddles_left_top", box(-10.25, -7.5, 30.75, 33.5))
    add("straddles_right_bottom", [[w - 30.5, h + 9], [w - 28, h - 33.25], [w + 12, h - 30], [w + 9.5, h + 12.25]])
    add("half_corners_round_to_even", [[10.5, 20.5], [10.5, 11.5], [20.5, 11.5], [20.5, 20.5]])   # box 10, 12, 11 x 9
    add("half_corners_round_to_even_2", [[11.5, 21.5], [11.5, 12.5], [21.5, 12.5], [21.5, 21.5]])  # box 12, 12, 11 x 11
    add("point", [[50, 40]] * 4)
    add("point_fractional", [[50.3, 40.7]] * 4)
    add("collinear_horizontal", [[10, 30], [30, 30], [50, 30], [40, 50]])
    add("collinear_vertical", [[30, 10], [30, 30], [30, 50], [50, 40]])
    add("collinear_diagonal", [[10, 50], [30, 30], [50, 10], [60, 60]])
    add("collinear_diagonal_fractional", [[10.25, 50.5], [30.25, 30.5], [50.25, 10.5], [60, 60]])
    near = np.array([[10, 50], [30, 30], [50, 10], [60, 60]], np.float32)
    for slot, way in itertools.product(range(2), (np.inf, -np.inf)):
        q = near.copy()
        q[1, slot] = np.nextafter(q[1, slot], F32(way))
        add("near_collinear_%s_%s" % ("xy"[slot], "up" if way > 0 else "down"), q)
    for base, corners in (("quad", QUAD), ("rect", RECT)):
        for p in itertools.permutations(range(4)):                            # every ordering: which row is the pivot of each column
            add("%s_order_%d%d%d%d" % ((base,) + p), [corners[i] for i in p])
    add("mirror", [QUAD[3], QUAD[2], QUAD[1], QUAD[0]])                       # negative determinant
    add("rotated_90", QUAD[1:] + QUAD[:1])
    add("rotated_180", QUAD[2:] + QUAD[:2])
    add("rotated_270", QUAD[3:] + QUAD[:3])
    for value, vname in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "minus_inf"), (-0.0, "minus_zero")):
        for i in range(4):
            for k in range(2):
                q = np.array(QUAD, np.float32)
                q[i, k] = value
                add("%s_in_%d%s" % (vname, i, "xy"[k]), q)
    add("probe_nan_inf", PROBE)
    add("all_nan", [[np.nan, np.nan]] * 4)
    add("all_minus_zero", [[-0.0, -0.0]] * 4)
    add("minus_zero_corner_box", [[-0.0, 30.0], [-0.0, -0.0], [25.0, -0.0], [25.0, 30.0]])
    return out


FAMILY = 40   # of each of random_icon's six kinds


@functools.lru_cache(maxsize=None)
def icon_cases(w, h):
    """[(name, icon)] for a w x h image: the named icons, then 40 of each kind of random_icon"""
    out = named_icons(w, h)
    rng = np.random.default_rng(SEED + 1000 * w + h)
    for kind in range(6):
        for i in range(FAMILY):
            out.append(("family%d_%02d" % (kind, i), random_icon(rng, h, w, kind)))
    for _, q in out:
        q.setflags(write=False)
    return out


def split(n, parts, least=9):
    """range(n) in `parts` consecutive slices of sizes n // parts - parts // 2 + k (the remainder goes to the first): all different but
    possibly the first, each at least `least` long"""
    sizes = [n // parts - parts // 2 + k for k in range(parts)]
    sizes[0] += n - sum(sizes)
    assert min(sizes) >= least
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [slice(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


# ---------------------------------------------------------------- the clamp, transcribed
def clamp_transcribed(icon, w, h):
    """std::max(0.0f, std::min(v, lim)) with min(a, b) = (b < a) ? b : a and max(a, b) = (a < b) ? b : a, scalar by scalar in float32"""
    out = np.array(icon, np.float32).reshape(4, 2).copy()
    zero = F32(0)
    for i in range(4):
        for k, lim in enumerate((F32(w) - F32(1), F32(h) - F32(1))):
            a, b = out[i, k], lim                                              # min(v, lim)
            t = b if b < a else a
            a, b = zero, t                                                    # max(0, t)
            out[i, k] = b if a < b else a
    return out


# ---------------------------------------------------------------- the vote, restated
def kvals(weights, row):
    """the linear kernel of every decision function as SVMImpl::predict computes it: float32 products, four of them summed left to right in
    float32, the sums accumulated in order in a double; the result rounded to float32"""
    w = np.asarray(weights, np.float32).reshape(-1, ROW)
    x = np.asarray(row, np.uint8).reshape(ROW).astype(np.float32)
    with np.errstate(all="ignore"):
        p = (w * x[None, :]).astype(np.float32).reshape(len(w), ROW // 4, 4)
        q = (((p[:, :, 0] + p[:, :, 1]).astype(np.float32) + p[:, :, 2]).astype(np.float32) + p[:, :, 3]).astype(np.float32)
        out = np.zeros(len(w), np.float32)
        for d in range(len(w)):
            s = np.float64(0)
            for v in q[d]:
                s = s + np.float64(v)
            out[d] = F32(s)
    return out


def vote(weights, rho, labels, n_class, row):
    """-> (label, votes per class): pair (i < j) votes i when -rho + kval > 0 and j otherwise (a NaN votes j); the first maximum wins"""
    k = kvals(weights, row).astype(np.float64)
    votes = [0] * n_class
    d = 0
    with np.errstate(all="ignore"):
        for i in range(n_class):
            for j in range(i + 1, n_class):
                votes[i if (-np.float64(rho[d]) + k[d]) > 0 else j] += 1
                d += 1
    best = 0
    for i in range(1, n_class):
        if votes[i] > votes[best]:
            best = i
    return int(labels[best]), votes


def pairs(n_class):
    return [(i, j) for i in range(n_class) for j in range(i + 1, n_class)]


def rows_from(image, icons):
    """the icon rows of `icons` on `image` by the second opinion (tests/independent_icon.py)"""
    import independent_icon as ind
    return [ind.affine_correction(image, q)[0].reshape(-1) for q in icons]


def edge_cases(row, seed, prefix="edge"):
    """[(name, weights, rho, labels, n_class)] for one icon row: full-mantissa weights over 2^-20 .. 2^20 for 2, 4 and 8 classes, rho at the
    pair's kval (every sum exactly 0), one double below it (every sum > 0), one above, and a seeded mix of the three: the last bit of the
    dot product decides every vote.  kval by kvals() above, not by the library."""
    rng = np.random.default_rng(seed)
    out = []
    for n_class in (2, 4, 8):
        n_df = n_class * (n_class - 1) // 2
        labels = (np.arange(n_class) * 3 + 10).astype(np.int32)
        wts = (rng.choice([-1.0, 1.0], (n_df, ROW)) * rng.uniform(1, 2, (n_df, ROW)) * np.exp2(rng.integers(-20, 21, (n_df, ROW)))).astype(np.float32)
        k = kvals(wts, row).astype(np.float64)
        assert np.isfinite(k).all()
        below, above = np.nextafter(k, -np.inf), np.nextafter(k, np.inf)
        mixed = np.where(rng.integers(0, 3, n_df) == 0, k, np.where(rng.integers(0, 2, n_df) == 0, below, above))
        for tag, rho in (("at", k), ("below", below), ("above", above), ("mixed", mixed)):
            out.append(("%s_%d_%s" % (prefix, n_class, tag), wts, rho, labels, n_class))
    return out


ROW_SOURCES = ("upright_integer_41", "area_40x40", "quad_order_0123", "w19_tall")   # the named icons whose rows the vote cases use


@functools.lru_cache(maxsize=None)
def vote_cases():
    """[(name, weights f32 [n_df, 1200], rho f64 [n_df], labels i32 [n_class], n_class, row u8 [1200], index of the row's icon in
    ROW_SOURCES)]; the rows are those of ROW_SOURCES on frame()"""
    named = dict(named_icons(W, H))
    rows = rows_from(frame(), [named[k] for k in ROW_SOURCES])
    rng = np.random.default_rng(SEED + 7)
    out = []

    def add(name, weights, rho, n_class, src=0, labels=None):
        n_df = n_class * (n_class - 1) // 2
        labels = np.arange(n_class) * 3 + 10 if labels is None else labels   # labels are not class indices
        out.append((name, np.ascontiguousarray(weights, np.float32).reshape(n_df, ROW), np.ascontiguousarray(rho, np.float64).reshape(n_df),
                    np.ascontiguousarray(labels, np.int32).reshape(n_class), n_class, rows[src], src))

    def zeros(n_class):
        return np.zeros((n_class * (n_class - 1) // 2, ROW), np.float32)
    # zero weights, so sum = -rho: every sign pattern for 2 and 3 classes, and the two zeros
    for n_class in (2, 3):
        n_df = n_class * (n_class - 1) // 2
        for signs in itertools.product((-1.0, 1.0), repeat=n_df):
            add("signs_%d_%s" % (n_class, "".join("-+"[s > 0] for s in signs)), zeros(n_class), signs, n_class, src=len(out) % len(rows))
        add("zeros_%d" % n_class, zeros(n_class), [0.0] * n_df, n_class)
        add("minus_zeros_%d" % n_class, zeros(n_class), [-0.0] * n_df, n_class)
        add("nans_%d" % n_class, zeros(n_class), [np.nan] * n_df, n_class)
    # seeded patterns of -1, +1, +0, -0 and NaN for 4 .. 8 classes
    for n_class in range(4, 9):
        n_df = n_class * (n_class - 1) // 2
        for k in range(5):
            rho = rng.choice(np.array([-1.0, 1.0, 1.0, -1.0, 0.0, -0.0, np.nan]), n_df)
            add("pattern_%d_%d" % (n_class, k), zeros(n_class), rho, n_class, src=k % len(rows))
    # every class index the winner, by seven votes to at most six
    for t in range(8):
        add("winner_%d" % t, zeros(8), [-1.0 if i == t else 1.0 for i, j in pairs(8)], 8, src=t % len(rows))
    # ties: the first maximum wins
    add("tie_all_3", zeros(3), [-1.0, 1.0, -1.0], 3)                                     # votes 1 1 1 -> class 0
    add("tie_two_4_first", zeros(4), [-1.0, -1.0, 1.0, -1.0, -1.0, -1.0], 4)             # votes 2 2 1 1 -> class 0
    add("tie_two_4_later", zeros(4), [1.0, -1.0, 1.0, 1.0, -1.0, -1.0], 4)               # votes 1 2 2 1 -> class 1
    for n_class in (5, 7):                                                               # a regular tournament: everybody wins (n - 1) / 2
        add("tie_all_%d" % n_class, zeros(n_class), [-1.0 if (j - i) <= (n_class - 1) // 2 else 1.0 for i, j in pairs(n_class)], n_class)
    # full-mantissa weights on real rows, rho at the pair's kval and one double either side of it (edge_cases)
    for src in range(len(rows)):
        for name, wts, rho, labels, n_class in edge_cases(rows[src], SEED + 100 + src, "edge_%d" % src):
            add(name, wts, rho, n_class, src, labels)
    return out


def model_of(case):
    """(weights, rho, labels) of a vote case, as Context.svm_load and the oracle's classify_armours take them"""
    return case[1], case[2], case[3]


# ---------------------------------------------------------------- a scene for the fused tail (it classifies only armours it has detected)
TAIL_W, TAIL_H = 320, 256
TAIL_PAIRS = [(36, 30, 36, 7, 54, -25), (286, 226, 36, 7, 54, -25), (160, 128, 40, 7, 60, 5), (160, 20, 30, 6, 45, 0), (20, 128, 30, 6, 30, -25)]
#             centre x, y of the pair, bar height and width, centre gap, tilt in degrees: two at opposite corners, one inside, one at the top
#             edge and one at the left edge -- the icons (the bars extended to twice their length) leave the frame on all four sides


def _paint_bar(img, cx, cy, bh, bw, deg, colour=(255, 120, 40)):
    a = np.deg2rad(deg)
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    u = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a)                         # across the bar
    v = (xx - cx) * np.sin(a) - (yy - cy) * np.cos(a)                         # along it
    img[(np.abs(u) <= bw / 2) & (np.abs(v) <= bh / 2)] = colour


@functools.lru_cache(maxsize=None)
def tail_scene():
    """a dark, textured 320 x 256 BGR frame with five pairs of blue bars"""
    rng = np.random.default_rng(SEED + 5)
    img = rng.integers(0, 60, (TAIL_H, TAIL_W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:TAIL_H, 0:TAIL_W]
    img[..., 2] = ((xx // 7 + yy // 5) % 2 * 60 + 10).astype(np.uint8)
    for cx, cy, bh, bw, gap, deg in TAIL_PAIRS:
        ox, oy = gap / 2 * np.cos(np.deg2rad(deg)), gap / 2 * np.sin(np.deg2rad(deg))
        _paint_bar(img, cx - ox, cy - oy, bh, bw, deg)
        _paint_bar(img, cx + ox, cy + oy, bh, bw, deg)
    img.setflags(write=False)
    return img


def sides_clamped(before, after, w, h):
    """which of (left, right, top, bottom) the clamp acted on, for icon tables [n, 4, 2] before and after it"""
    b, a = np.asarray(before, np.float32).reshape(-1, 4, 2), np.asarray(after, np.float32).reshape(-1, 4, 2)
    moved = b != a
    return (bool((moved[..., 0] & (a[..., 0] == 0)).any()), bool((moved[..., 0] & (a[..., 0] == w - 1)).any()),
            bool((moved[..., 1] & (a[..., 1] == 0)).any()), bool((moved[..., 1] & (a[..., 1] == h - 1)).any()))
