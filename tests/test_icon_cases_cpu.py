"""The icon path's case list (tests/icon_cases.py) on the CPU:

* the oracle's branch census (oracle/rmcv_oracle.c: ORC_CENSUS_ICON) over the list reaches every counter of the clamp, the box, the 6 x 6 LU,
  the inversion, the warp (at the pixels the resize reads), the resize and the vote -- or the counter is listed in UNREACHABLE with the
  argument, and is then asserted to stay at 0;
* tests/independent_icon.py agrees with the oracle bit for bit on every case: rc, clamped vertices, icon;
* the clamp of every case equals a direct transcription of the two library selects, in raw float32 bits;
* every vote case equals the numpy restatement of the rule in tests/icon_cases.py;
* what reading the code found is asserted: a collinear icon gives the constant image of the ROI's pixel (0, 0); NaN clamps to +0; -0 to +0.
Every comparison is exact; the only conditions are the coverage ones."""
import numpy as np
import pytest

import icon_cases as K
import independent_icon as ind
import oracle_lib as O

# Counters that no input can move (counted by the oracle all the same, and asserted to stay at 0), each with its argument:
UNREACHABLE = {
    # after the clamp every vertex lies in [0, w - 1] x [0, h - 1] (NaN and -Inf became +0, +Inf the limit), and rounding to nearest keeps
    # an integer interval: bx = min >= 0, bx + bw = max + 1 <= w, bw = max - min + 1 >= 1; the same for y.  w, h >= 1 for any image.
    "icon_box_degenerate": "the clamped, rounded vertices span a non-empty box inside the image",
    # `if (sx + 1 >= sw) { ... if (sx >= sw - 1)`: the two conditions are the same inequality on integers
    "icon_resize_edge_not_clamped": "sx >= sw - 1 is sx + 1 >= sw",
    # In exact arithmetic the inverted map sends (x, y) of the box to p1 + (x / bw)(p2 - p1) + (y / bh)(p0 - p1) with p0, p1, p2 inside the
    # box: within three box sides of it, below 3 * 4096 < 32768.  The computed map keeps that: float32 vertices within a side L make a
    # non-zero doubled triangle area A >= L * ulp(L) = L^2 2^-23, the double LU loses a factor L^2 / A <= 2^23 of its 2^-53 and the
    # determinant's cancellation the same again -- 2^-7 at worst, an inverse within 1 % of the exact one.  (A singular exit gives M = 0: sx = 0.)
    # The near-collinear cases, one ulp off a line, are in the list.
    "icon_warp_sx_saturated_high": "source coordinates stay within three box sides of the box",
    "icon_warp_sx_saturated_low": "as above",
    "icon_warp_sy_saturated_high": "as above",
    "icon_warp_sy_saturated_low": "as above",
    # the four weights are non-negative and sum to 2^15, the taps are bytes: 0 <= (sum + 2^14) >> 15 <= 255
    "icon_warp_v_below": "a convex combination of bytes", "icon_warp_v_above": "a convex combination of bytes",
    # a0 + a1 = b0 + b1 = 2048 with both non-negative (fx, fy in [0, 1): the two roundings of t * 2048 and (1 - t) * 2048 are complementary,
    # halves included, because 2048 is even); r <= 255 * 2048, r >> 4 <= 32640, (2048 * 32640) >> 16 = 1020, (1020 + 2) >> 2 = 255
    "icon_resize_v_below": "non-negative coefficients", "icon_resize_v_above": "coefficients sum to 2048",
    # sy = floor((dy + 0.5) * sh / 20 - 0.5): at least floor(0.5 * sh / 20 - 0.5) >= -1, at most floor(19.5 * sh / 20 - 0.5) <= sh - 1
    "icon_resize_sy0_high": "sy <= sh - 1", "icon_resize_sy1_low": "sy + 1 >= 0",
    # the system is two copies of the 3 x 3 block B = [x y 1] (rows 0, 2, 4 act on columns 0..2, rows 1, 3, 5 on columns 3..5).  Columns 0..2
    # never pick a row of the second copy (its entries there are 0 and the search wants a strictly larger one) and eliminate with alpha = 0
    # on them, so the second copy reaches columns 3..5 untouched and meets the same magnitudes the first copy met: it is singular exactly
    # when the first was, and that left through columns 0..2
    "icon_lu_col3_singular": "the second copy of the 3 x 3 block repeats the first", "icon_lu_col4_singular": "as column 3",
    "icon_lu_col5_singular": "as column 3",
    # row 1 is [0 0 0 x y 1]; column 0 swaps row 0 with row 0, 2 or 4 and adds nothing to row 1 (alpha = 0), so at column 1 the diagonal entry
    # is an exact 0: either a row below holds something strictly larger (swap) or the column is all zero (singular)
    "icon_lu_col1_no_swap": "the diagonal entry of column 1 is an exact zero",
    # column 5 is the last: rows i + 1 .. 5 are none, k stays i
    "icon_lu_col5_swap": "no row below the last",
}


def icon_names():
    names = O.icon_census_names()
    assert all(k.startswith(("icon_", "vote_")) for k in names) and not any(k.startswith(("icon_", "vote_")) for k in O.census_names())
    return names


@pytest.fixture(scope="module")
def scenes():
    O.set_math_mode(0)
    return [("frame", K.frame(), K.icon_cases(K.W, K.H))] + [("window%d" % k, K.window(k), K.icon_cases(K.WIN_W, K.WIN_H)) for k in (0, 2)]


@pytest.fixture(scope="module")
def oracle_runs(scenes):
    """(census of the whole list, {(scene, case): (icon image, clamped vertices, rc)})"""
    O.icon_census()
    out = {}
    for sname, img, cases in scenes:
        for name, q in cases:
            out[(sname, name)] = O.affine_correction(img, q)
    return O.icon_census(), out


@pytest.fixture(scope="module")
def vote_census():
    O.icon_census()
    got = []
    for name, wts, rho, labels, n_class, row, _ in K.vote_cases():
        x = row.astype(np.float32)
        got.append(O.lib().orc_svm_predict(O._p(x), K.ROW, O._p(wts), O._p(rho), O._p(labels), n_class))
    return O.icon_census(), got


def test_unreachable_names_exist():
    assert set(UNREACHABLE) <= set(icon_names())


def test_census_reaches_every_icon_branch(oracle_runs):
    cen, _ = oracle_runs
    own = [k for k in icon_names() if k.startswith("icon_")]
    print({k: cen[k] for k in own})
    missing = [k for k in own if cen[k] == 0 and k not in UNREACHABLE]
    assert not missing, missing
    taken = [k for k in UNREACHABLE if k.startswith("icon_") and cen[k] != 0]
    assert not taken, taken


def test_census_reaches_every_vote_branch(vote_census):
    cen, _ = vote_census
    own = [k for k in icon_names() if k.startswith("vote_")]
    print({k: cen[k] for k in own})
    missing = [k for k in own if cen[k] == 0 and k not in UNREACHABLE]
    assert not missing, missing


def test_second_opinion_agrees_on_every_case(scenes, oracle_runs):
    _, runs = oracle_runs
    n = 0
    for sname, img, cases in scenes:
        for name, q in cases:
            a, ia, ra = runs[(sname, name)]
            b, ib, rb = ind.affine_correction(img, q)
            assert ra == rb, (sname, name)
            assert ia.tobytes() == ib.tobytes(), (sname, name, ia.tolist(), ib.tolist())
            assert a.tobytes() == b.tobytes(), (sname, name)
            n += 1
    assert n >= 3 * (len(K.named_icons(K.W, K.H)) + 6 * K.FAMILY)


def test_clamp_is_the_transcribed_one(scenes, oracle_runs):
    import harvest_ref
    _, runs = oracle_runs
    changed = 0
    for sname, img, cases in scenes:
        h, w, _ = img.shape
        for name, q in cases:
            want = K.clamp_transcribed(q, w, h)
            assert runs[(sname, name)][1].tobytes() == want.tobytes(), (sname, name)
            assert harvest_ref.clamp_icon(q, w, h).tobytes() == want.tobytes(), (sname, name)
            assert not np.isnan(want).any() and not np.signbit(want).any() and (want[:, 0] <= w - 1).all() and (want[:, 1] <= h - 1).all()
            changed += want.tobytes() != q.tobytes()
    assert changed > 100


def test_vote_cases_equal_the_restatement(vote_census):
    _, got = vote_census
    seen = set()
    for (name, wts, rho, labels, n_class, row, _), g in zip(K.vote_cases(), got):
        want, votes = K.vote(wts, rho, labels, n_class, row)
        assert g == want, (name, votes)
        top = max(votes)
        if name.startswith("winner_"):
            assert votes.index(top) == int(name[-1]) and votes.count(top) == 1
        if name.startswith("tie_all"):
            assert votes.count(top) == n_class and want == labels[0]
        if name.startswith("tie_two"):
            assert votes.count(top) == 2
        seen.add(votes.index(top))
    assert seen == set(range(8))


def test_edge_vote_cases_sit_on_the_last_bit():
    """rho at kval: every sum is exactly 0 and votes j; one double below: every sum > 0 and votes i -- the two give different labels"""
    by = {c[0]: c for c in K.vote_cases()}
    n = 0
    for name, c in by.items():
        if name.endswith("_at"):
            lo, hi = by[name[:-3] + "_below"], by[name[:-3] + "_above"]
            k = K.kvals(c[1], c[5]).astype(np.float64)
            assert (-c[2] + k == 0).all() and (-lo[2] + k > 0).all() and (-hi[2] + k < 0).all()
            assert np.abs(np.log2(np.abs(c[1][c[1] != 0]))).max() > 19                   # the dynamic range is there
            assert K.vote(*c[1:6])[0] == K.vote(*hi[1:6])[0] == c[3][-1] and K.vote(*lo[1:6])[0] == c[3][0]
            n += 1
    assert n == len(K.ROW_SOURCES) * 3


def test_named_findings(scenes, oracle_runs):
    _, runs = oracle_runs
    sname, img, cases = scenes[0]
    by = dict(cases)
    # a collinear icon (and a point): a non-empty box, a singular system, M = 0: every output pixel is the ROI's pixel (0, 0)
    for name in ("collinear_horizontal", "collinear_vertical", "collinear_diagonal", "collinear_diagonal_fractional", "point", "point_fractional",
                 "outside_left", "outside_above"):
        out, ic, rc = runs[(sname, name)]
        pi = np.rint(ic.astype(np.float64)).astype(int)
        bx, by_ = pi[:, 0].min(), pi[:, 1].min()
        assert rc == 0 and (out == img[by_, bx]).all(), name
    assert runs[(sname, "collinear_diagonal")][0].any()                                  # ... which is not a zero image
    # one ulp off the line the system is regular again
    assert any(len(np.unique(runs[(sname, "near_collinear_%s_%s" % (a, b))][0].reshape(-1, 3), axis=0)) > 1 for a in "xy" for b in ("up", "down"))
    # NaN -> +0, -0 -> +0, +Inf -> the limit, -Inf -> +0, in bits
    _, ic, rc = runs[(sname, "probe_nan_inf")]
    assert rc == 0 and ic.tobytes() == np.array([[0, 50], [30, K.H - 1], [0, 10], [60, 60]], np.float32).tobytes()
    assert runs[(sname, "all_nan")][1].tobytes() == np.zeros((4, 2), np.float32).tobytes()
    assert runs[(sname, "all_minus_zero")][1].tobytes() == np.zeros((4, 2), np.float32).tobytes()
    assert by["all_minus_zero"].tobytes() != np.zeros((4, 2), np.float32).tobytes()
    # round half to even decides the box: the oracle's icon is the one cut from box 10, 12, 11 x 9 by hand (10.5 -> 10, 11.5 -> 12, 20.5 -> 20)
    out, ic, rc = runs[(sname, "half_corners_round_to_even")]
    bx, by_, bw, bh = 10, 12, 11, 9
    src = [(float(ic[i, 0]) - bx, float(ic[i, 1]) - by_) for i in (1, 2, 0)]
    m = ind.get_affine_transform(src, [(0.0, 0.0), (float(bw), 0.0), (0.0, float(bh))])
    by_hand = ind.resize_to(ind.warp_affine_same_size(img[by_:by_ + bh, bx:bx + bw], m), 20, 20)
    assert rc == 0 and np.array_equal(out, by_hand)
    for other in ((10, 11, 11, 10), (11, 12, 10, 9), (10, 12, 12, 10)):                   # ... and not from a box rounded another way
        ox, oy, ow, oh = other
        src = [(float(ic[i, 0]) - ox, float(ic[i, 1]) - oy) for i in (1, 2, 0)]
        m = ind.get_affine_transform(src, [(0.0, 0.0), (float(ow), 0.0), (0.0, float(oh))])
        assert not np.array_equal(out, ind.resize_to(ind.warp_affine_same_size(img[oy:oy + oh, ox:ox + ow], m), 20, 20)), other


def test_split_gives_different_mixes():
    n = len(K.icon_cases(K.W, K.H))
    parts = K.split(n, 8)
    assert len({p.stop - p.start for p in parts}) >= 3 and all(p.stop - p.start >= 9 for p in parts) and parts[-1].stop == n


def test_tail_scene_clamps_on_all_four_sides():
    """the scene the fused tail is given (tests/test_gpu_icon_cases.py): its detected armours' icons leave the frame on every side"""
    from rmcv_amd import synth
    O.set_math_mode(0)
    img = K.tail_scene()
    arm = O.detect_frame(img)["armours"]
    assert len(arm) == len(K.TAIL_PAIRS)
    _, after, icons = O.classify_armours(img, arm, synth.svm_weights())
    assert K.sides_clamped(arm["icon"], after["icon"], K.TAIL_W, K.TAIL_H) == (True, True, True, True)
    assert len({i.tobytes() for i in icons}) == len(arm)


def test_pivot_ties_tell_first_maximum_from_last(monkeypatch):
    """the pivot search takes the first of equal magnitudes: on the scene itself, taking the last changes bytes of every pivot_tie icon"""
    import functools
    named = dict(K.named_icons(K.W, K.H))
    first = [ind.affine_correction(K.frame(), named["pivot_tie_%d" % k])[0] for k in range(len(K.PIVOT_TIES))]
    monkeypatch.setattr(ind, "lu_solve", functools.partial(ind.lu_solve, last_maximum=True))
    last = [ind.affine_correction(K.frame(), named["pivot_tie_%d" % k])[0] for k in range(len(K.PIVOT_TIES))]
    assert all(not np.array_equal(a, b) for a, b in zip(first, last))
    assert [n for n, _ in K.icon_cases(K.W, K.H)[:len(K.PIVOT_TIES)]] == ["pivot_tie_%d" % k for k in range(len(K.PIVOT_TIES))]
