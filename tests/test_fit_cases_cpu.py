"""The contour cases of tests/fit_cases.py on the CPU oracle: every case reaches the branch of the fit it is named for (the oracle's branch
census), the cases of the 2^24 branch have the coordinate sums they claim, and -- accuracy, against the independent 50-digit reference
tests/fit_ref.py -- every case that takes the direct solution agrees with Fitzgibbon's constrained fit solved at 50 digits, per field, within
4 x the deviation of a float64 numpy solution of the same problem plus one float32 ulp.
    Measured (float32 ulps, worst case per field: oracle vs 50 digits / the tolerance that applied there):
        cx 0.44 / 1.00   cy 0.48 / 1.00   w 0.49 / 1.00   h 0.48 / 1.00   angle 0.41 / 1.00
    (first-attempt direct solutions; a jittered attempt solves a perturbed problem and is compared with the device only)"""
import numpy as np
import pytest

import fit_cases as F
import fit_ref as R
import oracle_lib as O

CASES = F.point_cases()
IMAGES = F.image_cases()


def _sum_kind(total):
    return "over" if total >= F.TWO24 else "under"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_point_case_reaches_its_branch(case):
    O.set_math_mode(0)
    assert len(case.pts) >= 6
    O.census()
    box, path = O.fit_ellipse_direct(case.pts)
    cen = O.census()
    assert path == case.path, (path, box)
    assert not [e for e in case.expect if cen[e] == 0], {k: v for k, v in cen.items() if v}
    sx, sy = int(case.pts["x"].astype(np.int64).sum()), int(case.pts["y"].astype(np.int64).sum())
    if case.sums is None:
        assert sx < F.TWO24 and sy < F.TWO24
    else:
        want = {"last_under": F.TWO24 - 1, "first_over": F.TWO24}
        for total, kind in ((sx, case.sums[0]), (sy, case.sums[1])):
            if kind in want:
                assert total == want[kind]
            else:
                assert _sum_kind(total) == kind
    assert int(case.pts["x"].min()) >= 0 and int(case.pts["y"].min()) >= 0   # what the entry points accept


def test_point_counts_sit_on_the_chunk_edges():
    by = {c.name: c for c in CASES}
    for n in F.COUNTS:
        assert len(by["general_n%d" % n].pts) == n
        if n < 2048:
            assert len(by["direct_first_n%d" % n].pts) == n
    assert max(F.COUNTS) > 2048 and {6, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= set(F.COUNTS)


def test_every_branch_of_the_whole_fit_is_reached():
    O.set_math_mode(0)
    O.census()
    for c in CASES:
        O.fit_ellipse_direct(c.pts)
    cen = O.census()
    for k in ("direct_attempt0", "direct_attempt1", "direct_none", "direct_bad_box", "general_fit", "general_jitter_retry", "general_no_retry",
              "centre_det_zero", "centre_det_nonzero", "general_swap", "general_no_swap", "direct_swap", "direct_no_swap"):
        assert cen[k] > 0, k
    # a good box after each attempt, a wild box after each attempt
    by = {c.name: c for c in CASES}
    assert by["direct_good_box_bar4"].path == 0 and by["direct_jittered_good_box"].path == 0
    assert by["direct_wild_box"].path == 1 and by["direct_jittered_two_rows"].path == 1


def test_degenerate_results_are_what_the_gates_must_pass_on():
    """zero width (ratio = inf) and 0 / 0 (ratio = NaN): with ratio_hi = +inf the first is a positive, the second a negative"""
    O.set_math_mode(0)
    by = {c.name: c for c in CASES}
    box, _ = O.fit_ellipse_direct(by["direct_none_collinear_horizontal"].pts)
    assert tuple(box) == (19.5, 50.0, 0.0, np.float32(0.0049972534), 0.0)
    box, _ = O.fit_ellipse_direct(by["direct_none_all_equal"].pts)
    assert box["w"] == 0 and box["h"] == 0
    pts = np.concatenate([by[n].pts for n in F.DEGENERATE])
    offs = np.cumsum([0] + [len(by[n].pts) for n in F.DEGENERATE]).astype(np.int32)
    p = O.default_params(ratio_lo=0.0, ratio_hi=float("inf"), area_lo=0.0, tilt_max=1e30)
    blobs, src, neg = O.filter_lightblobs(pts, offs, p)
    assert src.tolist() == [0, 2] and neg.tolist() == [1]


@pytest.mark.parametrize("case", IMAGES, ids=[c.name for c in IMAGES])
def test_image_case_reaches_its_branches(case):
    O.set_math_mode(0)
    O.census()
    ref = O.detect_frame(F.frame_of(case.mask), O.default_params(morph=O.MORPH_NONE, area_lo=0.0))
    cen = O.census()
    assert np.array_equal(ref["binary"], case.mask)
    assert not [e for e in case.expect if cen[e] == 0], {k: v for k, v in cen.items() if v}
    if case.name == "shapes":
        assert len(ref["blobs"]) >= 4 and len(ref["armours"]) >= 2          # blobs and armours, not just points
    if case.name == "comb_2p24":
        assert case.mask.shape == (1200, 1920) and len(ref["offs"]) == 2      # within the default limits: one border ...
        p = ref["pts"]
        assert len(p) == 15998 and len(p) <= 65536
        assert int(p["x"].astype(np.int64).sum()) == 30508186 >= F.TWO24 > int(p["y"].astype(np.int64).sum())


def test_direct_solutions_against_the_50_digit_fit():
    O.set_math_mode(0)
    worst = {f: (0.0, 0.0, None) for f in R.FIELDS}
    failures = []
    for c in CASES:
        if c.path != 0 or "direct_attempt0" not in c.expect:   # (a jittered attempt solves a perturbed problem: not this reference's)
            continue
        box, path = O.fit_ellipse_direct(c.pts)
        assert path == 0
        for f, v in R.field_errors(box, c.pts).items():
            if v is None:
                continue
            err, tol = v
            if not err <= worst[f][0]:
                worst[f] = (err, tol, c.name)
            if not err <= tol:
                failures.append((c.name, f, err, tol))
    print("worst float32 ulps per field (oracle vs 50 digits, tolerance, case):", worst)
    assert not failures, failures
