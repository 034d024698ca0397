"""The pose stage's case list (tests/pose_cases.py) on the CPU:

* the oracle's pose census (oracle/rmcv_oracle_pnp.c: ORC_CENSUS_POSE) over the list reaches every counter, or the counter is listed in UNREACHABLE
  with its argument (or in NO_INPUT_KNOWN with the families searched) and is then asserted to stay at 0;
* the undistortion of every point of every case is the mpmath restatement's (tests/pose_ref.py) to one float32 ulp, the give-up decision the same;
* on the well-posed families both IPPE candidates, the pose taken, tvec and the rotation of rvec are the restatement's, started from the
  oracle's own narrowed points, within four times the error measured (constants below, DESIGN.md pose section);
* on every case the rc and every decision of the census agree with the restatement wherever its deciding quantity is outside its band;
* what reading and running the code found is asserted in raw bits (test_named_findings);
* counting and tracing change no bit."""
import collections
import math

import mpmath as mpm
import numpy as np
import pytest
from mpmath import mpf

import oracle_lib as O
import pose_cases as K
import pose_ref as P

# Counters that no input can move (counted all the same, asserted to stay at 0), each with its argument:
UNREACHABLE = {
    # rotate_vec_to_z is only ever given v = (p, q, 1): c = 1 / |v| is positive, or NaN when p or q is (then the comparison is false), so
    # |1 + c| >= 1 is never below DBL_EPSILON.  (|v| = inf gives c = 0.)
    "pose_antipode": "the vector is (p, q, 1): its normalised z is positive or NaN, 1 + c never below DBL_EPSILON",
}
# ... and the one counter for which neither an input nor a proof is known.  A NaN error needs a NaN X z or Y z in reproj_error (the image points
# are finite there: a NaN or Inf one leaves at den or at gamma2; sums of squares cannot cancel).  R is finite and bounded once gamma passed, so
# that needs a non-finite t, i.e. a computed normal-equation determinant 16 S(x^2 + y^2) - 4 (S x)^2 - 4 (S y)^2 of exactly 0 with distinct
# points.  Its exact value is at least 2^-46 M^2 for float32 points of magnitude M, the rounding of its terms up to about 2^-43 M^2: the crude
# bound does not exclude the cancellation, and no input was found.  Searched: every pair of coordinates set to NaN, +-Inf, +-FLT_MAX, 1e20 ..
# 3e38 on five configurations; 300 000 seeded quadrilaterals of huge (1e4 .. 1e38) coordinates 0 .. 4095 ulps apart; 360 000 near-frontal and
# in-plane poses; 100 000 one-to-eight-ulp neighbours of centred squares in every roll; squares one to a thousand ulps wide at 1e10 .. 3e38.
# (Z == 0, for which the list was meant, HAS inputs: a single +-FLT_MAX coordinate, cases fltmax_at_* -- it is covered.)
NO_INPUT_KNOWN = {"pose_ea_nan": "needs the translation's 3 x 3 determinant to cancel to an exact zero on distinct points"}

# Measured against pose_ref at 240 bits on this list (seed pose_cases.SEED), worst per family; every tolerance is four times its measurement.
#   family      tvec, norm-wise relative    candidate rotations, elementwise absolute, where b > 0.05    matrix of rvec times sin(theta), less COND
#   projected   7.8e-12                     3.7e-15                                                      <= 0 (COND covers it)
#   detector    7.9e-13                     3.5e-15                                                      <= 0
#   roll        1.3e-14                     3.3e-15                                                      2.7e-13
TOL_T = {"projected": 3.2e-11, "detector": 3.2e-12, "roll": 5.2e-14}
TOL_R = {"projected": 1.5e-14, "detector": 1.4e-14, "roll": 1.4e-14}
TOL_RVEC = {"projected": 1.5e-14, "detector": 1.4e-14, "roll": 1.1e-12}
# COND, the conditioning of the construction, computed per case from the mp values: b = sqrt(1 - |column|^2), and the 1 - ... is exact to a few
# ulps of 1 (B_SQ_ERROR), so b is exact to min(sqrt(D), D / 2 b).  At the frontal pose, where b = 0, that is 4.2e-8 and it is the whole error
# of the rotation (measured there: 2.1e-8; 4.8e-14 at b = 0.0011); it falls below 2e-14 once b > 0.05.  A candidate is held to TOL_R + COND.
B_SQ_ERROR = 8 * 2.0 ** -52
# rot2vec takes theta from acos and multiplies R - R^T by theta / (2 sin theta): the matrix of the returned rvec is held to
# (TOL_RVEC + COND) / sin(theta).  Within 1e-3 of pi nothing is promised (test_named_findings pins what comes out there); below FLT_EPSILON
# rvec = 0 by the reference's own rule, an error of at most FLT_EPSILON.
TOL_ORDER_BAND = 1e-4          # the two float32 error sums decide the order inside this relative band of the mp errors
MAX_EXCUSED_ORDER = 0.05       # measured: 3 of 800 well-posed cases (0.4 %) take the other pose inside the band; 101 of 800 (12.6 %) lie inside it at all
MAX_DOUBLE_ROUNDING = 0.01     # measured: 0 of 14 592 undistorted coordinates differ from the correctly rounded float32
FLT_EPSILON = 2.0 ** -23
DBL_EPSILON = 2.0 ** -52
WELL_CONDITIONED = 1e6         # wild cases: decisions behind the homography are compared when (1 + max |q|)^2 / |den| is below this


def pose_names():
    names = O.pose_census_names()
    assert all(k.startswith("pose_") for k in names)
    assert not any(k.startswith("pose_") for k in O.census_names() + O.icon_census_names())
    return names


@pytest.fixture(scope="module")
def cfgs():
    O.set_math_mode(0)
    return {n: K.to_oracle_cfg(O, c) for n, c in K.configs().items()}


@pytest.fixture(scope="module")
def runs(cfgs):
    """(census of the whole list, {case name: (rc, rvec, tvec, trace, census of the case alone)})"""
    O.pose_census()
    total, out = collections.Counter(), {}
    for name, cfg, q, _ in K.cases():
        rc, r, t, tr = O.solve_pnp_trace(q, cfgs[cfg])
        cen = O.pose_census()
        total.update(cen)
        out[name] = (rc, r, t, tr, cen)
    return dict(total), out


@pytest.fixture(scope="module")
def mp_runs(runs):
    """{case name: pose_ref.solve from the oracle's own narrowed points} for every case whose narrowed points are finite"""
    vals = {n: P.config_values(c) for n, c in K.configs().items()}
    out = {}
    for name, cfg, _, _ in K.cases():
        img = runs[1][name][3]["img"]
        if np.isfinite(img).all():
            out[name] = P.solve([(P.M(img[2 * i]), P.M(img[2 * i + 1])) for i in range(4)], vals[cfg][2])
    return out


def test_unreachable_names_exist():
    assert set(UNREACHABLE) | set(NO_INPUT_KNOWN) <= set(pose_names()) and not set(UNREACHABLE) & set(NO_INPUT_KNOWN)
    assert len(NO_INPUT_KNOWN) <= 1


def test_list_is_a_couple_of_thousand_named_cases():
    cases = K.cases()
    assert 1500 <= len(cases) <= 2500 and len({c[0] for c in cases}) == len(cases)
    assert {c[1] for c in cases} == set(K.configs())
    assert all(c[2].dtype == np.float32 and c[2].shape == (4, 2) for c in cases)


def test_census_reaches_every_pose_branch(runs):
    cen, _ = runs
    print(cen)
    missing = [k for k in pose_names() if cen[k] == 0 and k not in UNREACHABLE and k not in NO_INPUT_KNOWN]
    assert not missing, missing
    taken = [k for k in list(UNREACHABLE) + list(NO_INPUT_KNOWN) if cen[k] != 0]
    assert not taken, taken


def test_every_configuration_meets_its_own_branch(runs):
    """... in cases of its own (the camera-table route gives every configuration a frame of them)"""
    per = collections.defaultdict(collections.Counter)
    for name, cfg, _, _ in K.cases():
        per[cfg].update(runs[1][name][4])
    assert per["icdist"]["pose_icdist_negative"] and per["pow2"]["pose_b0sq_clamped"] and per["pow2"]["pose_w_norm_below_eps"]
    assert per["pow2"]["pose_w_norm_nan"] and per["pow2"]["pose_ea_equal"] and per["fx0"]["pose_den_not_positive"] == len(K.by_config()["fx0"])
    for name in ("sq_zero", "sq_zero_w", "sq_tiny", "sq_inf", "sq_nan"):
        assert per[name]["pose_gamma2_exit"] == len(K.by_config()[name]), name
    for name in ("sq_huge20", "sq_huge30", "sq_huge38"):
        assert per[name]["pose_gamma_exit"] + per[name]["pose_den_not_positive"] == len(K.by_config()[name]) and per[name]["pose_gamma_exit"], name
    assert per["k1_huge"]["pose_den_not_positive"] == len(K.by_config()["k1_huge"]) and per["k1_huge"]["pose_undistort_abandoned"] == 0
    for name in ("default", "other", "sq_negative", "sq_mixed"):
        assert per[name]["pose_ea_greater"] and per[name]["pose_ea_less"] and per[name]["pose_sp_negative"] and per[name]["pose_sp_not_negative"], name


def test_counting_and_tracing_change_nothing(cfgs, runs):
    for name, cfg, q, _ in K.cases():
        rc, r, t = O.solve_pnp(q, cfgs[cfg])
        trc, tr, tt, _, _ = runs[1][name]
        assert rc == trc and r.tobytes() == tr.tobytes() and t.tobytes() == tt.tobytes(), name


def ulp32(x):
    return mpf(2) ** max(mpm.frexp(x)[1] - 24, -149) if x != 0 else mpf(2) ** -149


def test_undistortion_against_mp(cfgs):
    vals = {n: P.config_values(c) for n, c in K.configs().items()}
    n = off = decided = gave_up = 0
    for name, cfg, q, _ in K.cases():
        Kc, dist, _ = vals[cfg]
        for i in range(4):
            u, v = q[i]
            if not (np.isfinite(u) and np.isfinite(v)):
                continue
            x, y, gave, seen = P.undistort(P.M(u), P.M(v), Kc, dist)
            O.pose_census()
            ox, oy = O.undistort_point(u, v, cfgs[cfg])
            cen = O.pose_census()
            if seen and all(abs(s) > mpf(10) ** -12 for s in seen) and mpm.isfinite(x):    # (1 / radial is never near 0 unless radial is huge)
                assert bool(cen["pose_undistort_abandoned"]) == gave, (name, i)
                assert cen["pose_icdist_not_negative"] == len(seen) - gave, (name, i)
                decided += 1
                gave_up += gave
            if not (mpm.isfinite(x) and mpm.isfinite(y)):
                continue
            for got, want in ((ox, x), (oy, y)):
                w32 = P.to_f32(want)
                if not mpm.isfinite(w32):
                    assert not np.isfinite(got), (name, i)
                    continue
                n += 1
                if P.M(got) != w32:
                    off += 1
                    assert abs(P.M(got) - w32) <= ulp32(w32), (name, i, got, float(w32))
    print("undistorted coordinates %d, not the correctly rounded value %d, give-up decisions compared %d (gave up: %d)" % (n, off, decided, gave_up))
    assert n > 12000 and decided > 6000 and gave_up > 100
    assert off <= MAX_DOUBLE_ROUNDING * n


def rel_t(t, tm):
    return mpm.sqrt(sum((P.M(t[i]) - tm[i]) ** 2 for i in range(3))) / mpm.sqrt(sum(c ** 2 for c in tm))


def abs_R(R, Rm):
    return max(abs(P.M(R[i][j]) - Rm[i, j]) for i in range(3) for j in range(3))


def test_ippe_against_mp_on_the_well_posed_families(runs, mp_runs):
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    n = excused = near = rvecs = 0
    for name, cfg, _, fam in K.cases():
        if fam not in K.WELL_POSED:
            continue
        rc, r, t, tr, _ = runs[1][name]
        m = mp_runs[name]
        assert rc == 0 == m["rc"], name
        bmin = mpm.sqrt(max(min(m["b0sq"], m["b1sq"]), mpf(0)))
        cond = min(math.sqrt(B_SQ_ERROR), B_SQ_ERROR / (2 * float(bmin))) if bmin > 0 else math.sqrt(B_SQ_ERROR)
        # the two candidates, in the reference's order (b0 >= 0 first) or, where b0 = b1 = 0 makes them one pose, in either
        errs = []
        for perm in ((0, 1), (1, 0)):
            eR = max(abs_R(tr["R" + a].reshape(3, 3), m["R"][b]) for a, b in zip("ab", perm))
            eT = max(rel_t(tr["t" + a], m["t"][b]) for a, b in zip("ab", perm))
            errs.append((float(eR), float(eT)))
        eR, eT = min(errs)
        if bmin > 0.05:                                                              # (measured where the conditioning term is below 2e-14)
            worst[fam]["candidate R"] = max(worst[fam]["candidate R"], eR)
        worst[fam]["candidate t"] = max(worst[fam]["candidate t"], eT)
        assert eR <= TOL_R[fam] + cond and eT <= TOL_T[fam], (name, eR, eT, cond)
        # the pose taken
        big = max(m["err"])
        rel = abs(m["err"][0] - m["err"][1]) / big if big > 0 else mpf(0)
        taken = int(tr["taken"])
        n += 1
        near += rel < TOL_ORDER_BAND
        if taken != m["taken"]:
            assert rel < TOL_ORDER_BAND, (name, float(rel), tr["ea"], tr["eb"])
            excused += 1
        Rm, tm = m["R"][taken], m["t"][taken]
        eT = float(rel_t(t, tm))
        worst[fam]["tvec"] = max(worst[fam]["tvec"], eT)
        assert eT <= TOL_T[fam], (name, eT)
        angle = P.rotation_angle(Rm)
        if mpm.pi - angle <= mpf(10) ** -3:
            continue
        rvecs += 1
        eR = float(abs_R(P.rodrigues(r).tolist(), Rm))
        if angle < FLT_EPSILON / 2:                                                  # the reference's own rule: rvec = 0 there
            assert eR <= FLT_EPSILON + cond, (name, eR)
        else:
            s = float(mpm.sin(angle))
            worst[fam]["rvec R x sin"] = max(worst[fam]["rvec R x sin"], eR * s - cond)
            assert eR <= (TOL_RVEC[fam] + cond) / s, (name, eR, s)
    print({k: dict(v) for k, v in worst.items()})
    print("well-posed cases %d, inside the order band %d (%.1f %%), of them taking the other pose %d (%.2f %%), rvec compared %d"
          % (n, near, 100.0 * near / n, excused, 100.0 * excused / n, rvecs))
    assert n >= 700 and rvecs >= 650
    assert excused <= MAX_EXCUSED_ORDER * n


def test_decisions_agree_with_mp_on_every_case(runs, mp_runs):
    """rc and census, decision by decision, wherever the restatement's deciding quantity is outside its band"""
    seen = collections.Counter()
    for name, cfg, _, fam in K.cases():
        rc, r, t, tr, cen = runs[1][name]
        img = tr["img"]
        if not np.isfinite(img).all():                                               # a NaN or Inf point: nothing to solve
            # an Inf point can give den = +-Inf, which passes; then the homography is NaN and gamma2 leaves
            assert rc == 1 and (cen["pose_den_not_positive"] or cen["pose_gamma2_exit"]), name
            seen["not finite"] += 1
            continue
        m = mp_runs[name]
        x = [P.M(c) for c in img]
        terms = abs((x[2] - x[4]) * (x[7] - x[5])) + abs((x[6] - x[4]) * (x[3] - x[5]))
        den = m["den"]
        if den == 0 or abs(den) > mpf(2) ** -50 * terms:
            assert bool(cen["pose_den_positive"]) == (den != 0), name
            seen["den"] += 1
        if den == 0 or not cen["pose_den_positive"]:
            assert rc == 1 or abs(den) <= mpf(2) ** -50 * terms, name
            continue
        if "gamma" not in m:                                                         # a plate with no side (zero, NaN, Inf in float32)
            assert rc == 1 and (cen["pose_gamma2_exit"] or cen["pose_gamma_exit"]), name
            seen["no side"] += 1
            continue
        kappa = (1 + max(abs(c) for c in x)) ** 2 / abs(den)
        if kappa > WELL_CONDITIONED:
            seen["ill-conditioned"] += 1
            continue
        gamma = m["gamma"]
        assert cen["pose_gamma2_ok"] == 1, name
        if abs(gamma / DBL_EPSILON - 1) > mpf(10) ** -6:
            assert bool(cen["pose_gamma_exit"]) == (gamma < DBL_EPSILON), name
            seen["gamma"] += 1
        if gamma < DBL_EPSILON or cen["pose_gamma_exit"]:
            assert rc == 1, name
            continue
        assert rc == 0 == m["rc"], name
        for key, counter in (("b0sq", "pose_b0sq_positive"), ("b1sq", "pose_b1sq_positive")):
            if abs(m[key]) > mpf(10) ** -7:
                assert bool(cen[counter]) == (m[key] > 0), (name, key)
                seen[key] += 1
        if abs(m["sp"]) > mpf(10) ** -7:
            assert bool(cen["pose_sp_negative"]) == (m["sp"] < 0), name
            seen["sp"] += 1
        # the errors are float32: each residual is the difference of two values rounded to float32, exact to 2 ulps of the largest coordinate
        big, quantum = max(m["err"]), 4 * mpf(2) ** -24 * max(abs(c) for c in x)
        if big > 0 and abs(m["err"][0] - m["err"][1]) >= TOL_ORDER_BAND * big + quantum:
            assert bool(cen["pose_ea_greater"]) == (m["err"][0] > m["err"][1]) and not cen["pose_ea_equal"] and not cen["pose_ea_nan"], name
            seen["order"] += 1
        depth_scale = max(abs(c) for tt in m["t"] for c in tt)
        if all(abs(z) > mpf(10) ** -9 * depth_scale for d in m["depths"] for z in d):
            assert cen["pose_z_zero"] == 0 and cen["pose_z_nonzero"] == 8, name
            seen["depth"] += 1
        angle = P.rotation_angle(m["R"][int(tr["taken"])])
        if abs(angle - FLT_EPSILON) > 0.6 * FLT_EPSILON and mpm.pi - angle > mpf(10) ** -7:
            assert bool(cen["pose_w_norm_below_eps"]) == (angle < FLT_EPSILON) and not cen["pose_w_norm_nan"], name
            seen["angle"] += 1
    print(dict(seen))
    assert seen["den"] > 1500 and seen["order"] > 1000 and seen["angle"] > 1000 and seen["b0sq"] > 1000 and seen["gamma"] > 1200
    assert seen["not finite"] > 50 and seen["no side"] >= 5 * 8


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def test_named_findings(cfgs, runs):
    by = runs[1]
    zero3 = bits(np.zeros(3))
    half_pi = math.pi / 2
    for s in K.CENTRED_HALVES:
        z = 1024.0 * 13.5 / s
        # roll 0 is the frontal pose through the w_norm < eps branch; rolls 1 and 3 are quarter turns
        assert by["centred_%d_roll0" % s][4]["pose_w_norm_below_eps"] == 1
        assert bits(by["centred_%d_roll0" % s][1]) == zero3
        assert bits(by["centred_%d_roll1" % s][1]) == bits([0.0, 0.0, -half_pi]) and bits(by["centred_%d_roll3" % s][1]) == bits([0.0, 0.0, half_pi])
        # roll 2 and the reversed order are rotations by pi -- and come out as rvec = 0: R - R^T is an exact zero matrix, whatever theta / 2 sin theta
        for which in ("roll2", "reversed"):
            rc, r, t, tr, cen = by["centred_%d_%s" % (s, which)]
            assert rc == 0 and bits(r) == zero3 and cen["pose_w_norm_not_below"] == 1, (s, which)
            R = tr["Ra" if tr["taken"] == 0 else "Rb"]
            assert R[0] + R[4] + R[8] == -1.0, (s, which)
        for which in ("roll0", "roll1", "roll2", "roll3", "reversed"):               # every order clamps both b and ties the two errors
            rc, r, t, tr, cen = by["centred_%d_%s" % (s, which)]
            assert cen["pose_b0sq_clamped"] == cen["pose_b1sq_clamped"] == cen["pose_ea_equal"] == 1 and bits(t) == bits([0.0, 0.0, z]), (s, which)
    # one ulp beside a rotation by pi the trace can fall below -1: acos gives NaN and so does every component of rvec (tvec stays finite)
    hit = [n for n in ("near_pi_nan_0", "near_pi_nan_1") if by[n][4]["pose_w_norm_nan"]]
    assert hit == ["near_pi_nan_0", "near_pi_nan_1"]
    for n in hit:
        rc, r, t, _, _ = by[n]
        assert rc == 0 and np.isnan(r).all() and np.isfinite(t).all() and t[2] > 0
    # rc 1 with zero vectors for each degenerate configuration, whatever the vertices
    for cfg in K.DEGENERATE_SQUARES + ("fx0", "k1_huge"):
        for i in K.by_config()[cfg]:
            rc, r, t, _, _ = by[K.cases()[i][0]]
            assert rc == 1 and bits(r) == zero3 and bits(t) == zero3, K.cases()[i][0]
    # ... and for a NaN or Inf vertex, coincident points, collinear points without distortion
    for n in ("nan_at_0x_default", "pinf_at_2y_pow2", "ninf_all_default", "nan_all_pow2", "coincident_all_default", "coincident_two_pairs_other",
              "collinear_horizontal_pow2", "collinear_vertical_pow2", "collinear_diagonal_pow2", "collinear_diagonal_fractional_pow2"):
        rc, r, t, _, cen = by[n]
        assert rc == 1 and bits(r) == zero3 and bits(t) == zero3 and cen["pose_den_not_positive"] == 1, n
    # collinear pixels under distortion are NOT degenerate: rc 0 and a pose that means nothing
    for n in ("collinear_diagonal_default", "collinear_diagonal_other", "collinear_horizontal_default", "collinear_vertical_other"):
        rc, r, t, _, _ = by[n]
        assert rc == 0 and np.isfinite(r).all() and np.isfinite(t).all() and np.any(t != 0), n
    assert abs(by["collinear_diagonal_default"][2][2]) < 1000                        # (a plate a few hundred millimetres from the lens)
    # -0 and denormal vertices are ordinary numbers
    assert by["nzero_at_0x_default"][0] == 0 and by["denormal_all_default"][0] == 1 and by["nzero_all_pow2"][0] == 1
    # huge vertices: rc 0 and finite vectors
    for n in ("huge_vertices_plus", "huge_vertices_scaled_square"):
        rc, r, t, _, _ = by[n]
        assert rc == 0 and np.isfinite(r).all() and np.isfinite(t).all(), n
    # a single +-FLT_MAX coordinate reaches Z == 0 in the reprojection
    assert by["fltmax_at_0x_default"][4]["pose_z_zero"] and by["nfltmax_at_1x_pow2"][4]["pose_z_zero"]
    # a mirrored plate, square = (27, -27): the homography is still the canonical square's, the translation's points are mirrored -- the same
    # pixels take the other candidate than under (27, 27), and (-27, -27) the same one
    rc, r, t, tr = O.solve_pnp_trace(K.sq(600, 500, 660, 560), cfgs["default"])
    assert (by["plate_sq_mixed_detector"][3]["taken"], by["plate_sq_negative_detector"][3]["taken"], tr["taken"]) == (1.0, 0.0, 0.0)
    assert by["plate_sq_mixed_detector"][0] == 0 and bits(by["plate_sq_mixed_detector"][3]["Ra"]) == bits(tr["Ra"])
    # the point the icdist case is named for: all four points give up in the first round and keep their undistorted guess
    cen = by["icdist_all_four_give_up"][4]
    assert cen["pose_icdist_negative"] == 4 and cen["pose_icdist_not_negative"] == 0 and by["icdist_all_four_give_up"][0] == 0
