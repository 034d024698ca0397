"""The scalar tails of the ellipse fit on the CPU oracle, over the case lists of tests/fit_unit_cases.py (what tests/test_gpu_fit_units.py
then holds the device to, bit for bit):

* the oracle's branch census (oracle/rmcv_oracle.c: ORC_CENSUS) shows every branch of the eigen-solver (the device's eig3_orthes /
  eig3_step / eig3_backsub), direct_finish, jacobi_sym / normal_factor / normal_apply, general_centre and general_finish at least once
  -- or the branch is listed in UNREACHABLE with the argument, and is then asserted never to be taken;
* the cases that leave the eigen-solver through its iter > 300 guard are exactly those named in advance;
* accuracy, against the independent 50-digit reference tests/fit_ref.py: the residual of every returned eigenpair of every other case
  is within 8 x the largest residual numpy.linalg.eig leaves on the same list.
    Measured: numpy.linalg.eig 1.38e-15 (bound 1.10e-14), the oracle 1.91e-15."""
import numpy as np
import pytest

import fit_ref as R
import fit_unit_cases as U
import oracle_lib as O

# Branches that cannot be taken for n = 3 (counted by the oracle all the same, and asserted to stay at 0):
UNREACHABLE = {
    # the double-shift step runs only while no sub-diagonal element is small, i.e. with the active block n = 2 and l = 0; its search
    # for two consecutive small sub-diagonal elements starts at m = n - 2 = 0 = l and `if (m == l) break` ends it at once
    "qr_m_search_continues",
    # p, q, r were divided by x = |p| + |q| + |r| != 0, so the largest of them is at least 1/3 in magnitude and sqrt(p^2 + q^2 + r^2) >= 1/3;
    # were x 0 / 0 = NaN, s is NaN and `s != 0` holds
    "qr_s_zero",
    # back-substitution of a complex vector (the pair sits at (n - 1, n)) walks the rows i <= n - 2: with n = 2 that is row 0 alone, whose
    # eigenvalue is the one left over and therefore real (e[0] == 0); with n = 1 there is no row.  A second complex pair below the first
    # (e[i] < 0, then e[i] > 0: "solve complex equations") needs four eigenvalues.
    "back_complex_e_negative", "back_complex_pair_solve",
    # general_finish: the angle is 0 or 90 + rp[4] * 180 / pi with rp[4] = -atan2(..) / 2 in [-pi/2, pi/2], i.e. within [0, 180] -- or NaN,
    # for which both comparisons are false.  The two wraps are OpenCV's text, kept; no input takes them.
    "angle_wrap_up", "angle_wrap_down",
}
# Branches of the whole fit (which attempt, the box test, the general fit's retry): tests/test_fit_cases_cpu.py asserts them on contours.
FIT_LEVEL = {"direct_attempt0", "direct_attempt1", "direct_none", "direct_bad_box", "general_fit", "general_jitter_retry", "general_no_retry"}


@pytest.fixture(scope="module")
def census_by_record():
    O.set_math_mode(0)
    U.harvest()
    O.census()
    out = []
    for r in U.records():
        U.oracle_bits(r)
        out.append(O.census())
    return out


def test_census_names_are_partitioned():
    names = set(O.census_names())
    assert UNREACHABLE <= names and FIT_LEVEL <= names and not (UNREACHABLE & FIT_LEVEL)


def test_every_branch_of_the_tails_is_reached(census_by_record):
    total = {}
    for c in census_by_record:
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    print({k: v for k, v in total.items()})
    missing = [k for k, v in total.items() if v == 0 and k not in UNREACHABLE and k not in FIT_LEVEL]
    assert not missing, missing
    taken = [k for k in UNREACHABLE if total[k] != 0]
    assert not taken, taken


def test_each_function_reaches_its_own_branches(census_by_record):
    """... and not by accident of another record: the eigen-solver's branches by the eigen-solver's list alone, and so on"""
    eig, direct, n5, n3, centre, finish = census_by_record
    own_eig = [k for k in O.census_names()[:O.census_names().index("direct_attempt0")] if k not in UNREACHABLE]
    assert not [k for k in own_eig if eig[k] == 0], [k for k in own_eig if eig[k] == 0]
    for k in ("cond_pick0", "cond_pick1", "cond_pick2", "norm_negated", "norm_kept", "theta_pv1_zero_0", "theta_pv1_zero_90", "theta_atan2",
              "direct_swap", "direct_no_swap"):
        assert direct[k] > 0, k
    for c in (n5, n3):
        for k in ("jacobi_diagonal_on_entry", "jacobi_converged", "jacobi_sweeps_exhausted", "jacobi_apq_zero", "jacobi_apq_tiny",
                  "jacobi_apq_negligible", "jacobi_rotate", "jacobi_theta_negative", "normal_lam_not_positive", "normal_column_dropped",
                  "normal_column_used"):
            assert c[k] > 0, k
    assert centre["centre_det_zero"] > 0 and centre["centre_det_nonzero"] > 0
    for k in ("finish_c_above_eps", "finish_c_below_eps", "finish_rp2_above", "finish_rp2_below", "finish_rp3_above", "finish_rp3_below",
              "general_swap", "general_no_swap"):
        assert finish[k] > 0, k


def test_guard_cases_are_those_named_in_advance():
    O.set_math_mode(0)
    r = U.eig_record()
    left_by_guard = set()
    O.census()
    for name, x in zip(r.names, r.inputs):
        O.eigen_nonsymmetric3(x)
        c = O.census()
        if c["guard"]:
            assert c["qr_step"] + c["guard"] <= 301 * 2, (name, c["qr_step"])   # bounded: 301 steps per guard exit
            left_by_guard.add(name)
    assert left_by_guard == U.eig_parity_only()


def test_use_bits_of_rank_deficient_systems():
    n5, n3 = U.normal_records()
    for rec, k in ((n5, 5), (n3, 3)):
        by = dict(zip(rec.names, rec.inputs))
        for name in ("rank_deficient_collinear",) if k == 5 else ("rank_deficient",):
            lam, use, wmax, wmin, x = O.normal_unit(by[name][:k * k], by[name][k * k:], k)
            assert use != (1 << k) - 1 and use != 0, (name, use)
        lam, use, _, _, x = O.normal_unit(by["zero"][:k * k], by["zero"][k * k:], k)
        assert use == 0 and not x.any()


def test_unit_entry_points_restate_the_whole_fit():
    """the harvested inputs, put through the unit entry points, give the boxes the whole fits gave: the units ARE the fit's tails"""
    import fit_cases
    O.set_math_mode(0)
    for c in fit_cases.point_cases():
        box, path = O.fit_ellipse_direct(c.pts)
        t = O.last_fit()
        if path == 0:
            a = int(t["d_attempts"]) - 1
            _, _, _, ubox = O.direct_unit(t["dm"][21 * a:21 * a + 21], t["d_scale"], t["d_cx"], t["d_cy"])
        else:
            rp = O.general_centre(t["gfp5"])
            assert rp[0] == t["rp0"] and rp[1] == t["rp1"], c.name
            ubox = O.general_finish(t["gfp3"], t["rp0"], t["rp1"], t["g_scale"], t["g_cx"], t["g_cy"])
        assert ubox.tobytes() == box.tobytes(), (c.name, ubox, box)


def test_eigen_residuals_against_lapack_at_50_digits():
    O.set_math_mode(0)
    r = U.eig_record()
    skip = U.eig_parity_only()
    worst_oracle, worst_lapack, where = 0.0, 0.0, None
    for name, x in zip(r.names, r.inputs):
        if name in skip:
            continue
        assert np.isfinite(x).all()
        ev, vec, im = O.eigen_nonsymmetric3(x)
        a = R.eig_residual_returned(x, ev, vec, im)
        if not a <= worst_oracle:
            worst_oracle, where = a, name
        worst_lapack = max(worst_lapack, R.eig_residual_lapack(x))
    print("largest residual: numpy.linalg.eig %.3e (bound %.3e), oracle %.3e at %s" % (worst_lapack, 8 * worst_lapack, worst_oracle, where))
    assert worst_oracle <= 8 * worst_lapack, (worst_oracle, worst_lapack, where)
