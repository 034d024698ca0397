"""Case lists for the scalar tails of the ellipse fit, one function at a time: the 3 x 3 eigen-solver (cv::eigenNonSymmetric: JAMA orthes +
hqr2), direct_reduce + direct_finish, normal_factor + normal_apply for k = 5 and 3, general_centre and general_finish.  Shared by
tests/test_fit_units_cpu.py (the oracle's branch census over these lists, and its accuracy against tests/fit_ref.py) and
tests/test_gpu_fit_units.py (tests/fit_units/fit_units_main.hip on the device, bit for bit against the oracle).

Seeded and deterministic.  The expected bits come from the oracle's own static functions through its orc_* unit entry points
(oracle/rmcv_oracle.h).  File formats: see tests/fit_units/fit_units_main.hip."""
import struct
from collections import namedtuple

import numpy as np

import fit_cases
import oracle_lib as O

MAGIC = 0x54494655
FU_EIG, FU_DIRECT, FU_NORMAL5, FU_NORMAL3, FU_CENTRE, FU_FINISH = range(6)
FUNCS = ("eigen_nonsymmetric3", "direct_reduce_finish", "normal_factor_apply_5", "normal_factor_apply_3", "general_centre", "general_finish")
N_IN = (9, 24, 30, 12, 5, 8)
N_OUT = (12, 16, 13, 13, 2, 5)

Record = namedtuple("Record", "fid names inputs")   # inputs: float64 (count, N_IN[fid])

N_RANDOM_EIG = 4000
NAN, INF = float("nan"), float("inf")
TINY = 5e-324   # the smallest denormal


def eig_specials():
    """[(name, 3 x 3 matrix, parity_only)]: parity_only names, IN ADVANCE, the cases that are compared bit for bit only and take no part in the
    accuracy check: the non-finite ones, and the two finite ones that cannot converge by the text of hqr2 -- its deflation test is
    |H[l][l-1]| < eps * s with s = |H[l-1][l-1]| + |H[l][l]| (or norm where that is 0): for the zero matrix s = norm = 0, for a matrix of
    denormals eps * s underflows to 0, and nothing is below 0.  All of these leave through the solver's iter > 300 guard after 301 steps
    (tests/test_fit_units_cpu.py asserts that these, and only these, do)."""
    c, s = np.cos(0.7), np.sin(0.7)
    g = np.random.default_rng(424242).standard_normal((3, 3))
    d = np.array([1e50, 1.0, 1e-50])
    out = [
        ("zero", np.zeros((3, 3)), True),
        ("identity", np.eye(3), False),
        ("upper_triangular", [[2, 3, 5], [0, -1, 7], [0, 0, 4]], False),
        ("lower_triangular", [[2, 0, 0], [3, -1, 0], [5, 7, 4]], False),
        ("cycle_012", [[0, 1, 0], [0, 0, 1], [1, 0, 0]], False),
        ("cycle_021", [[0, 0, 1], [1, 0, 0], [0, 1, 0]], False),
        ("rotation_block_real_third", [[c, -s, 0], [s, c, 0], [0, 0, 2]], False),
        ("rotation_block_real_first", [[2, 0, 0], [0, c, -s], [0, s, c]], False),
        ("rotation_mixed", [[c, -s, 1], [s, c, -2], [0.5, 0.25, 2]], False),
        ("jordan_block", [[2, 1, 0], [0, 2, 1], [0, 0, 2]], False),
        ("nilpotent", [[0, 1, 0], [0, 0, 1], [0, 0, 0]], False),
        ("one_to_nine", [[1, 2, 3], [4, 5, 6], [7, 8, 9]], False),
        ("span_1e300_triangular", [[1e300, 1, 1e-300], [0, 1e-300, 1], [0, 0, 1]], False),
        ("span_graded_similarity", g * np.outer(d, 1.0 / d), False),   # D G D^-1: entries from 1e-100 to 1e+100
        ("scaled_up_1e140", g * 1e140, False),
        ("scaled_down_1e-140", g * 1e-140, False),
        ("near_equal_eigenvalues", [[1, 1e-8, 0], [1e-8, 1, 1e-8], [0, 1e-8, 1 + 1e-12]], False),
        ("near_equal_nonsymmetric", [[1, 1, 0], [1e-14, 1, 1], [0, 1e-14, 1]], False),
        ("first_column_reduced", [[3, 1, 2], [0, 4, -5], [0, 6, 7]], False),       # H[1][0] = H[2][0] = 0: the scale == 0 skip of orthes
        ("first_column_reduced_real", [[3, 1, 2], [0, 4, 5], [0, 6, 7]], False),
        ("symmetric", [[4, 1, 2], [1, 3, 0], [2, 0, 1]], False),
        ("negative_definite", [[-4, 1, 2], [1, -3, 0], [2, 0, -7]], False),
        ("rank_one", np.outer([1, 2, 3], [4, 5, 6]), False),
        # a complex pair next to a real eigenvalue 1e-3 away, coupled by 1e6: the complex vector's overflow control ((eps t) t > 1)
        ("complex_pair_huge_vector", [[1, 1e6, 1e6], [0, 1, -1e-3], [0, 1e-3, 1]], False),
        # wildly graded (entries from 1e-121 to 1e+79, found by a seeded search): 30 steps without a root, then the second exceptional
        # shift with s > 0 -- the one finite input known to take it
        ("graded_second_exceptional_shift", [[float.fromhex(h) for h in r] for r in (
            ("0x1.3a0b6d094bae5p-237", "-0x1.4104b8de58c08p-196", "-0x1.bc9bd95aea72ap+260"),
            ("-0x1.5bc56c0c7e408p+264", "-0x1.7f17d65129729p-354", "-0x1.34095eced46aep-401"),
            ("-0x1.71008ffea23a3p-217", "-0x1.395f948b5c466p+99", "0x1.4ffc1c6a9ae1ep-130"))], False),
        ("all_denormal", [[TINY * k for k in (1, 2, 3)], [TINY * k for k in (4, 5, 6)], [TINY * k for k in (7, 8, 10)]], True),
        ("all_nan", np.full((3, 3), NAN), True),
        ("one_nan", [[1, 2, 3], [4, NAN, 6], [7, 8, 9]], True),
        ("one_inf", [[1, 2, 3], [4, 5, INF], [7, 8, 9]], True),
    ]
    return [(n, np.array(m, np.float64).reshape(3, 3), p) for n, m, p in out]


def eig_record():
    rng = np.random.default_rng(20260301)
    rnd = rng.standard_normal((N_RANDOM_EIG, 9))
    sp = eig_specials()
    names = ["gauss%d" % i for i in range(N_RANDOM_EIG)] + [n for n, _, _ in sp]
    return Record(FU_EIG, names, np.concatenate([rnd, np.array([m.reshape(9) for _, m, _ in sp])]))


def eig_parity_only():
    return {n for n, _, p in eig_specials() if p}


_harvest = None


def harvest():
    """the inputs the oracle's fits of tests/fit_cases.py (point lists and the contours of the small image) hand to their scalar tails"""
    global _harvest
    if _harvest is None:
        O.set_math_mode(0)
        lists = [(c.name, c.pts) for c in fit_cases.point_cases()]
        mask = fit_cases.shapes_mask()
        pts, offs = O.find_contours(mask)
        lists += [("shapes_contour%d" % k, pts[offs[k]:offs[k + 1]]) for k in range(len(offs) - 1) if offs[k + 1] - offs[k] >= 6]
        out = []
        for name, p in lists:
            O.fit_ellipse_direct(p)
            out.append((name, O.last_fit()))
        _harvest = out
    return _harvest


def _sym(k, diag, off):
    """a k x k symmetric matrix from its diagonal and {(i, j): value}"""
    G = np.diag(np.array(diag, np.float64))
    for (i, j), v in off.items():
        G[i, j] = G[j, i] = v
    return G


def direct_record():
    names, rows = [], []
    for name, t in harvest():
        for a in range(int(t["d_attempts"])):
            names.append("%s_attempt%d" % (name, a))
            rows.append(np.concatenate([t["dm"][21 * a:21 * a + 21], [t["d_scale"], t["d_cx"], t["d_cy"]]]))
    return Record(FU_DIRECT, names, np.array(rows))


def normal_records():
    n5, r5, n3, r3 = [], [], [], []
    for name, t in harvest():
        if t["g_ran"]:
            n5.append(name)
            r5.append(np.concatenate([t["G5"], t["g5"]]))
            n3.append(name)
            r3.append(np.concatenate([t["G3"], t["g3"]]))
    # collinear points: a design matrix of rank 2 (the rows are (-x^2, 0, 0, x, 0)): `use` bits cleared
    xs = np.arange(-5.0, 6.0) / 7.0
    A = np.stack([-xs * xs, 0 * xs, 0 * xs, xs, 0 * xs], 1)
    hand5 = [
        ("rank_deficient_collinear", A.T @ A, A.T @ np.full(len(xs), 10000.0)),
        ("diagonal", np.diag([4.0, 1.0, 9.0, 0.25, 16.0]), [1, 2, 3, 4, 5]),                 # off == 0 on entry
        ("diagonal_with_zero_and_negative", np.diag([4.0, 0.0, -9.0, 0.25, 16.0]), [1, 2, 3, 4, 5]),
        ("off_diagonal_below_1e-300", _sym(5, [1, 2, 3, 4, 5], {(0, 1): 1e-310, (2, 4): -3e-305}), [1, 1, 1, 1, 1]),
        ("off_diagonal_negligible", _sym(5, [1, 2, 3, 4, 5], {(0, 3): 1e-20, (1, 2): 0.5}), [1, -1, 1, -1, 1]),
        ("equal_diagonal", _sym(5, [2, 2, 2, 2, 2], {(0, 1): 1, (1, 2): -1, (2, 3): 1, (3, 4): -1}), [1, 2, 3, 4, 5]),   # theta == 0
        ("zero", np.zeros((5, 5)), [1, 2, 3, 4, 5]),
        ("all_nan", np.full((5, 5), NAN), [1, 2, 3, 4, 5]),                                    # never converges: the 60-sweep limit
    ]
    hand3 = [
        ("rank_deficient", np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]), [1, 1, 1]),
        ("diagonal", np.diag([4.0, 1.0, 9.0]), [1, 2, 3]),
        ("off_diagonal_below_1e-300", _sym(3, [1, 2, 3], {(0, 2): 1e-310}), [1, 1, 1]),
        ("negative_off_diagonal", _sym(3, [3, 2, 1], {(0, 1): -0.5, (1, 2): 0.25}), [1, -2, 3]),
        ("zero", np.zeros((3, 3)), [1, 2, 3]),
        ("all_nan", np.full((3, 3), NAN), [1, 2, 3]),
    ]
    for n, G, g in hand5:
        n5.append(n)
        r5.append(np.concatenate([np.asarray(G, np.float64).reshape(25), np.asarray(g, np.float64)]))
    for n, G, g in hand3:
        n3.append(n)
        r3.append(np.concatenate([np.asarray(G, np.float64).reshape(9), np.asarray(g, np.float64)]))
    return Record(FU_NORMAL5, n5, np.array(r5)), Record(FU_NORMAL3, n3, np.array(r3))


def centre_record():
    names, rows = [], []
    for name, t in harvest():
        if t["g_ran"]:
            names.append(name)
            rows.append(t["gfp5"])
    hand = [("zero", [0, 0, 0, 0, 0]), ("det_zero_exactly", [1, 1, 2, 3, 4]), ("det_negative", [1, 1, 3, 3, 4]), ("plain", [2, 3, 1, -4, 5]),
            ("nan", [NAN, 1, 1, 1, 1])]
    for n, v in hand:
        names.append(n)
        rows.append(np.array(v, np.float64))
    return Record(FU_CENTRE, names, np.array(rows))


def finish_record():
    """(gfp[3], rp0, rp1, scale, cx, cy); cx and cy are float32 values"""
    names, rows = [], []
    for name, t in harvest():
        if t["g_ran"]:
            names.append(name)
            rows.append(np.concatenate([t["gfp3"], [t["rp0"], t["rp1"], t["g_scale"], t["g_cx"], t["g_cy"]]]))
    hand = [
        ("c_just_above_min_eps", [1.0, 2.0, 1.0000001e-8]), ("c_at_min_eps", [1.0, 2.0, 1e-8]), ("c_just_below_min_eps", [1.0, 2.0, 0.9999999e-8]),
        ("c_negative_above", [1.0, 2.0, -3e-8]), ("c_zero_w_greater", [1.0, 2.0, 0.0]), ("c_zero_w_smaller", [2.0, 1.0, 0.0]),
        ("equal_axes", [1.5, 1.5, 0.0]), ("tilted_w_greater", [1.0, 3.0, 0.8]), ("tilted_w_smaller", [3.0, 1.0, -0.8]),
        ("rp2_below_min_eps", [1e-9, 5e-9, 0.0]), ("rp3_below_min_eps", [5e-9, -5e-9 + 1e-10, 0.0]), ("zero", [0.0, 0.0, 0.0]),
        ("hyperbola", [1.0, -2.0, 0.5]), ("nan", [NAN, 1.0, 0.5]),
    ]
    for n, v in hand:
        names.append(n)
        rows.append(np.array(list(v) + [0.25, -0.125, 0.0125, 640.5, 511.75], np.float64))
    return Record(FU_FINISH, names, np.array(rows))


_records = None


def records():
    global _records
    if _records is None:
        n5, n3 = normal_records()
        _records = [eig_record(), direct_record(), n5, n3, centre_record(), finish_record()]
        for r in _records:
            assert r.inputs.shape == (len(r.names), N_IN[r.fid]) and r.inputs.dtype == np.float64, (r.fid, r.inputs.shape)
    return _records


def write_case_file(path, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(recs)))
        for r in recs:
            f.write(struct.pack("<IIIIQ", r.fid, N_IN[r.fid], N_OUT[r.fid], 0, len(r.names)))
            f.write(np.ascontiguousarray(r.inputs, "<f8").tobytes())


def read_result_file(path, recs):
    """[uint64 (count, N_OUT)] per record"""
    out = []
    with open(path, "rb") as f:
        magic, n = struct.unpack("<II", f.read(8))
        assert magic == MAGIC and n == len(recs), (magic, n)
        for r in recs:
            fid, n_out, count = struct.unpack("<IIQ", f.read(16))
            assert (fid, n_out, count) == (r.fid, N_OUT[r.fid], len(r.names)), (fid, n_out, count)
            out.append(np.frombuffer(f.read(8 * n_out * count), "<u8").reshape(count, n_out).copy())
        assert f.read() == b""
    return out


def _d(v):
    return np.array(v, np.float64).reshape(-1).view(np.uint64)


def _f(v):
    return np.array(v, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)


def _box(b):
    return _f([b["cx"], b["cy"], b["w"], b["h"], b["angle"]])


def oracle_bits(rec):
    """the oracle's results in the result file's slots: uint64 (count, N_OUT)"""
    O.set_math_mode(0)
    out = np.zeros((len(rec.names), N_OUT[rec.fid]), np.uint64)
    for i, x in enumerate(rec.inputs):
        if rec.fid == FU_EIG:
            ev, vec, _ = O.eigen_nonsymmetric3(x)
            out[i] = np.concatenate([_d(ev), _d(vec)])
        elif rec.fid == FU_DIRECT:
            det, M, Ts, box = O.direct_unit(x[:21], x[21], x[22], x[23])
            out[i] = np.concatenate([_d(det), _d(M), _d(Ts), _box(box)])
        elif rec.fid in (FU_NORMAL5, FU_NORMAL3):
            k = 5 if rec.fid == FU_NORMAL5 else 3
            lam, use, wmax, wmin, xs = O.normal_unit(x[:k * k], x[k * k:], k)
            out[i] = np.concatenate([_d(lam), np.array([use], np.uint64), _d(wmax), _d(wmin), _d(xs)])
        elif rec.fid == FU_CENTRE:
            out[i] = _d(O.general_centre(x))
        else:
            out[i] = _box(O.general_finish(x[:3], x[3], x[4], x[5], np.float32(x[6]), np.float32(x[7])))
    return out


# which result slots hold float32 bits (the others are doubles, or the integer `use`)
def slot_kinds(fid):
    if fid == FU_DIRECT:
        return "d" * 11 + "f" * 5
    if fid in (FU_NORMAL5, FU_NORMAL3):
        return "ddddd" + "i" + "dd" + "ddddd"
    if fid == FU_FINISH:
        return "fffff"
    return "d" * N_OUT[fid]


def same_bits(a, b, kinds):
    """element-wise: raw bits equal, or both NaN (of the slot's format)"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    eq = a == b
    for j, k in enumerate(kinds):
        if k == "d":
            nan = np.isnan(a[..., j].view(np.float64)) & np.isnan(b[..., j].view(np.float64))
        elif k == "f":
            nan = np.isnan(a[..., j].astype(np.uint32).view(np.float32)) & np.isnan(b[..., j].astype(np.uint32).view(np.float32)) & (a[..., j] >> 32 == 0) & (b[..., j] >> 32 == 0)
        else:
            continue
        eq[..., j] |= nan
    return eq
