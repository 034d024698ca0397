"""A plain high-precision reference for the ellipse fit (mpmath at 50 digits and numpy; CPU only), independent of the oracle's and the
device's text: tests/test_gpu_fit_units.py and tests/test_gpu_fit_cases.py prove device == oracle bit for bit, so the accuracy checks of
tests/test_fit_units_cpu.py and tests/test_fit_cases_cpu.py run on the oracle's outputs against THIS module.

Eigen-solver: the normalised residual |M v - lambda v| / (|M|_F |v|) of a returned pair at 50 digits -- a backward error, independent of
the problem's conditioning.  The bound is 8 x the largest residual numpy.linalg.eig (LAPACK's balanced solver) leaves on the same list
(the factor is for JAMA's unbalanced hqr2).
    Measured on tests/fit_unit_cases.py (4 000 Gaussian matrices and the 24 named finite, converging specials):
        numpy.linalg.eig   max residual 1.38e-15   -> bound 1.10e-14
        the oracle          max residual 1.91e-15   (at gauss2803; its worst over the named specials: 1.13e-15, `symmetric`)

Direct fit: Fitzgibbon's constrained problem (Halir & Flusser's reduced 3 x 3 form) at 50 digits from the integer points, with the
fit's own centroid and L1 scale; centre, axes and angle compared with the oracle's float32 RotatedRect in float32 ulps per field.  The
tolerance per field is 4 x the deviation of the float64 numpy solution of the SAME problem (direct_fit_numpy: widened from the
unconstrained SVD conic fit of tests/test_oracle_independent.py, which answers a different question) from the 50-digit one, plus one
float32 ulp.  The angle is compared where the 50-digit axis ratio is at least 1.05.
    Measured on the first-attempt direct solutions of tests/fit_cases.py (float32 ulps, the oracle against 50 digits; the tolerance was
    1.0 on each of them, numpy's own deviation being below 1e-7 ulp):  cx 0.44   cy 0.48   w 0.49   h 0.48   angle 0.41"""
import numpy as np
from mpmath import mp, mpf, mpc, matrix, eig as mp_eig, sqrt as mp_sqrt, atan2 as mp_atan2, pi as mp_pi

DIGITS = 50


def _mp_matrix(M):
    return matrix([[mpf(float(v)) for v in row] for row in np.asarray(M, np.float64).reshape(3, 3)])


def _residual(M, lam, v):
    """|M v - lam v|_2 / (|M|_F |v|_2) in the working precision; M 3 x 3 mp matrix, v a list of 3 (complex) numbers"""
    r2 = mpf(0)
    for i in range(3):
        t = sum(M[i, j] * v[j] for j in range(3)) - lam * v[i]
        r2 += abs(t) ** 2
    mn = mp_sqrt(sum(abs(M[i, j]) ** 2 for i in range(3) for j in range(3)))
    vn = mp_sqrt(sum(abs(x) ** 2 for x in v))
    if mn == 0 or vn == 0:
        return mpf(0) if r2 == 0 else mpf("inf")
    return mp_sqrt(r2) / (mn * vn)


def eig_residual_returned(M, evals, evecs, eimag):
    """the largest residual over what cv::eigenNonSymmetric returned (eigenvalues sorted descending, eigenvectors as ROWS; hqr2 leaves a
    complex pair lambda = d +- i e as two neighbours: the row whose e is positive is the real part of the vector of d + i e, the next row
    its imaginary part)"""
    with mp.workdps(DIGITS):
        A = _mp_matrix(M)
        worst = mpf(0)
        i = 0
        while i < 3:
            if eimag[i] == 0:
                v = [mpf(float(x)) for x in evecs[i]]
                worst = max(worst, _residual(A, mpf(float(evals[i])), v))
                i += 1
            else:
                assert i + 1 < 3 and eimag[i] > 0 and eimag[i + 1] == -eimag[i], (i, eimag)
                v = [mpc(float(a), float(b)) for a, b in zip(evecs[i], evecs[i + 1])]
                lam = mpc(float(evals[i]), float(eimag[i]))
                worst = max(worst, _residual(A, lam, v))   # (the conjugate pair has the same residual)
                i += 2
        return float(worst)


def eig_residual_lapack(M):
    """the same figure for numpy.linalg.eig on the same matrix"""
    w, V = np.linalg.eig(np.asarray(M, np.float64).reshape(3, 3))
    with mp.workdps(DIGITS):
        A = _mp_matrix(M)
        worst = mpf(0)
        for k in range(3):
            v = [mpc(float(np.real(V[j, k])), float(np.imag(V[j, k]))) for j in range(3)]
            worst = max(worst, _residual(A, mpc(float(np.real(w[k])), float(np.imag(w[k]))), v))
        return float(worst)


# ---------------------------------------------------------------- the direct fit
def _ellipse_from_conic(a, b, c, d, e, f, sqrt, atan2, pi):
    """centre, full axes (minor, major) and the minor axis' direction in degrees [0, 180) of a x^2 + b xy + c y^2 + d x + e y + f = 0"""
    den = b * b - 4 * a * c
    x0 = (2 * c * d - b * e) / den
    y0 = (2 * a * e - b * d) / den
    f0 = a * x0 * x0 + b * x0 * y0 + c * y0 * y0 + d * x0 + e * y0 + f       # the conic's value at the centre
    # eigenvalues of [[a, b/2], [b/2, c]]: l1 >= l2 (after making the form positive definite); semi-axis_i = sqrt(-f0 / l_i)
    if a + c < 0:
        a, b, c, f0 = -a, -b, -c, -f0
    root = sqrt((a - c) * (a - c) + b * b)
    l1, l2 = (a + c + root) / 2, (a + c - root) / 2
    minor, major = 2 * sqrt(-f0 / l1), 2 * sqrt(-f0 / l2)
    # the minor axis is the eigenvector of l1: (b/2, l1 - a) or (l1 - c, b/2)
    if abs(l1 - a) > abs(l1 - c):
        vx, vy = b / 2, l1 - a
    else:
        vx, vy = l1 - c, b / 2
    ang = atan2(vy, vx) * 180 / pi
    ang = ang % 180
    return x0, y0, minor, major, ang


def direct_fit_mp(pts):
    """Fitzgibbon's direct least-squares ellipse at 50 digits: (cx, cy, w, h, angle) as mpf, w <= h, angle = direction of the w axis"""
    with mp.workdps(DIGITS):
        xs = [mpf(int(v)) for v in pts["x"]]
        ys = [mpf(int(v)) for v in pts["y"]]
        n = len(xs)
        cx, cy = sum(xs) / n, sum(ys) / n
        s = sum(abs(x - cx) + abs(y - cy) for x, y in zip(xs, ys))
        k = 100 / s
        S = matrix(6, 6)
        for x, y in zip(xs, ys):
            px, py = (x - cx) * k, (y - cy) * k
            row = [px * px, px * py, py * py, px, py, mpf(1)]
            for i in range(6):
                for j in range(6):
                    S[i, j] += row[i] * row[j]
        S1, S2, S3 = S[0:3, 0:3], S[0:3, 3:6], S[3:6, 3:6]
        T = -(S3 ** -1) * S2.T
        Mr = S1 + S2 * T
        C1inv = matrix([[0, 0, mpf(1) / 2], [0, -1, 0], [mpf(1) / 2, 0, 0]])
        E, V = mp_eig(C1inv * Mr)
        best = None
        for j in range(3):
            v = [V[i, j] for i in range(3)]
            big = max(v, key=abs)
            v = [x / big for x in v]                 # (an eigenvector comes with an arbitrary, possibly complex, factor)
            if any(abs(x.imag) > mpf(10) ** -30 * max(abs(y) for y in v) for x in v if isinstance(x, mpc)):
                continue
            v = [x.real if isinstance(x, mpc) else x for x in v]
            cond = 4 * v[0] * v[2] - v[1] * v[1]
            nrm = mp_sqrt(sum(x * x for x in v))
            if cond > 0 and (best is None or cond / (nrm * nrm) > best[0]):
                best = (cond / (nrm * nrm), v)
        assert best is not None, "no elliptic eigenvector"
        a1 = matrix(best[1])
        a2 = T * a1
        x0, y0, w, h, ang = _ellipse_from_conic(a1[0], a1[1], a1[2], a2[0], a2[1], a2[2], mp_sqrt, mp_atan2, mp_pi)
        return x0 / k + cx, y0 / k + cy, w / k, h / k, ang


def direct_fit_numpy(pts):
    """the same problem in float64 with numpy (np.linalg.eig on the reduced system): what plain double arithmetic gives on this case"""
    x, y = pts["x"].astype(np.float64), pts["y"].astype(np.float64)
    cx, cy = x.mean(), y.mean()
    k = 100.0 / (np.abs(x - cx) + np.abs(y - cy)).sum()
    px, py = (x - cx) * k, (y - cy) * k
    D1 = np.stack([px * px, px * py, py * py], 1)
    D2 = np.stack([px, py, np.ones_like(px)], 1)
    S1, S2, S3 = D1.T @ D1, D1.T @ D2, D2.T @ D2
    T = -np.linalg.solve(S3, S2.T)
    Mr = S1 + S2 @ T
    Mr = np.array([Mr[2] / 2, -Mr[1], Mr[0] / 2])
    E, V = np.linalg.eig(Mr)
    V = np.real(V)
    cond = 4 * V[0] * V[2] - V[1] ** 2
    a1 = V[:, int(np.argmax(cond))]
    a2 = T @ a1
    x0, y0, w, h, ang = _ellipse_from_conic(a1[0], a1[1], a1[2], a2[0], a2[1], a2[2], np.sqrt, np.arctan2, np.pi)
    return x0 / k + cx, y0 / k + cy, w / k, h / k, ang


FIELDS = ("cx", "cy", "w", "h", "angle")


def ulp32(v):
    v = abs(float(v))
    return float(np.spacing(np.float32(v))) if v > 0 else float(np.spacing(np.float32(0)))


def field_errors(box, pts):
    """per field: (|oracle - exact| in float32 ulps of the exact value, the tolerance 4 x |numpy - exact| + 1 in the same ulps), or None
    for the angle of a nearly round ellipse (50-digit axis ratio below 1.05)"""
    ex = direct_fit_mp(pts)
    nm = direct_fit_numpy(pts)
    out = {}
    with mp.workdps(DIGITS):
        ratio = ex[3] / ex[2]
        for j, name in enumerate(FIELDS):
            if name == "angle" and ratio < mpf("1.05"):
                out[name] = None
                continue
            u = ulp32(ex[j])

            def dist(a, b):
                d = abs(mpf(float(a)) - b)
                if name == "angle":
                    d = min(d, 180 - d)          # directions of an axis: 179.99 and 0.01 are 0.02 apart
                return float(d / u)
            out[name] = (dist(box[name], ex[j]), 4 * dist(nm[j], ex[j]) + 1.0)
    return out
