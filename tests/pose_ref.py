"""The pose stage restated in mpmath (TEST INFRASTRUCTURE), from the mathematics and not from oracle/rmcv_oracle_pnp.c:

* the distortion model's inverse by five fixed-point rounds x <- (x0 - tangential(x)) / radial(x), given up (the starting point returned)
  as soon as 1 / radial turns negative;
* the homography of the plate from a linear solve of the eight DLT equations (h33 = 1), its Jacobian at the origin;
* the two IPPE rotations by the paper's construction (Collins & Bartoli 2014, section 4): R_v takes the optical axis to the ray of the
  plate's centre, B = [I2 | -v] R_v restricted to its first two columns, A = B^-1 J, gamma = its largest singular value, R22 = A / gamma, the last
  row (b0, b1) from the unit length and the orthogonality of the first two columns, the third column their cross product;
* each translation as the least-squares solution of its 8 x 3 system; the RMS reprojection error; rotation matrix <-> vector.

Everything at PREC bits.  The narrowing of the undistorted point to float32 is part of the semantics: to_f32 rounds the mp value to 24 bits
directly (to nearest, ties to even), never through a double."""
import mpmath as mpm
from mpmath import mp, mpf

PREC = 240
mp.prec = PREC


def M(x):
    """a Python float / numpy scalar as the mp value it is (exact)"""
    return mpf(float(x))


def to_f32(x):
    """an mp value rounded to the nearest float32 (ties to even), as an mp value; overflow gives +-inf, the subnormal range its fixed step"""
    if not mpm.isfinite(x) or x == 0:
        return x
    e = mpm.frexp(x)[1]                                                        # x = m 2^e, 0.5 <= |m| < 1
    step_exp = max(e - 24, -149)
    n = x / mpf(2) ** step_exp
    r = mpm.floor(n)
    d = n - r
    if d > mpf(0.5) or (d == mpf(0.5) and int(r) % 2):
        r += 1
    out = r * mpf(2) ** step_exp
    if abs(out) >= mpf(2) ** 128:
        return mpf("inf") if out > 0 else mpf("-inf")
    return out


def undistort(u, v, K, dist, rounds=5):
    """-> (x, y, gave_up, [1 / radial of every round run]); K = (fx, fy, cx, cy) and dist = (k1, k2, p1, p2, k3) as mp values"""
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = dist
    nan = mpf("nan")
    if fx == 0 or fy == 0:                                                     # nothing finite to say
        return nan, nan, False, []
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    seen = []
    for _ in range(rounds):
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        if radial == 0:
            return nan, nan, False, seen
        inv_radial = 1 / radial
        seen.append(inv_radial)
        if inv_radial < 0:
            return x0, y0, True, seen
        tx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        ty = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - tx) * inv_radial, (y0 - ty) * inv_radial
    return x, y, False, seen


def config_values(cfg):
    """(K, dist, (half_w, half_h)) of a PnpConfig as mp values; the half sides are halved in float32 like the plate's corners are built"""
    import numpy as np
    cm = list(cfg.camera_matrix)
    K = (M(cm[0]), M(cm[4]), M(cm[2]), M(cm[5]))
    dist = tuple(M(d) for d in cfg.dist)
    half = (M(np.float32(cfg.square_w) / np.float32(2)), M(np.float32(cfg.square_h) / np.float32(2)))
    return K, dist, half


def plate(half):
    hw, hh = half
    return [(-hw, hh), (hw, hh), (hw, -hh), (-hw, -hh)]


def homography(obj, img):
    """h (9 values, h[8] = 1) with img ~ H obj, from the eight DLT equations"""
    A, b = mpm.zeros(8, 8), mpm.zeros(8, 1)
    for i, ((X, Y), (x, y)) in enumerate(zip(obj, img)):
        A[2 * i, 0], A[2 * i, 1], A[2 * i, 2], A[2 * i, 6], A[2 * i, 7], b[2 * i] = X, Y, 1, -x * X, -x * Y, x
        A[2 * i + 1, 3], A[2 * i + 1, 4], A[2 * i + 1, 5], A[2 * i + 1, 6], A[2 * i + 1, 7], b[2 * i + 1] = X, Y, 1, -y * X, -y * Y, y
    h = mpm.lu_solve(A, b)
    return [h[i] for i in range(8)] + [mpf(1)]


def rotation_z_to(v):
    """the rotation about z x v that takes the z axis to v / |v| (Rodrigues' formula for two unit vectors)"""
    n = mpm.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    b = [c / n for c in v]
    w = (-b[1], b[0], mpf(0))                                                  # z x b
    c = b[2]
    W = mpm.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return mpm.eye(3) + W + W * W / (1 + c)


def ippe_rotations(h):
    """-> (R1, R2, detail): the two candidate rotations of the homography h, detail = dict(gamma2, gamma, b0sq, b1sq, sp)"""
    p, q = h[2], h[5]
    J = mpm.matrix([[h[0] - h[6] * p, h[1] - h[7] * p], [h[3] - h[6] * q, h[4] - h[7] * q]])
    Rv = rotation_z_to((p, q, mpf(1)))
    B = mpm.matrix([[Rv[0, 0] - p * Rv[2, 0], Rv[0, 1] - p * Rv[2, 1]], [Rv[1, 0] - q * Rv[2, 0], Rv[1, 1] - q * Rv[2, 1]]])
    A = mpm.inverse(B) * J
    AtA = A.T * A
    tr, det = AtA[0, 0] + AtA[1, 1], AtA[0, 0] * AtA[1, 1] - AtA[0, 1] * AtA[1, 0]
    gamma2 = (tr + mpm.sqrt(max(tr * tr - 4 * det, mpf(0)))) / 2            # the larger eigenvalue of A^T A
    gamma = mpm.sqrt(gamma2)
    detail = dict(gamma2=gamma2, gamma=gamma)
    if not gamma > 0:
        return None, None, detail
    R22 = A / gamma
    b0sq = 1 - R22[0, 0] ** 2 - R22[1, 0] ** 2
    b1sq = 1 - R22[0, 1] ** 2 - R22[1, 1] ** 2
    sp = -(R22[0, 0] * R22[0, 1] + R22[1, 0] * R22[1, 1])                     # = b0 b1
    b0 = mpm.sqrt(max(b0sq, mpf(0)))
    b1 = mpm.sqrt(max(b1sq, mpf(0))) * (-1 if sp < 0 else 1)
    detail.update(b0sq=b0sq, b1sq=b1sq, sp=sp)
    out = []
    for s in (1, -1):
        c1, c2 = (R22[0, 0], R22[1, 0], s * b0), (R22[0, 1], R22[1, 1], s * b1)
        c3 = (c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0])
        out.append(Rv * mpm.matrix([[c1[0], c2[0], c3[0]], [c1[1], c2[1], c3[1]], [c1[2], c2[2], c3[2]]]))
    return out[0], out[1], detail


def translation(obj, img, R):
    """least squares over the eight equations x_i (r3 . P_i + tz) = r1 . P_i + tx, y_i (...) = r2 . P_i + ty"""
    A, b = mpm.zeros(8, 3), mpm.zeros(8, 1)
    for i, ((X, Y), (x, y)) in enumerate(zip(obj, img)):
        rx, ry, rz = R[0, 0] * X + R[0, 1] * Y, R[1, 0] * X + R[1, 1] * Y, R[2, 0] * X + R[2, 1] * Y
        A[2 * i, 0], A[2 * i, 2], b[2 * i] = 1, -x, x * rz - rx
        A[2 * i + 1, 1], A[2 * i + 1, 2], b[2 * i + 1] = 1, -y, y * rz - ry
    t = mpm.lu_solve(A.T * A, A.T * b)
    return [t[0], t[1], t[2]]


def reprojection_error(obj, img, R, t):
    """(RMS error over the eight coordinates, the four depths)"""
    s, depths = mpf(0), []
    for (X, Y), (x, y) in zip(obj, img):
        cx, cy, cz = R[0, 0] * X + R[0, 1] * Y + t[0], R[1, 0] * X + R[1, 1] * Y + t[1], R[2, 0] * X + R[2, 1] * Y + t[2]
        depths.append(cz)
        s += (cx / cz - x) ** 2 + (cy / cz - y) ** 2
    return mpm.sqrt(s / 8), depths


def rotation_angle(R):
    return mpm.acos(max(min((R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2, mpf(1)), mpf(-1)))


def rodrigues(r):
    """rotation vector (3 numbers) -> matrix"""
    r = [M(c) for c in r]
    th = mpm.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)
    if th == 0:
        return mpm.eye(3)
    k = [c / th for c in r]
    W = mpm.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return mpm.eye(3) + mpm.sin(th) * W + (1 - mpm.cos(th)) * W * W


def solve(img, half):
    """the IPPE part on four normalised image points (in the order of the plate's corners).  -> dict: rc, den, and where reached H, R (two),
    t (two), err (two), depths (two), taken, angle (of the pose taken), gamma2, gamma, b0sq, b1sq, sp.  rc 1: the points are degenerate
    (den == 0, or nothing finite to solve) or the plate is (gamma not positive and finite)."""
    out = dict(rc=1)
    (x1, y1), (x2, y2), (x3, y3) = img[1], img[2], img[3]
    out["den"] = den = (x1 - x2) * (y3 - y2) - (x3 - x2) * (y1 - y2)           # twice the area of the triangle of points 1, 2, 3
    obj = plate(half)
    # IPPE_SQUARE by definition: the homography is that of the CANONICAL square whose side is the distance of the first two object points,
    # measured in float32 -- whatever the object points are (a rectangle, a mirrored plate); translation and error use the points given
    ddx, ddy = to_f32(obj[1][0] - obj[0][0]), to_f32(obj[1][1] - obj[0][1])
    out["side"] = side = to_f32(mpm.sqrt(to_f32(to_f32(ddx * ddx) + to_f32(ddy * ddy)))) if all(mpm.isfinite(c) for c in half) else mpf("nan")
    if not mpm.isfinite(den) or den == 0 or not mpm.isfinite(side) or side == 0:
        return out
    try:
        h = homography(plate((side / 2, side / 2)), img)
        R1, R2, detail = ippe_rotations(h)
    except ZeroDivisionError:
        return out
    out.update(detail, H=h)
    if R1 is None or not mpm.isfinite(detail["gamma"]):
        return out
    out["R"] = (R1, R2)
    out["t"] = (translation(obj, img, R1), translation(obj, img, R2))
    errs = [reprojection_error(obj, img, R, t) for R, t in zip(out["R"], out["t"])]
    out["err"], out["depths"] = (errs[0][0], errs[1][0]), (errs[0][1], errs[1][1])
    out["taken"] = 1 if out["err"][0] > out["err"][1] else 0
    out["angle"] = rotation_angle(out["R"][out["taken"]])
    out["rc"] = 0
    return out
