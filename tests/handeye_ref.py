"""The hand-eye solve restated from the text at the head of rmcv_amd/csrc/device_handeye.h in numpy and plain Python floats, in the
pinned order: every expression is written as the text writes it, every sum over pairs or views is a block sum (256 partials in ascending index,
a butterfly 32 .. 1 within each group of 64, then ((g0 + g1) + g2) + g3).  The gimbal's matrix is the library's pinned rmcv_euler_to_matrix
(the text names that function); behind it only + - * / and sqrt occur, and nothing else here calls the library."""
import math
from collections import namedtuple

import numpy as np

from rmcv_amd import abi

OK, T_UNOBSERVABLE, TOO_FEW_VIEWS, TOO_MANY_VIEWS = 1, 2, 4, 8
VIEWS_MIN, VIEWS_PER_CAMERA_MAX, JACOBI_SWEEPS = 3, 256, 30
DEFAULTS = dict(min_w=0.5)

# a camera without a solution is a Counts alone
Counts = namedtuple("Counts", "status views_used pairs_used pairs_skipped sweeps")
Result = namedtuple("Result", "cam2gripper q t eig pivots rot_rms trans_rms world_mean world_rms views_used pairs_used pairs_skipped sweeps status")


def block_sum(terms, keep=None):
    """terms (P, N) float64 -> (N,): partial T takes rows k % 256 == T in ascending k from 0.0 (rows with keep False add nothing); then within each
    group of 64 acc[l] += acc[l ^ s], s = 32 .. 1; then ((g0 + g1) + g2) + g3"""
    terms = np.asarray(terms, np.float64)
    if terms.ndim == 1:
        terms = terms[:, None]
    acc = np.zeros((256, terms.shape[1]))
    for r in range(0, len(terms), 256):
        blk = terms[r:r + 256]
        new = acc[:len(blk)] + blk
        acc[:len(blk)] = new if keep is None else np.where(keep[r:r + 256, None], new, acc[:len(blk)])
    g = acc.reshape(4, 64, -1)
    s = 32
    while s >= 1:
        g = g + g[:, np.arange(64) ^ s]
        s >>= 1
    return ((g[0, 0] + g[1, 0]) + g[2, 0]) + g[3, 0]


def mat_to_quat(R):
    """the calibration solve's rule: the first largest of (trace, R00, R11, R22), then divided by its norm"""
    R00, R01, R02, R10, R11, R12, R20, R21, R22 = (float(v) for v in np.asarray(R).reshape(9))
    tr = R00 + R11 + R22
    br, best = 0, tr
    for k, v in ((1, R00), (2, R11), (3, R22)):
        if v > best:
            best, br = v, k
    if br == 0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = (s / 4.0, (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s)
    elif br == 1:
        s = 2.0 * math.sqrt(1.0 + R00 - R11 - R22)
        q = ((R21 - R12) / s, s / 4.0, (R01 + R10) / s, (R02 + R20) / s)
    elif br == 2:
        s = 2.0 * math.sqrt(1.0 + R11 - R00 - R22)
        q = ((R02 - R20) / s, (R01 + R10) / s, s / 4.0, (R12 + R21) / s)
    else:
        s = 2.0 * math.sqrt(1.0 + R22 - R00 - R11)
        q = ((R10 - R01) / s, (R02 + R20) / s, (R12 + R21) / s, s / 4.0)
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def qmul(p, q):
    """p, q: sequences of four arrays (or floats)"""
    p0, p1, p2, p3 = p
    q0, q1, q2, q3 = q
    return [((p0 * q0 - p1 * q1) - p2 * q2) - p3 * q3, ((p0 * q1 + p1 * q0) + p2 * q3) - p3 * q2,
            ((p0 * q2 - p1 * q3) + p2 * q0) + p3 * q1, ((p0 * q3 + p1 * q2) - p2 * q1) + p3 * q0]


def conj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def positive_w(q):
    neg = (q[0] < 0.0) | ((q[0] == 0.0) & np.signbit(q[0]))
    return [np.where(neg, -c, c) for c in q]


def rot9(q):
    w, x, y, z = q
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def mv3(M, v):
    return [(M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2] for r in range(3)]


def mv4(M, v):
    return [((M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2]) + M[r][3] * v[3] for r in range(4)]


def jacobi(A, n):
    """the cyclic Jacobi of device_calib.h's text on an n x n matrix -> (A, V, the sweeps begun)"""
    A = [[float(A[i][j]) for j in range(n)] for i in range(n)]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    sweeps = 0
    while sweeps < JACOBI_SWEEPS:
        off = 0.0
        for p in range(n):
            for q in range(p + 1, n):
                off += abs(A[p][q])
        if off == 0.0:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq, app, aqq = A[p][q], A[p][p], A[q][q]
                if apq == 0.0:
                    continue
                if abs(apq) < 1e-300 or abs(apq) <= 1.1102230246251565e-16 * 1e-3 * math.sqrt(abs(app * aqq)):
                    A[p][q] = A[q][p] = 0.0
                    continue
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        nrp, nrq = c * arp - s * arq, s * arp + c * arq
                        A[r][p] = A[p][r] = nrp
                        A[r][q] = A[q][r] = nrq
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - s * vrq
                    V[r][q] = s * vrp + c * vrq
                A[p][p] = app - t * apq
                A[q][q] = aqq + t * apq
                A[p][q] = A[q][p] = 0.0
        sweeps += 1
    return A, V, sweeps


def used_views(views, attitudes, gripper_t=None, view_camera=None, n_cameras=1, cam=0):
    out = []
    for v in range(len(views)):
        label = 0 if view_camera is None else int(view_camera[v])
        if (label if 0 <= label < n_cameras else 0) != cam or int(views["used"][v]) != 1:
            continue
        read = list(views["q"][v]) + list(views["tvec"][v]) + [attitudes["roll"][v], attitudes["pitch"][v], attitudes["yaw"][v]]
        if gripper_t is not None:
            read += list(gripper_t[v])
        if all(math.isfinite(float(x)) for x in read):
            out.append(v)
    return out


def solve(views, attitudes, gripper_t=None, view_camera=None, n_cameras=1, cam=0, min_w=0.5):
    """-> (Result | Counts, {view: world (3,)})"""
    use = used_views(views, attitudes, gripper_t, view_camera, n_cameras, cam)
    n = len(use)
    if n < VIEWS_MIN or n > VIEWS_PER_CAMERA_MAX:
        return Counts(TOO_FEW_VIEWS if n < VIEWS_MIN else TOO_MANY_VIEWS, n, 0, 0, 0), {}
    B = np.stack([abi.euler_to_matrix((attitudes["roll"][v], attitudes["pitch"][v], attitudes["yaw"][v])) for v in use])          # (n, 3, 3)
    qg = np.array([mat_to_quat(B[u]) for u in range(n)])
    qc = np.array([views["q"][v] for v in use], np.float64)
    tc = np.array([views["tvec"][v] for v in use], np.float64)
    tg = np.zeros((n, 3)) if gripper_t is None else np.array([gripper_t[v] for v in use], np.float64)
    # the pairs, i < j in lexicographic order
    pi, pj = np.triu_indices(n, 1)
    col = lambda m, idx: [m[idx, k] for k in range(m.shape[1])]
    a = positive_w(qmul(conj(col(qg, pj)), col(qg, pi)))
    b = positive_w(qmul(col(qc, pj), conj(col(qc, pi))))
    keep = (a[0] >= min_w) & (b[0] >= min_w)
    # 1: the rotation
    d = [a[k] - b[k] for k in range(4)]
    s = [a[k] + b[k] for k in range(4)]
    D = [[d[0], -d[1], -d[2], -d[3]], [d[1], d[0], -s[3], s[2]], [d[2], s[3], d[0], -s[1]], [d[3], -s[2], s[1], d[0]]]
    terms = [((D[0][i] * D[0][k] + D[1][i] * D[1][k]) + D[2][i] * D[2][k]) + D[3][i] * D[3][k] for i in range(4) for k in range(i, 4)]
    ones = np.ones(len(pi))
    m = block_sum(np.stack(terms + [ones], 1), keep)
    pairs_used, pairs_skipped = int(m[10]), int(block_sum(ones, ~keep)[0])
    if pairs_used == 0:
        return Counts(TOO_FEW_VIEWS, n, 0, pairs_skipped, 0), {}
    M, at = [[0.0] * 4 for _ in range(4)], 0
    for i in range(4):
        for k in range(i, 4):
            M[i][k] = M[k][i] = float(m[at])
            at += 1
    A, V, sweeps = jacobi(M, 4)
    diag = [A[i][i] for i in range(4)]
    sel = 0
    for i in range(1, 4):
        if diag[i] < diag[sel]:
            sel = i
    eig = sorted(diag)
    q = [V[r][sel] for r in range(4)]
    nq = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [c / nq for c in q]
    first = next((c for c in q[:3] if c != 0.0), q[3])
    if first < 0.0:
        q = [0.0 - c for c in q]
    RX = rot9(q)
    # 2: the translation
    Rb, Ra = rot9(b), rot9(a)
    e = [tg[pi, k] - tg[pj, k] for k in range(3)]
    Bj = B[pj]
    tA = [(Bj[:, 0, k] * e[0] + Bj[:, 1, k] * e[1]) + Bj[:, 2, k] * e[2] for k in range(3)]
    rbt = mv3(Rb, col(tc, pi))
    tB = [tc[pj, k] - rbt[k] for k in range(3)]
    rxt = mv3(RX, tB)
    g = [rxt[k] - tA[k] for k in range(3)]
    Cm = [[Ra[r][c] - 1.0 if r == c else Ra[r][c] for c in range(3)] for r in range(3)]
    terms = [(Cm[0][i] * Cm[0][k] + Cm[1][i] * Cm[1][k]) + Cm[2][i] * Cm[2][k] for i in range(3) for k in range(i, 3)]
    terms += [(Cm[0][i] * g[0] + Cm[1][i] * g[1]) + Cm[2][i] * g[2] for i in range(3)]
    s9 = [float(v) for v in block_sum(np.stack(terms, 1), keep)]
    N = [[s9[0], s9[1], s9[2]], [s9[1], s9[3], s9[4]], [s9[2], s9[4], s9[5]]]
    r = s9[6:9]
    L, piv, ok = [[0.0] * 3 for _ in range(3)], [0.0, 0.0, 0.0], True
    for i in range(3):
        for k in range(i + 1):
            if not ok:
                break
            v = N[i][k]
            for mm in range(k):
                v = v - L[i][mm] * L[k][mm]
            if i == k:
                piv[i] = v
                if not (v > 0.0) or not math.isfinite(v):
                    ok = False
                else:
                    L[i][i] = math.sqrt(v)
            else:
                L[i][k] = v / L[k][k]
    t = [0.0, 0.0, 0.0]
    if ok:
        x = [0.0, 0.0, 0.0]
        for i in range(3):
            v = r[i]
            for k in range(i):
                v = v - L[i][k] * x[k]
            x[i] = v / L[i][i]
        for i in (2, 1, 0):
            v = x[i]
            for k in range(i + 1, 3):
                v = v - L[k][i] * x[k]
            x[i] = v / L[i][i]
        t = x
    G = [RX[0] + [t[0]], RX[1] + [t[1]], RX[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]]
    # 3: the check loop
    world = np.zeros((n, 3))
    for u in range(n):
        p = mv4(G, [float(tc[u, 0]), float(tc[u, 1]), float(tc[u, 2]), 1.0])
        H = [[float(B[u, r_, 0]), float(B[u, r_, 1]), float(B[u, r_, 2]), float(tg[u, r_])] for r_ in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
        world[u] = mv4(H, p)[:3]
    mean = block_sum(world) / float(n)
    # 4: the residuals
    ew = world - mean
    world_rms = math.sqrt(float(block_sum((ew[:, 0] * ew[:, 0] + ew[:, 1] * ew[:, 1]) + ew[:, 2] * ew[:, 2])[0]) / float(n))
    ct = mv3(Cm, t)
    et = [ct[k] - g[k] for k in range(3)]
    trans_rms = math.sqrt(float(block_sum((et[0] * et[0] + et[1] * et[1]) + et[2] * et[2], keep)[0]) / float(pairs_used))
    rot_rms = math.sqrt((eig[0] if eig[0] > 0.0 else 0.0) / float(pairs_used))
    res = Result(np.array(G).reshape(16), np.array(q), np.array(t), np.array(eig), np.array(piv), rot_rms, trans_rms, mean, world_rms, n, pairs_used, pairs_skipped,
                 sweeps, OK if ok else T_UNOBSERVABLE)
    return res, {v: world[u] for u, v in enumerate(use)}


def records(res, world, n_views):
    """what the entry points write into zeroed tables -> (HANDEYE_RESULT (1,), HANDEYE_VIEW (n_views,))"""
    rec, rows = abi.handeye_outputs(1, n_views)
    for k in res._fields:
        rec[k][0] = getattr(res, k)
    for v, w in world.items():
        rows["world"][v], rows["used"][v] = w, 1
    return rec, rows
