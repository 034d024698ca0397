"""Independent restatement of DESIGN.md 4l (training the icon classifier) in numpy and Python floats: Gram, the SMO pair problem, rho,
w, predict and trainAuto.  Written from the section's prose, not from rmcv_amd/csrc/device_svm.h; Python floats and numpy float64 /
float32 element-wise operations are single rounded IEEE operations, and nothing here is fused.  Every solve also counts which branches
of the rule it took (BRANCHES), so that tests/svm_cases.py can assert that each case still covers what it is for."""
import collections
import math

import numpy as np

NFEAT = 1200
ETA_FLOOR = 1e-12
BRANCHES = collections.Counter()


def default_params():
    grid, c = [], 0.1
    for _ in range(6):
        grid.append(c)
        c = c * 5.0
    return {"eps": 1e-3, "max_iter": 1000, "k_fold": 10, "c_grid": grid}


def gram(samples):
    x = np.asarray(samples, np.uint8).astype(np.int64)
    g = x @ x.T
    assert g.max(initial=0) <= 78030000
    return g


def class_table(responses):
    labels = sorted(set(int(r) for r in responses))
    return labels, np.array([labels.index(int(r)) for r in responses], np.int64)


def pairs(n_class):
    return [(i, j) for i in range(n_class) for j in range(i + 1, n_class)]


def solve_pair(G, rows, y, C, eps, max_iter):
    """rows: the pair's dataset rows, ascending; y: +1 / -1 per sample -> dict(alpha, g, rho, objective, iterations, converged)"""
    rows = np.asarray(rows, np.int64)
    y = np.asarray(y, np.int64)
    n = len(rows)
    K = G[np.ix_(rows, rows)]                               # integers
    yf = y.astype(np.float64)
    alpha, g = np.zeros(n), np.full(n, -1.0)
    iterations, converged = 0, 0
    while True:
        v = -yf * g
        up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0))
        low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
        if not up.any() or not low.any():
            BRANCHES["empty_set"] += 1
            converged = 1
            break
        m, M = v[up].max(), v[low].min()
        i = int(np.flatnonzero(up & (v == m))[0])            # the lowest t among equals
        j = int(np.flatnonzero(low & (v == M))[0])
        if (np.count_nonzero(up & (v == m)) > 1) or (np.count_nonzero(low & (v == M)) > 1):
            BRANCHES["selection_tie"] += 1
        m, M = float(m), float(M)
        if m - M < eps:
            BRANCHES["converged"] += 1
            converged = 1
            break
        if iterations == max_iter:
            BRANCHES["max_iter"] += 1
            break
        eta_int = int(K[i, i]) + int(K[j, j]) - 2 * int(K[i, j])
        eta = float(eta_int)
        if not eta > 0.0:
            BRANCHES["eta_floor"] += 1
            eta = ETA_FLOOR
        lam = (m - M) / eta
        ai, aj = float(alpha[i]), float(alpha[j])
        room_i = C - ai if y[i] > 0 else ai
        room_j = aj if y[j] > 0 else C - aj
        cut = 0
        if room_i < lam:
            lam, cut = room_i, 1
        if room_j < lam:
            lam, cut = room_j, 2
        BRANCHES["cut%d" % cut] += 1
        ni = ai + lam if y[i] > 0 else ai - lam
        nj = aj - lam if y[j] > 0 else aj + lam
        if cut == 1:
            ni = C if y[i] > 0 else 0.0
        if cut == 2:
            nj = 0.0 if y[j] > 0 else C
        ni, nj = min(max(ni, 0.0), C), min(max(nj, 0.0), C)
        di, dj = ni - ai, nj - aj
        qi = (yf * yf[i]) * K[:, i].astype(np.float64)       # exact
        qj = (yf * yf[j]) * K[:, j].astype(np.float64)
        g = (g + qi * di) + qj * dj
        alpha[i], alpha[j] = ni, nj
        iterations += 1
    # outputs
    sum_free, n_free, obj, ub, lb = 0.0, 0, 0.0, math.inf, -math.inf
    for t in range(n):
        a, yg = float(alpha[t]), float(yf[t] * g[t])
        if 0.0 < a < C:
            sum_free, n_free = sum_free + yg, n_free + 1
        elif (y[t] > 0 and a <= 0.0) or (y[t] < 0 and a >= C):
            ub = min(ub, yg)
        else:
            lb = max(lb, yg)
        obj = obj + a * (float(g[t]) - 1.0)
    if n_free:
        BRANCHES["rho_free"] += 1
        rho = sum_free / n_free
    else:
        BRANCHES["rho_midpoint"] += 1
        rho = (ub + lb) / 2.0
    if np.count_nonzero(alpha >= C) >= 2:
        BRANCHES["two_at_C"] += 1
    return {"alpha": alpha, "g": g, "rho": rho, "objective": obj / 2.0, "iterations": iterations, "converged": converged}


def weights(samples, rows, y, alpha):
    w = np.zeros(NFEAT)
    for t in range(len(rows)):
        if alpha[t] > 0.0:
            w = w + (float(y[t]) * float(alpha[t])) * np.asarray(samples[rows[t]], np.uint8).astype(np.float64)
    return w.astype(np.float32)


def decision_values(W, rho, rows_u8):
    """W f32 [n_df, 1200], rho [n_df], rows uint8 [n, 1200] -> fp64 [n, n_df]"""
    f = np.asarray(rows_u8, np.uint8).astype(np.float32).reshape(-1, 1, NFEAT // 4, 4)
    w = np.asarray(W, np.float32).reshape(1, -1, NFEAT // 4, 4)
    p = w * f                                                 # f32 products
    q = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]     # f32, left to right
    assert q.dtype == np.float32
    s = np.cumsum(q.astype(np.float64), axis=-1)[..., -1]     # sequential fp64 accumulation in feature order
    kval = s.astype(np.float32)
    return -np.asarray(rho, np.float64)[None, :] + kval.astype(np.float64)


def predict(W, rho, n_class, rows_u8):
    """-> class indices"""
    d = decision_values(W, rho, rows_u8)
    out = np.zeros(len(d), np.int64)
    for r in range(len(d)):
        votes = [0] * n_class
        for k, (i, j) in enumerate(pairs(n_class)):
            votes[i if d[r, k] > 0 else j] += 1
        out[r] = votes.index(max(votes))
    return out


def train_set(samples, cls, G, n_class, keep, C, eps, max_iter):
    """every pair problem over the rows where keep is true -> (W, rho, per-pair results, per-pair rows)"""
    W, rho, res, lists = [], [], [], []
    for i, j in pairs(n_class):
        rows = np.flatnonzero(keep & ((cls == i) | (cls == j)))
        y = np.where(cls[rows] == i, 1, -1)
        r = solve_pair(G, rows, y, C, eps, max_iter)
        W.append(weights(samples, rows, y, r["alpha"]))
        rho.append(r["rho"])
        res.append(r)
        lists.append(rows)
    return np.array(W, np.float32), np.array(rho), res, lists


def folds(n, k_fold, perm):
    perm = np.arange(n) if perm is None else np.asarray(perm)
    return [perm[(k * n) // k_fold:((k + 1) * n) // k_fold] for k in range(k_fold)]


def train_auto(samples, responses, perm=None, eps=1e-3, max_iter=1000, k_fold=10, c_grid=None):
    """-> dict(labels, W, rho, best_index, best_c, cv_errors, iterations, converged, objective, alpha [n_df, n])"""
    samples = np.asarray(samples, np.uint8)
    c_grid = default_params()["c_grid"] if c_grid is None else [float(c) for c in c_grid]
    labels, cls = class_table(responses)
    n, n_class = len(samples), len(labels)
    G = gram(samples)
    cv_errors, best = [-1] * len(c_grid), 0
    if k_fold > 1 and len(c_grid) > 1:
        cv_errors = []
        for C in c_grid:
            err = 0
            for test in folds(n, k_fold, perm):
                keep = np.ones(n, bool)
                keep[test] = False
                W, rho, _, _ = train_set(samples, cls, G, n_class, keep, C, eps, max_iter)
                if len(test):
                    err += int(np.count_nonzero(predict(W, rho, n_class, samples[test]) != cls[test]))
            cv_errors.append(err)
        best = cv_errors.index(min(cv_errors))               # the earlier entry on a tie
        if cv_errors.count(min(cv_errors)) > 1:
            BRANCHES["grid_tie"] += 1
    W, rho, res, lists = train_set(samples, cls, G, n_class, np.ones(n, bool), c_grid[best], eps, max_iter)
    alpha = np.zeros((len(res), n))
    for d, (r, rows) in enumerate(zip(res, lists)):
        alpha[d, rows] = r["alpha"]
    return {"labels": labels, "cls": cls, "W": W, "rho": rho, "best_index": best, "best_c": c_grid[best], "cv_errors": cv_errors,
            "iterations": [r["iterations"] for r in res], "converged": [r["converged"] for r in res], "objective": [r["objective"] for r in res],
            "alpha": alpha, "results": res, "lists": lists, "G": G}
