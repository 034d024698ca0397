"""The chessboard detector's rule (the text at the head of rmcv_amd/csrc/device_chess.h) restated in numpy and plain Python, written
from the text and not from the header's code: the response as whole-image array arithmetic, the candidates as a masked comparison with shifted
copies, the graph with sorted lists and sets, the labelling with dictionaries.  Python integers do not overflow, so every value is exact.
find() returns what rmcv_find_chessboard_host returns: (corners (cols rows, 2) float32 or None, the status word, candidates (n, 3) int32)."""
from collections import deque

import numpy as np

COUNT_MASK, FOUND, OVERFLOW, NO_GRID, CAND_MAX = 0x7FF, 1 << 11, 1 << 12, 1 << 13, 1024
DEFAULTS = dict(threshold=1000, contrast=10, nms=3, dist_min=6, dist_max=255)
RING = [(0, -5), (2, -5), (3, -3), (5, -2), (5, 0), (5, 2), (3, 3), (2, 5), (0, 5), (-2, 5), (-3, 3), (-5, 2), (-5, 0), (-5, -2), (-3, -3), (-2, -5)]


def gray(bgr):
    b, g, r = (bgr[:, :, c].astype(np.int64) for c in range(3))
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def shifted(img, dx, dy, fill=None):
    """img[y + dy, x + dx] for every (x, y): taps clamped into the image (fill None) or `fill` outside it"""
    h, w = img.shape
    m = max(abs(dx), abs(dy), 1)
    pad = np.pad(img, m, mode="edge") if fill is None else np.pad(img, m, mode="constant", constant_values=fill)
    return pad[m + dy:m + dy + h, m + dx:m + dx + w]


def response(g):
    ring = [shifted(g, dx, dy) for dx, dy in RING]
    sr = sum(np.abs((ring[n] + ring[n + 8]) - (ring[n + 4] + ring[n + 12])) for n in range(4))
    dr = sum(np.abs(ring[n] - ring[n + 8]) for n in range(8))
    loc = g + shifted(g, -1, 0) + shifted(g, 1, 0) + shifted(g, 0, -1) + shifted(g, 0, 1)
    out = 5 * sr - 5 * dr - np.abs(5 * sum(ring) - 16 * loc)
    h, w = g.shape
    ys, xs = np.mgrid[0:h, 0:w]
    out[(xs < 5) | (ys < 5) | (xs >= w - 5) | (ys >= h - 5)] = 0
    return out


def candidates(resp, threshold, nms):
    """(n, 3) int64 rows (x, y, R) in row-major order"""
    keep = resp > threshold
    for dy in range(-nms, nms + 1):
        for dx in range(-nms, nms + 1):
            if dx == 0 and dy == 0:
                continue
            other = shifted(resp, dx, dy, fill=-10 ** 9)       # (a pixel outside the image is no pixel of the neighbourhood)
            earlier = dy < 0 or (dy == 0 and dx < 0)
            keep &= ~((other > resp) | ((other == resp) & earlier))
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys, resp[ys, xs]], axis=1).astype(np.int64).reshape(-1, 3)


def box(g, x, y):
    h, w = g.shape
    return sum(int(g[min(max(y + v, 0), h - 1), min(max(x + u, 0), w - 1)]) for v in (-1, 0, 1) for u in (-1, 0, 1))


def edge_passes(g, P, a, b, contrast):
    p, q = (a, b) if a < b else (b, a)
    dx, dy = P[q][0] - P[p][0], P[q][1] - P[p][1]
    nx, ny = -dy, dx
    diffs = []
    for k in range(1, 8):
        lx, ly = 8 * P[p][0] + k * dx + nx, 8 * P[p][1] + k * dy + ny
        rx, ry = 8 * P[p][0] + k * dx - nx, 8 * P[p][1] + k * dy - ny
        diffs.append(box(g, (lx + 4) >> 3, (ly + 4) >> 3) - box(g, (rx + 4) >> 3, (ry + 4) >> 3))
    return all(d > 9 * contrast for d in diffs) or all(d < -9 * contrast for d in diffs)


def neighbours(g, P, contrast, dist_min, dist_max):
    n = len(P)
    arr = np.array(P, np.int64).reshape(-1, 2)
    accepted = []
    for a in range(n):
        d2 = ((arr - arr[a]) ** 2).sum(axis=1)
        near = sorted((int(d2[b]), b) for b in range(n) if b != a and dist_min ** 2 <= d2[b] <= dist_max ** 2)[:8]
        acc = []
        for _, b in near:
            if len(acc) < 4 and edge_passes(g, P, a, b, contrast):
                acc.append(b)
        accepted.append(acc)
    return [sorted(b for b in accepted[a] if a in accepted[b]) for a in range(n)]


def sign(v):
    return 1 if v > 0 else -1


def attempt(P, nb, s, attempted, cols, rows):
    """the attempt seeded at s -> the board's candidates in row-major order, or None"""
    lab, u = {s: (0, 0)}, {s: (P[nb[s][0]][0] - P[s][0], P[nb[s][0]][1] - P[s][1])}
    attempted.add(s)
    queue, failed = deque([s]), False
    while queue:
        c = queue.popleft()
        for r in nb[c]:
            e = (P[r][0] - P[c][0], P[r][1] - P[c][1])
            dot, cr = u[c][0] * e[0] + u[c][1] * e[1], u[c][0] * e[1] - u[c][1] * e[0]
            if abs(dot) >= abs(cr):
                sg = sign(dot)
                l, d = (lab[c][0] + sg, lab[c][1]), (sg * e[0], sg * e[1])
            else:
                sg = sign(cr)
                l, d = (lab[c][0], lab[c][1] + sg), (sg * e[1], -sg * e[0])
            if r in lab:
                failed |= lab[r] != l
                continue
            lab[r], u[r] = l, d
            attempted.add(r)
            queue.append(r)
    if failed or len(lab) != cols * rows or len(set(lab.values())) != len(lab):
        return None
    mi, mj = min(l[0] for l in lab.values()), min(l[1] for l in lab.values())
    at = {(l[0] - mi, l[1] - mj): node for node, l in lab.items()}
    ex, ey = 1 + max(k[0] for k in at), 1 + max(k[1] for k in at)
    if (ex, ey) not in ((cols, rows), (rows, cols)):
        return None
    choices = []
    for swap in (False, True):
        if ((ey, ex) if swap else (ex, ey)) != (cols, rows):
            continue
        for flip_i in (False, True):
            for flip_j in (False, True):
                def node(i, j):
                    i, j = (cols - 1 - i if flip_i else i), (rows - 1 - j if flip_j else j)
                    return at[(j, i) if swap else (i, j)]
                o, a, b = P[node(0, 0)], P[node(1, 0)], P[node(0, 1)]
                if (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]) > 0:
                    choices.append(((o[0] + o[1], o[1]), [node(i, j) for j in range(rows) for i in range(cols)]))
    if not choices:
        return None
    assert len(set(c[0] for c in choices)) == len(choices)      # (two orientations never tie: they start at different corners)
    return min(choices, key=lambda c: c[0])[1]


def find(bgr, cols, rows, threshold=1000, contrast=10, nms=3, dist_min=6, dist_max=255):
    g = gray(np.asarray(bgr))
    cand = candidates(response(g), threshold, nms)
    count = min(len(cand), COUNT_MASK)
    if len(cand) > CAND_MAX:
        return None, count | OVERFLOW, np.zeros((0, 3), np.int32)
    P = [(int(x), int(y)) for x, y, _ in cand]
    nb = neighbours(g, P, contrast, dist_min, dist_max)
    attempted = set()
    for s in range(len(P)):
        if s in attempted or not nb[s]:
            continue
        order = attempt(P, nb, s, attempted, cols, rows)
        if order is not None:
            return np.array([P[i] for i in order], np.float32), count | FOUND, cand.astype(np.int32)
    return None, count | NO_GRID, cand.astype(np.int32)
