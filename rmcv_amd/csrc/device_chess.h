// device_chess.h -- the chessboard detector: the step in front of the corner refinement in executable/calibration/hand_eye.cpp
// (findChessboardCorners, :119).  OpenCV's detector is not restated: this text is the rule, in integer arithmetic throughout, one source for
// rmcv_find_chessboard_host (the sequential form, this file) and k_chess_response / k_chess_grid (k_chess.hip), which agree byte for byte.
//
// Gray.   (1868 B + 9617 G + 4899 R + 8192) >> 14 of SRC(f), the BGR image a frame's results are defined on (device_corner.h's accessor over
//         source_view_plan.h's five kinds of source).  Every tap is clamped into the image.
// 1. Response (ChESS, Bennett and Lasenby, scaled by 5 to stay integer).  The ring I_0 .. I_15 lies at (dx, dy) = (0,-5) (2,-5) (3,-3) (5,-2)
//         (5,0) (5,2) (3,3) (2,5) (0,5) (-2,5) (-3,3) (-5,2) (-5,0) (-5,-2) (-3,-3) (-2,-5).  SR = sum over n = 0..3 of
//         |(I_n + I_{n+8}) - (I_{n+4} + I_{n+12})|, DR = sum over n = 0..7 of |I_n - I_{n+8}|, ring = sum of the I_n, loc = the centre pixel plus
//         its 4-neighbours; R = 5 SR - 5 DR - |5 ring - 16 loc| in int32 (it lies in -30600 .. 10200).  R = 0 for x < 5, y < 5, x >= w - 5 or
//         y >= h - 5.
// 2. Candidates.  A pixel with R > threshold such that no other pixel of its (2 nms + 1)^2 neighbourhood, clipped to the image, has a larger R
//         or an equal R and an earlier place in row-major order.  Candidates are indexed in row-major order (y, then x).  More than
//         RMCV_CHESS_CAND_MAX of them: status OVERFLOW, no board and no candidate list.  The status word's count is min(candidates, 2047).
// 3. Neighbour graph.  For candidate a: the (at most) 8 other candidates b with the smallest key (d2 << 10 | b), d2 = |P[b] - P[a]|^2, among
//         those with dist_min^2 <= d2 <= dist_max^2.  In ascending key they take the edge test, and a accepts the first (at most) 4 that pass.
//         The edge test of the unordered pair, from the lower index p to the higher q: d = P[q] - P[p], n = (-d.y, d.x); for k = 1..7 the two
//         points 8 P[p] + k d + n and 8 P[p] + k d - n in eighths of a pixel, each rounded to a pixel with (v + 4) >> 3 (arithmetic shift),
//         and the 3 x 3 clamped gray box sums L_k, R_k there.  The pair passes if all seven L_k - R_k > 9 contrast or all seven < -9 contrast.
//         a and b are neighbours iff each accepted the other; a's neighbours are held in ascending index.
// 4. Labelling (sequential).  Every candidate s in ascending index that has a neighbour and was not labelled by an earlier attempt seeds an
//         attempt: lab[s] = (0, 0), u[s] = P[s's first neighbour] - P[s], then a FIFO breadth-first search, neighbours in ascending index.
//         For neighbour r of c: e = P[r] - P[c], dot = u[c] . e, cr = u[c].x e.y - u[c].y e.x; |dot| >= |cr|: sg = sign(dot),
//         lab = lab[c] + (sg, 0), u = sg e; otherwise sg = sign(cr), lab = lab[c] + (0, sg), u = sg (e.y, -e.x).  An r not yet labelled takes
//         lab and u and joins the queue; an r labelled otherwise marks the attempt failed, and the search runs on to the end of the component
//         (every node of it counts as attempted).  The attempt also fails if the component has not exactly cols rows nodes, if the extents of
//         its labels are neither (cols, rows) nor (rows, cols), if two nodes share a label, or if no orientation below is right-handed.
//         Orientation: labels shifted so that both minima are 0; of the 8 maps t = 0..7 (bit 0: swap the axes, bit 1: flip i, bit 2: flip j)
//         those whose extents are (cols, rows) and with cross(P[1,0] - P[0,0], P[0,1] - P[0,0]) > 0; of them the one whose P[0,0] has the
//         smallest x + y, then the smallest y (the lowest t if both tie).  The first attempt that passes is the board; none: status NO_GRID.
// 5. Output.  cols rows corners in row-major order (j cols + i), floats (x, y) holding the integer pixel positions, in SRC(f)'s coordinates.
//         A frame without a board leaves its corner row untouched.
#pragma once
#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "device_corner.h"

#if defined(__HIPCC__)
#define CHESS_FN __host__ __device__ static inline
#else
#define CHESS_FN static inline
#endif

namespace rmcv {

static constexpr int CHESS_RING = 5;     // the ring's radius: R = 0 closer than this to an image edge
static constexpr int CHESS_NEAR = 8;     // nearest others that take the edge test
static constexpr int CHESS_DEGREE = 4;   // neighbours a candidate accepts

CHESS_FN int chess_abs(int v) { return v < 0 ? -v : v; }
CHESS_FN int chess_x(uint32_t key) { return (int)(key & 0xFFFFu); }
CHESS_FN int chess_y(uint32_t key) { return (int)(key >> 16); }
CHESS_FN uint32_t chess_key(int x, int y) { return ((uint32_t)y << 16) | (uint32_t)x; }

// acc + |a - b| for 0 <= a, b (one instruction on the device)
CHESS_FN int chess_sad(int a, int b, int acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__usad((unsigned)a, (unsigned)b, (unsigned)acc);
#else
    return acc + chess_abs(a - b);
#endif
}
// R from the gray of the centre's surroundings: g(dx, dy).  p_n = I_n + I_{n+8}: SR = sum |p_n - p_{n+4}|, ring = sum p_n
template <class Gray>
CHESS_FN int chess_response(Gray g)
{
    const int i0 = g(0, -5), i1 = g(2, -5), i2 = g(3, -3), i3 = g(5, -2), i4 = g(5, 0), i5 = g(5, 2), i6 = g(3, 3), i7 = g(2, 5);
    const int i8 = g(0, 5), i9 = g(-2, 5), i10 = g(-3, 3), i11 = g(-5, 2), i12 = g(-5, 0), i13 = g(-5, -2), i14 = g(-3, -3), i15 = g(-2, -5);
    const int p0 = i0 + i8, p1 = i1 + i9, p2 = i2 + i10, p3 = i3 + i11, p4 = i4 + i12, p5 = i5 + i13, p6 = i6 + i14, p7 = i7 + i15;
    const int sr = chess_sad(p3, p7, chess_sad(p2, p6, chess_sad(p1, p5, chess_sad(p0, p4, 0))));
    const int dr = chess_sad(i7, i15, chess_sad(i6, i14, chess_sad(i5, i13, chess_sad(i4, i12, chess_sad(i3, i11, chess_sad(i2, i10, chess_sad(i1, i9, chess_sad(i0, i8, 0))))))));
    const int ring = p0 + p1 + p2 + p3 + p4 + p5 + p6 + p7;
    const int loc = g(0, 0) + g(-1, 0) + g(1, 0) + g(0, -1) + g(0, 1);
    return 5 * sr - 5 * dr - chess_abs(5 * ring - 16 * loc);
}
CHESS_FN bool chess_inside_ring(int x, int y, int w, int h) { return x >= CHESS_RING && y >= CHESS_RING && x < w - CHESS_RING && y < h - CHESS_RING; }
// does the neighbour at (dx, dy) with response `other` disqualify a pixel with response `mine`
CHESS_FN bool chess_beaten(int mine, int other, int dx, int dy) { return other > mine || (other == mine && (dy < 0 || (dy == 0 && dx < 0))); }

// the key a orders b by, or -1 where b is no partner of a
CHESS_FN int32_t chess_near_key(uint32_t pa, uint32_t pb, int a, int b, int dmin2, int dmax2)
{
    const int dx = chess_x(pb) - chess_x(pa), dy = chess_y(pb) - chess_y(pa);
    const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy;
    if (a == b || d2 < dmin2 || d2 > dmax2) return -1;
    return (int32_t)((d2 << 10) | b);
}

// L_k - R_k of the edge test from p to q (p the lower index); at(x, y): clamped gray
template <class At>
CHESS_FN int chess_edge_diff(At at, uint32_t p, uint32_t q, int k)
{
    const int dx = chess_x(q) - chess_x(p), dy = chess_y(q) - chess_y(p);
    const int bx = 8 * chess_x(p) + k * dx, by = 8 * chess_y(p) + k * dy;
    const int lx = (bx - dy + 4) >> 3, ly = (by + dx + 4) >> 3, rx = (bx + dy + 4) >> 3, ry = (by - dx + 4) >> 3;
    int diff = 0;
    for (int v = -1; v <= 1; v++)
        for (int u = -1; u <= 1; u++) diff += at(lx + u, ly + v) - at(rx + u, ry + v);
    return diff;
}

// ---- the labelling on tables of n <= RMCV_CHESS_CAND_MAX candidates.  key[n]: sorted; adj[n][4]: neighbours, ascending, -1 behind the last;
// lab[n][2], u[n][2], queue[n], seen[n], grid[cols rows]: working tables; order[cols rows]: the candidate at (i, j) in j cols + i.  True: a board
struct ChessTables {
    const uint32_t* key;
    const int16_t* adj;
    int16_t *lab, *u, *queue, *grid, *order;
    uint8_t* seen;
};
CHESS_FN int chess_oriented(const ChessTables& T, int t, int i, int j, int cols, int rows, int ex)
{
    if (t & 2) i = cols - 1 - i;
    if (t & 4) j = rows - 1 - j;
    return (t & 1) ? T.grid[i * ex + j] : T.grid[j * ex + i];
}
CHESS_FN bool chess_label(const ChessTables& T, int n, int cols, int rows)
{
    const int want = cols * rows;
    for (int i = 0; i < n; i++) T.seen[i] = 0;
    for (int s = 0; s < n; s++) {
        if (T.seen[s] || T.adj[4 * s] < 0) continue;
        int head = 0, tail = 0, min_i = 0, max_i = 0, min_j = 0, max_j = 0;
        bool ok = true;
        const int first = T.adj[4 * s];
        T.seen[s] = 1;
        T.lab[2 * s] = T.lab[2 * s + 1] = 0;
        T.u[2 * s] = (int16_t)(chess_x(T.key[first]) - chess_x(T.key[s]));
        T.u[2 * s + 1] = (int16_t)(chess_y(T.key[first]) - chess_y(T.key[s]));
        T.queue[tail++] = (int16_t)s;
        while (head < tail) {
            const int c = T.queue[head++];
            const int ux = T.u[2 * c], uy = T.u[2 * c + 1];
            for (int t = 0; t < CHESS_DEGREE; t++) {
                const int r = T.adj[4 * c + t];
                if (r < 0) break;
                const int ex = chess_x(T.key[r]) - chess_x(T.key[c]), ey = chess_y(T.key[r]) - chess_y(T.key[c]);
                const int dot = ux * ex + uy * ey, cr = ux * ey - uy * ex;
                int li = T.lab[2 * c], lj = T.lab[2 * c + 1], nx, ny;
                if (chess_abs(dot) >= chess_abs(cr)) {
                    const int sg = dot > 0 ? 1 : -1;
                    li += sg; nx = sg * ex; ny = sg * ey;
                } else {
                    const int sg = cr > 0 ? 1 : -1;
                    lj += sg; nx = sg * ey; ny = -sg * ex;
                }
                if (T.seen[r]) {
                    if (T.lab[2 * r] != li || T.lab[2 * r + 1] != lj) ok = false;
                    continue;
                }
                T.seen[r] = 1;
                T.lab[2 * r] = (int16_t)li; T.lab[2 * r + 1] = (int16_t)lj;
                T.u[2 * r] = (int16_t)nx; T.u[2 * r + 1] = (int16_t)ny;
                T.queue[tail++] = (int16_t)r;
                min_i = li < min_i ? li : min_i; max_i = li > max_i ? li : max_i;
                min_j = lj < min_j ? lj : min_j; max_j = lj > max_j ? lj : max_j;
            }
        }
        const int ex = max_i - min_i + 1, ey = max_j - min_j + 1;
        if (!ok || tail != want || !((ex == cols && ey == rows) || (ex == rows && ey == cols))) continue;
        for (int g = 0; g < want; g++) T.grid[g] = -1;
        for (int q = 0; q < tail; q++) {
            const int node = T.queue[q], g = (T.lab[2 * node + 1] - min_j) * ex + (T.lab[2 * node] - min_i);
            if (T.grid[g] >= 0) ok = false;
            T.grid[g] = (int16_t)node;
        }
        if (!ok) continue;
        int best = -1, best_sum = 0, best_y = 0;
        for (int t = 0; t < 8; t++) {
            if (((t & 1) ? ey : ex) != cols || ((t & 1) ? ex : ey) != rows) continue;
            const uint32_t p00 = T.key[chess_oriented(T, t, 0, 0, cols, rows, ex)], p10 = T.key[chess_oriented(T, t, 1, 0, cols, rows, ex)],
                           p01 = T.key[chess_oriented(T, t, 0, 1, cols, rows, ex)];
            const int ax = chess_x(p10) - chess_x(p00), ay = chess_y(p10) - chess_y(p00), bx = chess_x(p01) - chess_x(p00), by = chess_y(p01) - chess_y(p00);
            if (!(ax * by - ay * bx > 0)) continue;
            const int sum = chess_x(p00) + chess_y(p00), y = chess_y(p00);
            if (best < 0 || sum < best_sum || (sum == best_sum && y < best_y)) { best = t; best_sum = sum; best_y = y; }
        }
        if (best < 0) continue;
        for (int j = 0; j < rows; j++)
            for (int i = 0; i < cols; i++) T.order[j * cols + i] = (int16_t)chess_oriented(T, best, i, j, cols, rows, ex);
        return true;
    }
    return false;
}

CHESS_FN int32_t chess_status(int64_t candidates, int flag) { return (int32_t)(candidates > RMCV_CHESS_COUNT_MASK ? RMCV_CHESS_COUNT_MASK : candidates) | flag; }

// ---- the host form: a BGR image, rows `stride` bytes apart; the sequential statement of the rule.  corners_out: cols rows x 2 floats, written
// when a board is found; cand_out (nullable): RMCV_CHESS_CAND_MAX x (x, y, R), the first *cand_n_out rows written ----
static inline void chess_find_host(const uint8_t* bgr, int w, int h, int stride, int cols, int rows, const rmcv_chess_params& prm, float* corners_out,
                                   int32_t* status_out, int32_t* cand_out, int32_t* cand_n_out)
{
    const int nms = prm.nms;
    uint8_t* gray = new uint8_t[(size_t)w * h];
    int32_t* resp = new int32_t[(size_t)w * h];
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) gray[(size_t)y * w + x] = (uint8_t)corner_gray_host_at(bgr, w, h, stride, x, y);
    auto at = [&](int x, int y) { return (int)gray[(size_t)corner_clamp(y, h) * w + corner_clamp(x, w)]; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            resp[(size_t)y * w + x] = chess_inside_ring(x, y, w, h) ? chess_response([&](int dx, int dy) { return at(x + dx, y + dy); }) : 0;
    uint32_t* key = new uint32_t[RMCV_CHESS_CAND_MAX];
    int32_t* val = new int32_t[RMCV_CHESS_CAND_MAX];
    int64_t total = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int mine = resp[(size_t)y * w + x];
            if (!(mine > prm.threshold)) continue;
            bool keep = true;
            for (int dy = -nms; dy <= nms && keep; dy++)
                for (int dx = -nms; dx <= nms && keep; dx++) {
                    if ((dx == 0 && dy == 0) || x + dx < 0 || x + dx >= w || y + dy < 0 || y + dy >= h) continue;
                    keep = !chess_beaten(mine, resp[(size_t)(y + dy) * w + x + dx], dx, dy);
                }
            if (!keep) continue;
            if (total < RMCV_CHESS_CAND_MAX) { key[total] = chess_key(x, y); val[total] = mine; }
            total++;
        }
    delete[] resp;
    int32_t status = 0;
    int n = (int)total;
    if (total > RMCV_CHESS_CAND_MAX) {
        status = chess_status(total, RMCV_CHESS_OVERFLOW);
        n = 0;
    } else {
        int16_t* acc = new int16_t[4 * RMCV_CHESS_CAND_MAX];
        int16_t* tab = new int16_t[4 * RMCV_CHESS_CAND_MAX + 2 * RMCV_CHESS_CAND_MAX + 2 * RMCV_CHESS_CAND_MAX + 3 * RMCV_CHESS_CAND_MAX];
        uint8_t* seen = new uint8_t[RMCV_CHESS_CAND_MAX];
        const int dmin2 = prm.dist_min * prm.dist_min, dmax2 = prm.dist_max * prm.dist_max;
        for (int a = 0; a < n; a++) {
            int32_t last = -1;
            int got = 0;
            for (int t = 0; t < CHESS_DEGREE; t++) acc[4 * a + t] = -1;
            for (int round = 0; round < CHESS_NEAR && got < CHESS_DEGREE; round++) {
                int32_t best = INT32_MAX;
                for (int b = 0; b < n; b++) {
                    const int32_t k = chess_near_key(key[a], key[b], a, b, dmin2, dmax2);
                    if (k > last && k < best) best = k;
                }
                if (best == INT32_MAX) break;
                last = best;
                const int b = best & 1023, p = a < b ? a : b, q = a < b ? b : a;
                bool pos = true, neg = true;
                for (int k = 1; k <= 7; k++) {
                    const int diff = chess_edge_diff(at, key[p], key[q], k);
                    pos = pos && diff > 9 * prm.contrast;
                    neg = neg && diff < -9 * prm.contrast;
                }
                if (pos || neg) acc[4 * a + got++] = (int16_t)b;
            }
        }
        int16_t* adj = tab;
        for (int a = 0; a < n; a++) {
            int deg = 0;
            for (int t = 0; t < CHESS_DEGREE; t++) {
                const int b = acc[4 * a + t];
                bool mutual = false;
                for (int s = 0; b >= 0 && s < CHESS_DEGREE; s++) mutual = mutual || acc[4 * b + s] == a;
                if (!mutual) continue;
                int at_ = deg++;
                for (; at_ > 0 && adj[4 * a + at_ - 1] > b; at_--) adj[4 * a + at_] = adj[4 * a + at_ - 1];
                adj[4 * a + at_] = (int16_t)b;
            }
            for (int t = deg; t < CHESS_DEGREE; t++) adj[4 * a + t] = -1;
        }
        ChessTables T;
        T.key = key; T.adj = adj; T.seen = seen;
        T.lab = tab + 4 * RMCV_CHESS_CAND_MAX; T.u = T.lab + 2 * RMCV_CHESS_CAND_MAX; T.queue = T.u + 2 * RMCV_CHESS_CAND_MAX;
        T.grid = T.queue + RMCV_CHESS_CAND_MAX; T.order = T.grid + RMCV_CHESS_CAND_MAX;
        const bool found = chess_label(T, n, cols, rows);
        if (found)
            for (int g = 0; g < cols * rows; g++) {
                corners_out[2 * g] = (float)chess_x(key[T.order[g]]);
                corners_out[2 * g + 1] = (float)chess_y(key[T.order[g]]);
            }
        status = chess_status(total, found ? RMCV_CHESS_FOUND : RMCV_CHESS_NO_GRID);
        delete[] seen;
        delete[] tab;
        delete[] acc;
    }
    if (cand_out)
        for (int i = 0; i < n; i++) {
            cand_out[3 * i] = chess_x(key[i]);
            cand_out[3 * i + 1] = chess_y(key[i]);
            cand_out[3 * i + 2] = val[i];
        }
    if (cand_n_out) *cand_n_out = n;
    if (status_out) *status_out = status;
    delete[] val;
    delete[] key;
    delete[] gray;
}

} // namespace rmcv
