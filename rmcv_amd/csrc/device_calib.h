// device_calib.h -- the calibration solve: camera matrix and distortion from chessboard views, the library's pinned statement
// of cv::calibrateCamera as executable/calibration/hand_eye.cpp:128-131 calls it.  One source for rmcv_calibrate_camera_host (the sequential
// form: CalibHostExec below) and the kernels k_calib_homography / k_calib_solve (k_calib.hip), which agree bit for bit.  OpenCV is not the
// reference here: this text is, and DESIGN.md 4u lists where it knowingly departs.  Everything is double, built with -ffp-contract=off;
// every expression is evaluated as written, left to right; between the input and the final intrinsics only + - x / and sqrt occur.
//
// Input.  corners float [n_views][per_frame][2], counts int32 [n_views]; a cols x rows pattern, P = cols rows; square; the image (w, h);
//         view_camera int32 [n_views] or null (camera 0); a value outside 0 .. n_cameras - 1 is camera 0 (frame_camera_eff).  Object point k
//         is (X, Y) = ((k % cols) square, (k / cols) square), Z = 0.  View v is USED iff counts[v] == P and its 2 P floats are finite.  A camera's
//         used views are taken in ascending v.  Fewer than 3: TOO_FEW_VIEWS; more than 256: TOO_MANY_VIEWS; outputs untouched but for the
//         result's status, views_used and iters (0).
// Sums.   Every sum over a view's points is a WAVE SUM: partial l (0 .. 63) takes the points k % 64 == l in ascending k, starting from 0.0;
//         then acc[l] = acc[l] + acc[l ^ s] for s = 32, 16, 8, 4, 2, 1, all 64 at once per s.  Every sum over views runs over the camera's used
//         views in ascending order, sequentially, starting from 0.0.
// 1 Homography (per used view).  Hartley: m = (sum x / P, sum y / P) (a wave sum of two), d = (sum sqrt((x - mx)^2 + (y - my)^2)) / P,
//         s = 1.4142135623730951 / d, point = ((x - mx) s, (y - my) s); for the object points (X, Y) and the image points (u, v) alike.
//         Rows r1 = (-X, -Y, -1, 0, 0, 0, u X, u Y, u), r2 = (0, 0, 0, -X, -Y, -1, v X, v Y, v); A[i][j] = wave sum of r1[i] r1[j] + r2[i] r2[j],
//         45 sums (i <= j), mirrored.  Cyclic Jacobi on A (9 x 9), V = I: at most 30 sweeps, a sweep runs (p, q), p < q, row-major; before a
//         sweep off = sum |A[p][q]| in that order, off == 0 ends.  A pair with apq == 0 is skipped; |apq| < 1e-300 or
//         |apq| <= 1.1102230246251565e-16 x 1e-3 x sqrt(|app aqq|) sets apq = 0 and is skipped; otherwise theta = (aqq - app) / (2 apq),
//         t = 1 / (|theta| + sqrt(theta theta + 1)), negated for theta < 0, c = 1 / sqrt(t t + 1), s = t c; app -= t apq, aqq += t apq, apq = 0;
//         for r != p, q: (A[r][p], A[r][q]) = (c arp - s arq, s arp + c arq), mirrored; for every r the same on (V[r][p], V[r][q]).  The
//         eigenvector: column m of V, m the first index of the smallest A[m][m].  Denormalise: G[r][0] = e[r][0] so, G[r][1] = e[r][1] so,
//         G[r][2] = e[r][2] - (G[r][0] mox + G[r][1] moy); H row 0 = G row 0 / si + miu G row 2, row 1 = G row 1 / si + miv G row 2, row 2 = G
//         row 2; then every entry is divided by H[8].
// 2 Initial intrinsics (per camera).  cx = (w - 1) / 2, cy = (h - 1) / 2.  Per view the centred H: rows 0, 1 minus cx, cy times row 2; h, v
//         its first two columns, d1 = (h + v) 0.5, d2 = (h - v) 0.5, each of the four scaled by 1 / sqrt(sum of squares).  Two equations in
//         n = (1 / fx^2, 1 / fy^2): (h0 v0, h1 v1) n = -(h2 v2), then (d1_0 d2_0, d1_1 d2_1) n = -(d1_2 d2_2).  Normal equations summed over
//         views (first equation, then second): a00, a01, a11, b0, b1; det = a00 a11 - a01 a01, n0 = (a11 b0 - a01 b1) / det,
//         n1 = (a00 b1 - a01 b0) / det, f = sqrt(|1 / n|).  Distortion 0.  A guess (fx != 0) replaces all nine.  f not finite or <= 0: BAD_INIT.
// 3 Initial pose (per view).  M rows: (H row 0 - cx H row 2) / fx, (H row 1 - cy H row 2) / fy, H row 2.  k = 1 / |column 0|, negated when
//         M[2][2] k < 0.  r0 = column 0 times k, b = column 1 times k, t = column 2 times k; b -= (r0 . b) r0, r1 = b / |b|, r2 = r0 x r1.
//         R = (r0 r1 r2) to a quaternion (w, x, y, z) by the first largest of (trace, R00, R11, R22), s = 2 sqrt(1 + ..), then divided by
//         its norm.  The pose is (q, t) from here on.
// 4 Levenberg-Marquardt over a = (fx fy cx cy k1 k2 p1 p2 k3) and, per view, b = (omega, delta t).  Model and Jacobian: calib_project,
//         calib_jacobian below, as written.  Bit j of fix_mask zeroes column j.  Per view the wave sums of the upper triangle of J^T J (15 x 15:
//         U, W, V), of J^T r (ga, gb) and of the cost r.r: term(i, j) = ju[i] ju[j] + jv[i] jv[j], gradient ju[i] ru + jv[i] rv, cost
//         ru ru + rv rv.  lambda = 1e-3.  A trial (each counts one iteration; blocks are of the current state):
//         per view: Cholesky of V with its diagonal times (1 + lambda) (calib_chol: rows ascending, columns ascending, a pivot not > 0 or not
//         finite rejects the trial); Y = W Vd^-1 row by row, z = Vd^-1 gb (calib_chol_solve); T(i, j) = U(i, j) [times (1 + lambda) on the
//         diagonal] - sum_m Y[i][m] W[j][m]; e_i = ga_i - sum_m W[i][m] z_m.  Per camera: S = sum T, rs = sum e over views; a fixed j gets
//         S[j][j] = 1, rs_j = 0; Cholesky of S; da = -(S^-1 rs).  Per view: db_m = -(z_m + sum_i Y[i][m] da_i);
//         q' = ((1, omega / 2) (x) q) / norm, t' = t + dt.  a' = a + da.  cost' = sum over views of the trial's cost.
//         |d|^2 = sum da^2 + sum_views sum db^2, |p|^2 = sum a^2 + sum_views (q.q + t.t) (of the state before the step).
//         Accepted iff no pivot failed and cost' is finite and < cost: state = trial, lambda /= 10, and |d|^2 <= eps^2 |p|^2 ends with
//         CONVERGED.  Otherwise lambda *= 10, and lambda > 1e12 ends with STALLED.  iters == max_iters before a trial ends with MAX_ITERS.
//         The initial cost not finite: BAD_INIT.
// 5 Output.  Result: camera_matrix (fx 0 cx; 0 fy cy; 0 0 1), dist, rms = sqrt(cost / (P views)), rms_init, views_used, iters, status.
//         View: q as carried; for rvec (w, v) is negated when w < 0, n = |v|; n < FLT_EPSILON: rvec = 0; else rvec = v (2 pm_atan2(n, w) / n);
//         tvec; rms = sqrt(view cost / P); used = 1; the reserved words 0.  Rows of views not used, or of a camera without a solution, are not touched.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "calib_plan.h"
#include "pinned_math.h"

#if defined(__HIPCC__)
#define CALIB_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define CALIB_FN static inline __attribute__((always_inline))
#endif

namespace rmcv {

// one call's tables; on the device every pointer is device memory
struct CalibJob {
    const float* corners;        // [n_views][per_frame][2]
    const int32_t* counts;       // [n_views]
    const int32_t* view_camera;  // [n_views] nullable
    const rmcv_calib_guess* guesses; // [n_cameras] nullable; fx == 0: none for that camera
    double* ws;                  // [n_views][CALIB_VIEW_WS]
    int32_t* vcam;               // [n_views] the view's effective camera, -1 for a view not used
    rmcv_calib_result* results;  // [n_cameras]
    rmcv_calib_view* views;      // [n_views]
    double square, eps;
    int per_frame, n_views, n_cameras, cols, rows, w, h, max_iters, fix_mask;
};

// a camera's state: LDS on the device
struct CalibCam {
    double a[9], at[9], da[9], S[81], rs[9];
    double lambda, cost, cost_t, dn, pn, rms_init;
    int32_t nused, iters, status, ok, done;
};

CALIB_FN bool calib_finite(double v)
{
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return (u & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
CALIB_FN bool calib_finite_f(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}
CALIB_FN double calib_abs(double v) { return v < 0 ? -v : v; }
CALIB_FN int calib_hidx(int i, int j) { return i * 15 - i * (i - 1) / 2 + (j - i); }   // the upper triangle of the 15 x 15 J^T J, i <= j

// ---- the model ----
// R00 R01 R10 R11 R20 R21 of the unit quaternion (w, x, y, z): the board has Z = 0
CALIB_FN void calib_rot6(const double* q, double* R)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * y + w * z);
    R[3] = 1.0 - 2.0 * (x * x + z * z);
    R[4] = 2.0 * (x * z - w * y);
    R[5] = 2.0 * (y * z + w * x);
}
struct CalibProj {
    double rx, ry, rz, iz, x, y, xx, yy, xy, r2, rad, xd, yd;
};
CALIB_FN void calib_project(const double* a, const double* R, const double* t, double X, double Y, CalibProj& p)
{
    p.rx = R[0] * X + R[1] * Y;
    p.ry = R[2] * X + R[3] * Y;
    p.rz = R[4] * X + R[5] * Y;
    const double xc = p.rx + t[0], yc = p.ry + t[1], zc = p.rz + t[2];
    p.iz = 1.0 / zc;
    p.x = xc * p.iz;
    p.y = yc * p.iz;
    p.xx = p.x * p.x;
    p.yy = p.y * p.y;
    p.xy = p.x * p.y;
    p.r2 = p.xx + p.yy;
    p.rad = 1.0 + p.r2 * (a[4] + p.r2 * (a[5] + p.r2 * a[8]));
    p.xd = p.x * p.rad + (2.0 * a[6] * p.xy + a[7] * (p.r2 + 2.0 * p.xx));
    p.yd = p.y * p.rad + (a[6] * (p.r2 + 2.0 * p.yy) + 2.0 * a[7] * p.xy);
}
struct CalibPt {
    double ju[15], jv[15], ru, rv;
};
CALIB_FN void calib_residual(const double* a, const CalibProj& p, double uo, double vo, double& ru, double& rv)
{
    ru = (a[0] * p.xd + a[2]) - uo;
    rv = (a[1] * p.yd + a[3]) - vo;
}
CALIB_FN void calib_jacobian(const double* a, const CalibProj& p, int fix_mask, CalibPt& o)
{
    const double fx = a[0], fy = a[1], k1 = a[4], k2 = a[5], p1 = a[6], p2 = a[7], k3 = a[8];
    const double r4 = p.r2 * p.r2, r6 = r4 * p.r2;
    const double dr = k1 + p.r2 * (2.0 * k2 + 3.0 * k3 * p.r2);
    const double xdx = p.rad + 2.0 * p.xx * dr + 2.0 * p1 * p.y + 6.0 * p2 * p.x;
    const double xdy = 2.0 * p.xy * dr + 2.0 * p1 * p.x + 2.0 * p2 * p.y;
    const double ydy = p.rad + 2.0 * p.yy * dr + 6.0 * p1 * p.y + 2.0 * p2 * p.x;
    const double A0 = fx * (xdx * p.iz), A1 = fx * (xdy * p.iz), A2 = fx * (-(xdx * p.x + xdy * p.y) * p.iz);
    const double B0 = fy * (xdy * p.iz), B1 = fy * (ydy * p.iz), B2 = fy * (-(xdy * p.x + ydy * p.y) * p.iz);
    o.ju[0] = p.xd; o.ju[1] = 0.0; o.ju[2] = 1.0; o.ju[3] = 0.0;
    o.ju[4] = fx * (p.x * p.r2); o.ju[5] = fx * (p.x * r4); o.ju[6] = fx * (2.0 * p.xy); o.ju[7] = fx * (p.r2 + 2.0 * p.xx); o.ju[8] = fx * (p.x * r6);
    o.jv[0] = 0.0; o.jv[1] = p.yd; o.jv[2] = 0.0; o.jv[3] = 1.0;
    o.jv[4] = fy * (p.y * p.r2); o.jv[5] = fy * (p.y * r4); o.jv[6] = fy * (p.r2 + 2.0 * p.yy); o.jv[7] = fy * (2.0 * p.xy); o.jv[8] = fy * (p.y * r6);
    o.ju[9] = A2 * p.ry - A1 * p.rz; o.ju[10] = A0 * p.rz - A2 * p.rx; o.ju[11] = A1 * p.rx - A0 * p.ry;
    o.ju[12] = A0; o.ju[13] = A1; o.ju[14] = A2;
    o.jv[9] = B2 * p.ry - B1 * p.rz; o.jv[10] = B0 * p.rz - B2 * p.rx; o.jv[11] = B1 * p.rx - B0 * p.ry;
    o.jv[12] = B0; o.jv[13] = B1; o.jv[14] = B2;
#pragma unroll
    for (int j = 0; j < 9; j++)
        if ((fix_mask >> j) & 1) o.ju[j] = o.jv[j] = 0.0;
}

// ---- the per-view sums in passes: pass <R0, R1> holds rows R0 .. R1 - 1 of the upper triangle, their gradient entries and, in the first
// pass, the cost.  No pass holds more than CALIB_PASS_MAX sums per lane.
template <int R0, int R1>
struct CalibPass {
    static constexpr int NH = 15 * (R1 - R0) - (R1 * (R1 - 1) / 2 - R0 * (R0 - 1) / 2);
    static constexpr int N = NH + (R1 - R0) + (R0 == 0 ? 1 : 0);
    static_assert(N <= CALIB_PASS_MAX, "a pass holds at most CALIB_PASS_MAX sums per lane");
};
template <int R0, int R1>
CALIB_FN void calib_pass_add(const CalibPt& o, double* acc)
{
    int n = 0;
#pragma unroll
    for (int i = R0; i < R1; i++) {
#pragma unroll
        for (int j = i; j < 15; j++) {
            acc[n] = acc[n] + (o.ju[i] * o.ju[j] + o.jv[i] * o.jv[j]);
            n++;
        }
    }
#pragma unroll
    for (int i = R0; i < R1; i++) {
        acc[n] = acc[n] + (o.ju[i] * o.ru + o.jv[i] * o.rv);
        n++;
    }
    if (R0 == 0) acc[n] = acc[n] + (o.ru * o.ru + o.rv * o.rv);
}
// blk: 120 of the triangle, 15 of the gradient, the cost
template <int R0, int R1>
CALIB_FN void calib_pass_store(const double* acc, double* blk)
{
    int n = 0;
#pragma unroll
    for (int i = R0; i < R1; i++) {
#pragma unroll
        for (int j = i; j < 15; j++) blk[calib_hidx(i, j)] = acc[n++];
    }
#pragma unroll
    for (int i = R0; i < R1; i++) blk[120 + i] = acc[n++];
    if (R0 == 0) blk[135] = acc[n];
}

// ---- small dense algebra on memory (LDS or the workspace on the device): nothing here indexes a register array ----
// in place: the lower triangle of the n x n matrix at L (row pitch n) becomes its Cholesky factor; false: a pivot not > 0 or not finite
CALIB_FN bool calib_chol(double* L, int n)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            double s = L[i * n + j];
            for (int k = 0; k < j; k++) s = s - L[i * n + k] * L[j * n + k];
            if (i == j) {
                if (!(s > 0.0) || !calib_finite(s)) return false;
                L[i * n + i] = sqrt(s);
            } else
                L[i * n + j] = s / L[j * n + j];
        }
    return true;
}
// x = (L L^T)^-1 b; b and x may be the same
CALIB_FN void calib_chol_solve(const double* L, int n, const double* b, double* x)
{
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - L[i * n + k] * x[k];
        x[i] = s / L[i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i];
        for (int k = i + 1; k < n; k++) s = s - L[k * n + i] * x[k];
        x[i] = s / L[i * n + i];
    }
}

// ---- the sequential executor: what a wavefront, a workgroup and their barriers do, one after the other ----
struct CalibHostExec {
    double lds[CALIB_WAVE_LDS];
    // out[n] = the wave sum of what f(k, acc) adds for point k
    template <int N, class F>
    void wsum(int P, F f, double* out)
    {
        double acc[64][N];
        for (int l = 0; l < 64; l++) {
            for (int n = 0; n < N; n++) acc[l][n] = 0.0;
            for (int k = l; k < P; k += 64) f(k, acc[l]);
        }
        for (int s = 32; s >= 1; s >>= 1)
            for (int l = 0; l < s; l++)
                for (int n = 0; n < N; n++) acc[l][n] = acc[l][n] + acc[l ^ s][n];   // (lane l of the butterfly; lanes >= s are no longer read)
        for (int n = 0; n < N; n++) out[n] = acc[0][n];
    }
    double* wave_lds() { return lds; }
    template <class F> void lanes(int n, F f) { for (int i = 0; i < n; i++) f(i); }          // lane i < n runs f(i); then the wavefront meets
    template <class F> void each_view(int n, F f) { for (int i = 0; i < n; i++) f(i); }      // wavefronts take the views in turn; then a barrier
    template <class F> void each(int n, F f) { for (int i = 0; i < n; i++) f(i); }           // thread i < n runs f(i); then a barrier
};

// ---- the cyclic Jacobi of 1 on the symmetric N x N matrix at A, V = I on entry (both row pitch N, memory the whole wavefront sees): A's diagonal
// becomes the eigenvalues, V's columns the eigenvectors.  Every lane walks the sweeps; lane r takes row r of a rotation.  -> the sweeps begun
template <int N, class X>
CALIB_FN int calib_jacobi(X& x, double* A, double* V)
{
    int sweep = 0;
    for (; sweep < CALIB_JACOBI_SWEEPS; sweep++) {
        double off = 0.0;
        for (int p = 0; p < N; p++)
            for (int q = p + 1; q < N; q++) off += calib_abs(A[p * N + q]);
        if (off == 0.0) break;
        for (int p = 0; p < N; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];   // (every lane reads them before lane 0 writes)
                if (apq == 0.0) continue;
                const bool tiny = calib_abs(apq) < 1e-300 || calib_abs(apq) <= 1.1102230246251565e-16 * 1e-3 * sqrt(calib_abs(app * aqq));
                double cs = 1.0, sn = 0.0, t = 0.0;
                if (!tiny) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    t = 1.0 / (calib_abs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0) t = -t;
                    cs = 1.0 / sqrt(t * t + 1.0);
                    sn = t * cs;
                }
                x.lanes(N, [&](int r) {
                    if (tiny) {
                        if (r == 0) A[p * N + q] = A[q * N + p] = 0.0;
                        return;
                    }
                    if (r != p && r != q) {
                        const double arp = A[r * N + p], arq = A[r * N + q];
                        const double nrp = cs * arp - sn * arq, nrq = sn * arp + cs * arq;
                        A[r * N + p] = nrp;
                        A[p * N + r] = nrp;
                        A[r * N + q] = nrq;
                        A[q * N + r] = nrq;
                    }
                    const double vrp = V[r * N + p], vrq = V[r * N + q];
                    V[r * N + p] = cs * vrp - sn * vrq;
                    V[r * N + q] = sn * vrp + cs * vrq;
                    if (r == p) {   // (lane p owns the pair's own three entries: no row update reads them)
                        A[p * N + p] = app - t * apq;
                        A[q * N + q] = aqq + t * apq;
                        A[p * N + q] = 0.0;
                        A[q * N + p] = 0.0;
                    }
                });
            }
    }
    return sweep;
}

// ---- 1: the homography of view v, by one wavefront; lds: 162 doubles (A, V) ----
template <class X, class G>
CALIB_FN void calib_hartley(X& x, int P, G pt, double* m)
{
    double s2[2];
    x.template wsum<2>(P, [&](int k, double* acc) {
        double px, py;
        pt(k, px, py);
        acc[0] = acc[0] + px;
        acc[1] = acc[1] + py;
    }, s2);
    const double mx = s2[0] / (double)P, my = s2[1] / (double)P;
    double d[1];
    x.template wsum<1>(P, [&](int k, double* acc) {
        double px, py;
        pt(k, px, py);
        const double dx = px - mx, dy = py - my;
        acc[0] = acc[0] + sqrt(dx * dx + dy * dy);
    }, d);
    m[0] = mx;
    m[1] = my;
    m[2] = 1.4142135623730951 / (d[0] / (double)P);
}

template <class X>
CALIB_FN void calib_view_homography(X& x, const CalibJob& j, int v)
{
    const int P = j.cols * j.rows;
    const float* c = j.corners + (int64_t)v * j.per_frame * 2;
    double* A = x.wave_lds();
    double* V = A + 81;
    double* Hout = j.ws + (int64_t)v * CALIB_VIEW_WS + CV_H;
    const int cols = j.cols;
    const double square = j.square;
    auto obj = [&](int k, double& px, double& py) {
        px = (double)(k % cols) * square;
        py = (double)(k / cols) * square;
    };
    auto img = [&](int k, double& px, double& py) {
        px = (double)c[2 * k];
        py = (double)c[2 * k + 1];
    };
    double mo[3], mi[3];
    calib_hartley(x, P, obj, mo);
    calib_hartley(x, P, img, mi);
    {
        double acc[45];
        x.template wsum<45>(P, [&](int k, double* a) {
            double X0, Y0, u0, v0;
            obj(k, X0, Y0);
            img(k, u0, v0);
            const double Xn = (X0 - mo[0]) * mo[2], Yn = (Y0 - mo[1]) * mo[2], u = (u0 - mi[0]) * mi[2], w = (v0 - mi[1]) * mi[2];
            const double r1[9] = {-Xn, -Yn, -1.0, 0.0, 0.0, 0.0, u * Xn, u * Yn, u}, r2[9] = {0.0, 0.0, 0.0, -Xn, -Yn, -1.0, w * Xn, w * Yn, w};
            int n = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) {
#pragma unroll
                for (int q = i; q < 9; q++) {
                    a[n] = a[n] + (r1[i] * r1[q] + r2[i] * r2[q]);
                    n++;
                }
            }
        }, acc);
        x.lanes(1, [&](int) {
            int n = 0;
#pragma unroll
            for (int i = 0; i < 9; i++) {
#pragma unroll
                for (int q = i; q < 9; q++) {
                    A[i * 9 + q] = acc[n];
                    A[q * 9 + i] = acc[n];
                    n++;
                }
            }
            for (int i = 0; i < 81; i++) V[i] = (i / 9 == i % 9) ? 1.0 : 0.0;
        });
    }
    calib_jacobi<9>(x, A, V);
    x.lanes(1, [&](int) {
        int m = 0;
        for (int i = 1; i < 9; i++)
            if (A[i * 9 + i] < A[m * 9 + m]) m = i;
        double G[9];
        for (int r = 0; r < 3; r++) {
            G[3 * r] = V[(3 * r) * 9 + m] * mo[2];
            G[3 * r + 1] = V[(3 * r + 1) * 9 + m] * mo[2];
            G[3 * r + 2] = V[(3 * r + 2) * 9 + m] - (G[3 * r] * mo[0] + G[3 * r + 1] * mo[1]);
        }
        double H[9];
        for (int i = 0; i < 3; i++) {
            H[i] = G[i] / mi[2] + mi[0] * G[6 + i];
            H[3 + i] = G[3 + i] / mi[2] + mi[1] * G[6 + i];
            H[6 + i] = G[6 + i];
        }
        const double h8 = H[8];
        for (int i = 0; i < 9; i++) Hout[i] = H[i] / h8;
    });
}

// is view v used?  (what one lane checks of it: points k = lane, lane + 64, ..; the wavefront ORs)
CALIB_FN bool calib_points_finite(const float* c, int P, int first, int step)
{
    bool ok = true;
    for (int k = first; k < P; k += step) ok = ok && calib_finite_f(c[2 * k]) && calib_finite_f(c[2 * k + 1]);
    return ok;
}

// ---- 2: initial intrinsics of one camera from its views' homographies (one thread) ----
CALIB_FN void calib_init_intrinsics(const CalibJob& j, const int32_t* list, int nused, double* a)
{
    const double cx = ((double)j.w - 1.0) / 2.0, cy = ((double)j.h - 1.0) / 2.0;
    double a00 = 0.0, a01 = 0.0, a11 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int i = 0; i < nused; i++) {
        const double* H = j.ws + (int64_t)list[i] * CALIB_VIEW_WS + CV_H;
        double h[3] = {H[0] - cx * H[6], H[3] - cy * H[6], H[6]}, v[3] = {H[1] - cx * H[7], H[4] - cy * H[7], H[7]};
        double d1[3], d2[3];
        for (int k = 0; k < 3; k++) {
            d1[k] = (h[k] + v[k]) * 0.5;
            d2[k] = (h[k] - v[k]) * 0.5;
        }
        const double nh = 1.0 / sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]), nv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double n1 = 1.0 / sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]), n2 = 1.0 / sqrt(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
        for (int k = 0; k < 3; k++) {
            h[k] = h[k] * nh;
            v[k] = v[k] * nv;
            d1[k] = d1[k] * n1;
            d2[k] = d2[k] * n2;
        }
        for (int e = 0; e < 2; e++) {
            const double p0 = e ? d1[0] * d2[0] : h[0] * v[0], p1 = e ? d1[1] * d2[1] : h[1] * v[1], rhs = e ? -(d1[2] * d2[2]) : -(h[2] * v[2]);
            a00 = a00 + p0 * p0;
            a01 = a01 + p0 * p1;
            a11 = a11 + p1 * p1;
            b0 = b0 + p0 * rhs;
            b1 = b1 + p1 * rhs;
        }
    }
    const double det = a00 * a11 - a01 * a01;
    const double n0 = (a11 * b0 - a01 * b1) / det, n1 = (a00 * b1 - a01 * b0) / det;
    a[0] = sqrt(calib_abs(1.0 / n0));
    a[1] = sqrt(calib_abs(1.0 / n1));
    a[2] = cx;
    a[3] = cy;
    for (int k = 4; k < 9; k++) a[k] = 0.0;
}

// ---- the unit quaternion (w, x, y, z) of a rotation matrix, as 3 states it: the first largest of (trace, R00, R11, R22), then divided by its norm ----
CALIB_FN void calib_mat_to_quat(double R00, double R01, double R02, double R10, double R11, double R12, double R20, double R21, double R22, double* q)
{
    const double tr = R00 + R11 + R22;
    int br = 0;
    double best = tr;
    if (R00 > best) { best = R00; br = 1; }
    if (R11 > best) { best = R11; br = 2; }
    if (R22 > best) { best = R22; br = 3; }
    double w, x, y, z;
    if (br == 0) {
        const double s = 2.0 * sqrt(1.0 + tr);
        w = s / 4.0; x = (R21 - R12) / s; y = (R02 - R20) / s; z = (R10 - R01) / s;
    } else if (br == 1) {
        const double s = 2.0 * sqrt(1.0 + R00 - R11 - R22);
        w = (R21 - R12) / s; x = s / 4.0; y = (R01 + R10) / s; z = (R02 + R20) / s;
    } else if (br == 2) {
        const double s = 2.0 * sqrt(1.0 + R11 - R00 - R22);
        w = (R02 - R20) / s; x = (R01 + R10) / s; y = s / 4.0; z = (R12 + R21) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R22 - R00 - R11);
        w = (R10 - R01) / s; x = (R02 + R20) / s; y = (R12 + R21) / s; z = s / 4.0;
    }
    const double n = sqrt(w * w + x * x + y * y + z * z);
    q[0] = w / n; q[1] = x / n; q[2] = y / n; q[3] = z / n;
}

// ---- 3: the initial pose of a view from its homography and the intrinsics (one lane) ----
CALIB_FN void calib_init_pose(const double* H, const double* a, double* q, double* t)
{
    double M[9];
    for (int i = 0; i < 3; i++) {
        M[i] = (H[i] - a[2] * H[6 + i]) / a[0];
        M[3 + i] = (H[3 + i] - a[3] * H[6 + i]) / a[1];
        M[6 + i] = H[6 + i];
    }
    double k = 1.0 / sqrt(M[0] * M[0] + M[3] * M[3] + M[6] * M[6]);
    if (M[8] * k < 0) k = -k;
    const double r0[3] = {M[0] * k, M[3] * k, M[6] * k};
    double b[3] = {M[1] * k, M[4] * k, M[7] * k};
    t[0] = M[2] * k;
    t[1] = M[5] * k;
    t[2] = M[8] * k;
    const double dt = r0[0] * b[0] + r0[1] * b[1] + r0[2] * b[2];
    for (int i = 0; i < 3; i++) b[i] = b[i] - dt * r0[i];
    const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    const double r1[3] = {b[0] / nb, b[1] / nb, b[2] / nb};
    const double r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    // R[i][c]: c = 0 -> r0[i], 1 -> r1[i], 2 -> r2[i]
    const double R00 = r0[0], R01 = r1[0], R02 = r2[0], R10 = r0[1], R11 = r1[1], R12 = r2[1], R20 = r0[2], R21 = r1[2], R22 = r2[2];
    calib_mat_to_quat(R00, R01, R02, R10, R11, R12, R20, R21, R22, q);
}

// ---- 4: what a wavefront does for view v ----
// the cost of the view at (a, q, t) -> every lane's return value
template <class X>
CALIB_FN double calib_view_cost(X& x, const CalibJob& j, int v, const double* a, const double* q, const double* t)
{
    const float* c = j.corners + (int64_t)v * j.per_frame * 2;
    const int cols = j.cols;
    const double square = j.square;
    double R[6], aa[9], tt[3];
    calib_rot6(q, R);
    for (int i = 0; i < 9; i++) aa[i] = a[i];
    for (int i = 0; i < 3; i++) tt[i] = t[i];
    double out[1];
    x.template wsum<1>(j.cols * j.rows, [&](int k, double* acc) {
        CalibProj p;
        calib_project(aa, R, tt, (double)(k % cols) * square, (double)(k / cols) * square, p);
        double ru, rv;
        calib_residual(aa, p, (double)c[2 * k], (double)c[2 * k + 1], ru, rv);
        acc[0] = acc[0] + (ru * ru + rv * rv);
    }, out);
    return out[0];
}

template <int R0, int R1, class X>
CALIB_FN void calib_view_pass(X& x, const CalibJob& j, const float* c, const double* aa, const double* R, const double* tt, double* blk)
{
    const int cols = j.cols, fix = j.fix_mask;
    const double square = j.square;
    double acc[CalibPass<R0, R1>::N];
    x.template wsum<CalibPass<R0, R1>::N>(j.cols * j.rows, [&](int k, double* s) {
        CalibProj p;
        CalibPt o;
        calib_project(aa, R, tt, (double)(k % cols) * square, (double)(k / cols) * square, p);
        calib_residual(aa, p, (double)c[2 * k], (double)c[2 * k + 1], o.ru, o.rv);
        calib_jacobian(aa, p, fix, o);
        calib_pass_add<R0, R1>(o, s);
    }, acc);
    x.lanes(1, [&](int) { calib_pass_store<R0, R1>(acc, blk); });
}

// the blocks of view v at the current state, their elimination under lambda: T, e, Y, z and the flag into the view's workspace row
template <class X>
CALIB_FN void calib_view_eliminate(X& x, const CalibJob& j, int v, const double* a, double lambda)
{
    double* wsv = j.ws + (int64_t)v * CALIB_VIEW_WS;
    double* blk = x.wave_lds();     // 120 + 15 + 1, then L (36)
    double* L = blk + 136;
    double R[6], aa[9], tt[3];
    calib_rot6(wsv + CV_Q, R);
    for (int i = 0; i < 9; i++) aa[i] = a[i];
    for (int i = 0; i < 3; i++) tt[i] = wsv[CV_T + i];
    const float* c = j.corners + (int64_t)v * j.per_frame * 2;
    calib_view_pass<0, 2>(x, j, c, aa, R, tt, blk);
    calib_view_pass<2, 4>(x, j, c, aa, R, tt, blk);
    calib_view_pass<4, 7>(x, j, c, aa, R, tt, blk);
    calib_view_pass<7, 10>(x, j, c, aa, R, tt, blk);
    calib_view_pass<10, 15>(x, j, c, aa, R, tt, blk);
    const double damp = 1.0 + lambda;
    x.lanes(1, [&](int) {
        for (int i = 0; i < 6; i++)
            for (int m = 0; m <= i; m++) L[i * 6 + m] = blk[calib_hidx(9 + m, 9 + i)] * (i == m ? damp : 1.0);
        wsv[CV_BAD] = calib_chol(L, 6) ? 0.0 : 1.0;
    });
    if (wsv[CV_BAD] != 0.0) return;   // (the same for every lane)
    x.lanes(10, [&](int i) {
        if (i < 9) {
            double* Y = wsv + CV_Y + 6 * i;
            for (int m = 0; m < 6; m++) Y[m] = blk[calib_hidx(i, 9 + m)];
            calib_chol_solve(L, 6, Y, Y);
        } else
            calib_chol_solve(L, 6, blk + 120 + 9, wsv + CV_Z);
    });
    x.lanes(54, [&](int n) {
        if (n < 45) {
            int i = 0, r = n;
            while (r >= 9 - i) {
                r -= 9 - i;
                i++;
            }
            const int q = i + r;   // entry (i, q), i <= q, of the 9 x 9 upper triangle in row-major order
            double s = blk[calib_hidx(i, q)];
            if (i == q) s = s * damp;
            for (int m = 0; m < 6; m++) s = s - wsv[CV_Y + 6 * i + m] * blk[calib_hidx(q, 9 + m)];
            wsv[CV_RED + n] = s;
        } else {
            const int i = n - 45;
            double s = blk[120 + i];
            for (int m = 0; m < 6; m++) s = s - blk[calib_hidx(i, 9 + m)] * wsv[CV_Z + m];
            wsv[CV_RED + n] = s;
        }
    });
}

// the step of view v from da: the trial pose, its cost, |db|^2 and |q|^2 + |t|^2
template <class X>
CALIB_FN void calib_view_trial(X& x, const CalibJob& j, int v, const double* da, const double* at)
{
    double* wsv = j.ws + (int64_t)v * CALIB_VIEW_WS;
    x.lanes(1, [&](int) {
        double db[6], dn = 0.0;
        for (int m = 0; m < 6; m++) {
            double s = wsv[CV_Z + m];
            for (int i = 0; i < 9; i++) s = s + wsv[CV_Y + 6 * i + m] * da[i];
            db[m] = -s;
            dn = dn + db[m] * db[m];
        }
        const double* q = wsv + CV_Q;
        const double* t = wsv + CV_T;
        const double ox = db[0] * 0.5, oy = db[1] * 0.5, oz = db[2] * 0.5;
        const double w = q[0] - (ox * q[1] + oy * q[2] + oz * q[3]);
        const double qx = q[1] + ox * q[0] + (oy * q[3] - oz * q[2]);
        const double qy = q[2] + oy * q[0] + (oz * q[1] - ox * q[3]);
        const double qz = q[3] + oz * q[0] + (ox * q[2] - oy * q[1]);
        const double n = sqrt(w * w + qx * qx + qy * qy + qz * qz);
        wsv[CV_QT] = w / n;
        wsv[CV_QT + 1] = qx / n;
        wsv[CV_QT + 2] = qy / n;
        wsv[CV_QT + 3] = qz / n;
        for (int i = 0; i < 3; i++) wsv[CV_TT + i] = t[i] + db[3 + i];
        wsv[CV_DN] = dn;
        wsv[CV_PN] = (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) + (t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    });
    const double cost = calib_view_cost(x, j, v, at, wsv + CV_QT, wsv + CV_TT);
    x.lanes(1, [&](int) { wsv[CV_COSTT] = cost; });
}

// entry `off` of the workspace rows summed over the camera's views
CALIB_FN double calib_sum_views(const CalibJob& j, const int32_t* list, int nused, int off)
{
    double s = 0.0;
    for (int i = 0; i < nused; i++) s = s + j.ws[(int64_t)list[i] * CALIB_VIEW_WS + off];
    return s;
}

// the rvec of 5 from (q, t) carried
CALIB_FN void calib_rvec(const double* q, double* rvec)
{
    double w = q[0], x = q[1], y = q[2], z = q[3];
    if (w < 0) {
        w = -w; x = -x; y = -y; z = -z;
    }
    const double n = sqrt(x * x + y * y + z * z);
    if (n < (double)FLT_EPSILON) {
        rvec[0] = rvec[1] = rvec[2] = 0.0;
        return;
    }
    const double k = 2.0 * pm_atan2(n, w) / n;
    rvec[0] = x * k;
    rvec[1] = y * k;
    rvec[2] = z * k;
}

// ---- one camera: c.nused and list (its used views, ascending) are set; X says who runs what ----
template <class X>
CALIB_FN void calib_camera(X& x, CalibCam& c, const int32_t* list, const CalibJob& j, int cam)
{
    const int P = j.cols * j.rows, nused = c.nused;
    rmcv_calib_result* res = j.results + cam;
    if (nused < CALIB_VIEWS_MIN || nused > CALIB_VIEWS_PER_CAMERA_MAX) {
        x.each(1, [&](int) {
            res->status = nused < CALIB_VIEWS_MIN ? RMCV_CALIB_TOO_FEW_VIEWS : RMCV_CALIB_TOO_MANY_VIEWS;
            res->views_used = nused;
            res->iters = 0;
        });
        return;
    }
    x.each(1, [&](int) {
        const rmcv_calib_guess* g = j.guesses ? j.guesses + cam : nullptr;
        if (g && g->camera_matrix[0] != 0.0) {
            c.a[0] = g->camera_matrix[0]; c.a[1] = g->camera_matrix[4]; c.a[2] = g->camera_matrix[2]; c.a[3] = g->camera_matrix[5];
            for (int k = 0; k < 5; k++) c.a[4 + k] = g->dist[k];
        } else
            calib_init_intrinsics(j, list, nused, c.a);
        c.ok = calib_finite(c.a[0]) && calib_finite(c.a[1]) && c.a[0] > 0.0 && c.a[1] > 0.0;
        c.lambda = 1e-3;
        c.iters = 0;
        c.status = 0;
        c.done = 0;
    });
    if (c.ok) {
        x.each_view(nused, [&](int i) {
            double* wsv = j.ws + (int64_t)list[i] * CALIB_VIEW_WS;
            x.lanes(1, [&](int) { calib_init_pose(wsv + CV_H, c.a, wsv + CV_Q, wsv + CV_T); });
            const double cost = calib_view_cost(x, j, list[i], c.a, wsv + CV_Q, wsv + CV_T);
            x.lanes(1, [&](int) { wsv[CV_COST] = cost; });
        });
        x.each(1, [&](int) {
            c.cost = calib_sum_views(j, list, nused, CV_COST);
            c.rms_init = sqrt(c.cost / ((double)P * (double)nused));
            c.ok = calib_finite(c.cost);
        });
    }
    if (!c.ok) {
        x.each(1, [&](int) {
            res->status = RMCV_CALIB_BAD_INIT;
            res->views_used = nused;
            res->iters = 0;
        });
        return;
    }
    while (!c.done) {
        if (c.iters == j.max_iters) {
            x.each(1, [&](int) {
                c.status = RMCV_CALIB_MAX_ITERS;
                c.done = 1;
            });
            continue;
        }
        x.each_view(nused, [&](int i) { calib_view_eliminate(x, j, list[i], c.a, c.lambda); });
        x.each(54, [&](int n) {
            const double s = calib_sum_views(j, list, nused, CV_RED + n);
            if (n < 45) {
                int i = 0, r = n;
                while (r >= 9 - i) {
                    r -= 9 - i;
                    i++;
                }
                c.S[(i + r) * 9 + i] = s;   // the lower triangle, for calib_chol
            } else
                c.rs[n - 45] = s;
        });
        x.each(1, [&](int) {
            c.iters++;
            c.ok = calib_sum_views(j, list, nused, CV_BAD) == 0.0;
            for (int k = 0; k < 9; k++)
                if ((j.fix_mask >> k) & 1) {
                    c.S[k * 9 + k] = 1.0;
                    c.rs[k] = 0.0;
                }
            if (c.ok) c.ok = calib_chol(c.S, 9);
            if (c.ok) {
                calib_chol_solve(c.S, 9, c.rs, c.da);
                for (int k = 0; k < 9; k++) {
                    c.da[k] = -c.da[k];
                    c.at[k] = c.a[k] + c.da[k];
                }
            }
        });
        if (c.ok) x.each_view(nused, [&](int i) { calib_view_trial(x, j, list[i], c.da, c.at); });
        x.each(1, [&](int) {
            bool accept = false;
            if (c.ok) {
                c.cost_t = calib_sum_views(j, list, nused, CV_COSTT);
                accept = calib_finite(c.cost_t) && c.cost_t < c.cost;
            }
            if (accept) {
                double dn = 0.0, pn = 0.0;
                for (int k = 0; k < 9; k++) {
                    dn = dn + c.da[k] * c.da[k];
                    pn = pn + c.a[k] * c.a[k];
                }
                dn = dn + calib_sum_views(j, list, nused, CV_DN);
                pn = pn + calib_sum_views(j, list, nused, CV_PN);
                for (int k = 0; k < 9; k++) c.a[k] = c.at[k];
                c.cost = c.cost_t;
                c.lambda = c.lambda / 10.0;
                if (dn <= j.eps * j.eps * pn) {
                    c.status = RMCV_CALIB_CONVERGED;
                    c.done = 1;
                }
                c.ok = 1;
            } else {
                c.lambda = c.lambda * 10.0;
                if (c.lambda > 1e12) {
                    c.status = RMCV_CALIB_STALLED;
                    c.done = 1;
                }
                c.ok = 0;
            }
        });
        if (c.ok)   // accepted: the trial poses and costs become the state
            x.each(nused, [&](int i) {
                double* wsv = j.ws + (int64_t)list[i] * CALIB_VIEW_WS;
                for (int k = 0; k < 7; k++) wsv[CV_Q + k] = wsv[CV_QT + k];
                wsv[CV_COST] = wsv[CV_COSTT];
            });
    }
    x.each(nused + 1, [&](int i) {
        if (i == nused) {
            for (int k = 0; k < 9; k++) res->camera_matrix[k] = 0.0;
            res->camera_matrix[0] = c.a[0]; res->camera_matrix[4] = c.a[1]; res->camera_matrix[2] = c.a[2]; res->camera_matrix[5] = c.a[3];
            res->camera_matrix[8] = 1.0;
            for (int k = 0; k < 5; k++) res->dist[k] = c.a[4 + k];
            res->rms = sqrt(c.cost / ((double)P * (double)nused));
            res->rms_init = c.rms_init;
            res->views_used = nused;
            res->iters = c.iters;
            res->status = c.status;
            res->reserved = 0;
            return;
        }
        const double* wsv = j.ws + (int64_t)list[i] * CALIB_VIEW_WS;
        rmcv_calib_view* o = j.views + list[i];
        calib_rvec(wsv + CV_Q, o->rvec);
        for (int k = 0; k < 3; k++) o->tvec[k] = wsv[CV_T + k];
        for (int k = 0; k < 4; k++) o->q[k] = wsv[CV_Q + k];
        o->rms = sqrt(wsv[CV_COST] / (double)P);
        o->used = 1;
        o->reserved = 0;
    });
}

// ---- the sequential form: every view's flag and homography, then camera by camera.  ws: n_views x CALIB_VIEW_WS doubles, vcam: n_views ----
static inline void calib_solve_host(const CalibJob& j)
{
    CalibHostExec x;
    const int P = j.cols * j.rows;
    for (int v = 0; v < j.n_views; v++) {
        const bool used = j.counts[v] == P && calib_points_finite(j.corners + (int64_t)v * j.per_frame * 2, P, 0, 1);
        j.vcam[v] = used ? frame_camera_eff(j.view_camera ? j.view_camera[v] : 0, j.n_cameras) : -1;
        if (used) calib_view_homography(x, j, v);
    }
    int32_t list[CALIB_VIEWS_PER_CAMERA_MAX];
    for (int cam = 0; cam < j.n_cameras; cam++) {
        CalibCam c;
        c.nused = 0;
        for (int v = 0; v < j.n_views; v++)
            if (j.vcam[v] == cam) {
                if (c.nused < CALIB_VIEWS_PER_CAMERA_MAX) list[c.nused] = v;
                c.nused++;
            }
        calib_camera(x, c, list, j, cam);
    }
}

} // namespace rmcv
