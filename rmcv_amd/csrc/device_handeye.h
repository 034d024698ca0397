// device_handeye.h -- the hand-eye solve: the camera's mounting on the gimbal from the board poses of the calibration solve
// (4u) and the gimbal's attitudes, the library's pinned statement of cv::calibrateHandEye as executable/calibration/hand_eye.cpp:140-155
// calls it, with the check loop behind it (:157-180).  One source for rmcv_calibrate_hand_eye_host (the sequential form: HandEyeHostExec
// below) and the kernel k_handeye (k_handeye.hip), which agree bit for bit.  OpenCV is not the reference here: this text is, and DESIGN.md 4v
// lists where it knowingly departs (the closed form of Horaud and Dornaika over all pairs, where the reference's call takes Tsai's).
// Everything is double, built with -ffp-contract=off; every expression is evaluated as written, left to right; behind the gimbal's
// rotation matrix only + - x / and sqrt occur.
//
// Input.  views rmcv_calib_view [n_views] as the calibration solve leaves them: q (w, x, y, z) and tvec are read as they stand (board to
//         camera: q_c, t_c), and `used`; rvec and rms are not read.  attitudes rmcv_attitude [n_views], radians.  gripper_t double
//         [n_views][3] or null (zeros).  view_camera int32 [n_views] or null (camera 0); a value outside 0 .. n_cameras - 1 is camera 0
//         (frame_camera_eff).  View v is USED for camera c iff view_camera maps it to c, its used == 1, and q, tvec, (roll, pitch, yaw) and,
//         when the table is given, its gripper_t are all finite.  A camera's used views are taken in ascending v: u = 0 .. n - 1 below.
//         n < 3: TOO_FEW_VIEWS; n > 256: TOO_MANY_VIEWS; then status, views_used and pairs_used = pairs_skipped = sweeps = 0 are written and
//         nothing else.
// Views.  B = rmcv_euler_to_matrix(attitude) (att_to_matrix, NaN canonical); q_g = the unit quaternion of B by the calibration solve's
//         rule (calib_mat_to_quat: the first largest of trace and diagonal, divided by its norm).  t_g = the view's gripper_t or (0, 0, 0).
// Algebra. conj(q) negates x, y, z.  p (x) q = (((p0 q0 - p1 q1) - p2 q2) - p3 q3, ((p0 q1 + p1 q0) + p2 q3) - p3 q2,
//         ((p0 q2 - p1 q3) + p2 q0) + p3 q1, ((p0 q3 + p1 q2) - p2 q1) + p3 q0).  R(q), taking q as a unit quaternion: rows
//         (1 - 2 (y y + z z), 2 (x y - w z), 2 (x z + w y)), (2 (x y + w z), 1 - 2 (x x + z z), 2 (y z - w x)),
//         (2 (x z - w y), 2 (y z + w x), 1 - 2 (x x + y y)).  A matrix times a 3-vector: row r gives (m0 v0 + m1 v1) + m2 v2.
// Pairs.  All i < j of the used views in lexicographic order; pair index p counts them from 0.  a = conj(q_g[j]) (x) q_g[i],
//         b = q_c[j] (x) conj(q_c[i]); each has all four components negated when its w < 0 or its w is -0.0.
//         The pair is USED iff a.w >= min_w and b.w >= min_w (a NaN fails), else SKIPPED.
//         t_A = B_j^T (t_g[i] - t_g[j]): entry k is (B_j[0][k] e0 + B_j[1][k] e1) + B_j[2][k] e2.  t_B = t_c[j] - R(b) t_c[i].
// Sums.   Every sum over pairs or over views is a BLOCK SUM of 256 partials: partial T takes the items (pairs p, views u) with index
//         % 256 == T in ascending order, starting from 0.0 (a skipped pair adds nothing); then within each group of 64 partials
//         acc[l] = acc[l] + acc[l ^ s] for s = 32, 16, 8, 4, 2, 1, all 64 at once per s; the sum is ((g0 + g1) + g2) + g3 of the groups' results.
// 1 Rotation.  d = a - b, s = a + b (componentwise); D = L(a) - R(b) = rows (d0, -d1, -d2, -d3), (d1, d0, -s3, s2), (d2, s3, d0, -s1),
//         (d3, -s2, s1, d0).  M[i][k] (i <= k) = block sum of ((D[0][i] D[0][k] + D[1][i] D[1][k]) + D[2][i] D[2][k]) + D[3][i] D[3][k]:
//         10 sums, mirrored; pairs_used and pairs_skipped are block sums of 1.0 in the same pass.  pairs_used == 0: TOO_FEW_VIEWS as above,
//         with pairs_skipped written.  Otherwise the cyclic Jacobi of device_calib.h (calib_jacobi, 4 x 4, V = I); sweeps = the sweeps
//         begun.  eig = M's diagonal sorted ascending; q_X = column m of V, m the first index of the smallest diagonal entry, divided by
//         sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3); when its first non-zero component is negative every component becomes 0.0 - q.
//         R_X = R(q_X).
// 2 Translation.  Per used pair C = R(a) with 1.0 subtracted on the diagonal, g = R_X t_B - t_A (row r: ((R_X t_B)[r]) - t_A[r]).
//         N[i][k] (i <= k) = block sum of (C[0][i] C[0][k] + C[1][i] C[1][k]) + C[2][i] C[2][k]; r[i] = block sum of
//         (C[0][i] g0 + C[1][i] g1) + C[2][i] g2.  Cholesky of N, rows ascending, columns ascending; pivots[i] = the i-th diagonal's value
//         before its root.  A pivot not > 0 or not finite: T_UNOBSERVABLE, the later pivots 0, t_X = 0.  Else t_X = N^-1 r by
//         calib_chol_solve, status OK.  cam2gripper = rmcv_homogeneous(R_X, t_X).
// 3 Check.  Per used view: p = cam2gripper (t_c, 1) and world = rmcv_homogeneous(B, t_g) p as general 4 x 4 products, row r
//         ((m0 v0 + m1 v1) + m2 v2) + m3 v3, the zeros and ones taking part (t_g = 0 is the reference's h_base2gripper); views_out row:
//         world, used = 1, reserved = 0.
//         world_mean = (block sum of world) / n.
// 4 Residuals.  world_rms = sqrt((block sum of (e0 e0 + e1 e1) + e2 e2, e = world - world_mean) / n).  trans_rms = sqrt((block sum over
//         used pairs of (e0 e0 + e1 e1) + e2 e2, e = C t_X - g) / pairs_used).  rot_rms = sqrt(max(eig[0], 0) / pairs_used).
//         Every double that leaves is NaN-canonical (att_canon).  Rows of views not used, or of a camera without a solution, are not touched.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "device_attitude.h"
#include "device_calib.h"
#include "handeye_plan.h"

namespace rmcv {

// one call's tables; on the device every pointer is device memory
struct HandEyeJob {
    const rmcv_calib_view* views;    // [n_views]
    const rmcv_attitude* att;        // [n_views]
    const double* gripper_t;         // [n_views][3] nullable
    const int32_t* view_camera;      // [n_views] nullable
    rmcv_handeye_result* results;    // [n_cameras]
    rmcv_handeye_view* views_out;    // [n_views]
    double min_w;
    int n_views, n_cameras;
};

// a camera's state: LDS on the device
struct HandEyeCam {
    double A[16], V[16], L[9], r[3], q[4], RX[9], t[3], G[16], mean[3], eig[4], piv[3], world_ss, trans_ss;
    int32_t nused, pairs_used, pairs_skipped, sweeps, status, pad;
};
static_assert(sizeof(HandEyeCam) == HANDEYE_CAM_STATE_BYTES, "handeye_plan.h states the camera's LDS");

CALIB_FN bool handeye_view_used(const HandEyeJob& j, int v, int cam)
{
    if (frame_camera_eff(j.view_camera ? j.view_camera[v] : 0, j.n_cameras) != cam) return false;
    const rmcv_calib_view* w = j.views + v;
    if (w->used != 1) return false;
    bool ok = calib_finite(w->q[0]) && calib_finite(w->q[1]) && calib_finite(w->q[2]) && calib_finite(w->q[3]);
    ok = ok && calib_finite(w->tvec[0]) && calib_finite(w->tvec[1]) && calib_finite(w->tvec[2]);
    ok = ok && calib_finite(j.att[v].roll) && calib_finite(j.att[v].pitch) && calib_finite(j.att[v].yaw);
    if (j.gripper_t) ok = ok && calib_finite(j.gripper_t[3 * (int64_t)v]) && calib_finite(j.gripper_t[3 * (int64_t)v + 1]) && calib_finite(j.gripper_t[3 * (int64_t)v + 2]);
    return ok;
}

// Views: the staged row of used view v (HANDEYE_VIEW_LDS doubles at s)
CALIB_FN void handeye_stage(const HandEyeJob& j, int v, double* s)
{
    double R[9];
    att_to_matrix(j.att + v, R);
#pragma unroll
    for (int k = 0; k < 9; k++) s[HV_B + k] = att_canon(R[k]);
    calib_mat_to_quat(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s + HV_QG);
#pragma unroll
    for (int k = 0; k < 4; k++) s[HV_QC + k] = j.views[v].q[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s[HV_TC + k] = j.views[v].tvec[k];
        s[HV_TG + k] = j.gripper_t ? j.gripper_t[3 * (int64_t)v + k] : 0.0;
    }
}

// Algebra
CALIB_FN void handeye_qmul(double p0, double p1, double p2, double p3, double q0, double q1, double q2, double q3, double* o)
{
    o[0] = ((p0 * q0 - p1 * q1) - p2 * q2) - p3 * q3;
    o[1] = ((p0 * q1 + p1 * q0) + p2 * q3) - p3 * q2;
    o[2] = ((p0 * q2 - p1 * q3) + p2 * q0) + p3 * q1;
    o[3] = ((p0 * q3 + p1 * q2) - p2 * q1) + p3 * q0;
}
CALIB_FN bool handeye_sign_set(double v)
{
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) != 0;
}
CALIB_FN void handeye_positive_w(double* q)
{
    if (q[0] < 0.0 || (q[0] == 0.0 && handeye_sign_set(q[0]))) {
        q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3];
    }
}
CALIB_FN void handeye_rot9(const double* q, double* R)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}
#define HANDEYE_ROW3(M, r, v) (((M)[3 * (r)] * (v)[0] + (M)[3 * (r) + 1] * (v)[1]) + (M)[3 * (r) + 2] * (v)[2])
#define HANDEYE_ROW4(M, r, v) ((((M)[4 * (r)] * (v)[0] + (M)[4 * (r) + 1] * (v)[1]) + (M)[4 * (r) + 2] * (v)[2]) + (M)[4 * (r) + 3] * (v)[3])

// Pairs: a and b of the staged views si, sj (i < j) -> is the pair used?
CALIB_FN bool handeye_pair(const double* si, const double* sj, double min_w, double* a, double* b)
{
    handeye_qmul(sj[HV_QG], -sj[HV_QG + 1], -sj[HV_QG + 2], -sj[HV_QG + 3], si[HV_QG], si[HV_QG + 1], si[HV_QG + 2], si[HV_QG + 3], a);
    handeye_qmul(sj[HV_QC], sj[HV_QC + 1], sj[HV_QC + 2], sj[HV_QC + 3], si[HV_QC], -si[HV_QC + 1], -si[HV_QC + 2], -si[HV_QC + 3], b);
    handeye_positive_w(a);
    handeye_positive_w(b);
    return a[0] >= min_w && b[0] >= min_w;
}
// 2: C and g of a used pair
CALIB_FN void handeye_pair_trans(const double* si, const double* sj, const double* a, const double* b, const double* RX, double* Cm, double* g)
{
    double Rb[9];
    handeye_rot9(b, Rb);
    const double e[3] = {si[HV_TG] - sj[HV_TG], si[HV_TG + 1] - sj[HV_TG + 1], si[HV_TG + 2] - sj[HV_TG + 2]};
    const double* Bj = sj + HV_B;
    const double tA[3] = {(Bj[0] * e[0] + Bj[3] * e[1]) + Bj[6] * e[2], (Bj[1] * e[0] + Bj[4] * e[1]) + Bj[7] * e[2], (Bj[2] * e[0] + Bj[5] * e[1]) + Bj[8] * e[2]};
    const double* tci = si + HV_TC;
    const double tB[3] = {sj[HV_TC] - HANDEYE_ROW3(Rb, 0, tci), sj[HV_TC + 1] - HANDEYE_ROW3(Rb, 1, tci), sj[HV_TC + 2] - HANDEYE_ROW3(Rb, 2, tci)};
    g[0] = HANDEYE_ROW3(RX, 0, tB) - tA[0];
    g[1] = HANDEYE_ROW3(RX, 1, tB) - tA[1];
    g[2] = HANDEYE_ROW3(RX, 2, tB) - tA[2];
    handeye_rot9(a, Cm);
    Cm[0] = Cm[0] - 1.0;
    Cm[4] = Cm[4] - 1.0;
    Cm[8] = Cm[8] - 1.0;
}
// 3: the board's origin in the base frame as the staged view s has it
CALIB_FN void handeye_world(const double* G, const double* s, double* world)
{
    const double tc[4] = {s[HV_TC], s[HV_TC + 1], s[HV_TC + 2], 1.0};
    const double p[4] = {HANDEYE_ROW4(G, 0, tc), HANDEYE_ROW4(G, 1, tc), HANDEYE_ROW4(G, 2, tc), HANDEYE_ROW4(G, 3, tc)};
    double H[16];
    att_homogeneous(s + HV_B, s + HV_TG, H);
    world[0] = att_canon(HANDEYE_ROW4(H, 0, p));
    world[1] = att_canon(HANDEYE_ROW4(H, 1, p));
    world[2] = att_canon(HANDEYE_ROW4(H, 2, p));
}

// ---- the sequential executor: what the workgroup's 256 threads, its wavefront 0 and their barriers do, one after the other ----
struct HandEyeHostExec {
    template <int N>
    static void reduce(double (*acc)[N], double* out)
    {
        for (int g = 0; g < HANDEYE_WAVES; g++)
            for (int s = 32; s >= 1; s >>= 1)
                for (int l = 0; l < s; l++)
                    for (int n = 0; n < N; n++) acc[64 * g + l][n] = acc[64 * g + l][n] + acc[64 * g + (l ^ s)][n];   // (lanes >= s are no longer read)
        for (int n = 0; n < N; n++) out[n] = ((acc[0][n] + acc[64][n]) + acc[128][n]) + acc[192][n];
    }
    // out[n] = the block sum of what f(i, j, acc) adds for the pair (i, j) of n views
    template <int N, class F>
    void pair_sum(int n, F f, double* out)
    {
        double acc[HANDEYE_THREADS][N];
        for (int T = 0; T < HANDEYE_THREADS; T++) {
            for (int k = 0; k < N; k++) acc[T][k] = 0.0;
            int i = 0, j = 1;
            handeye_pair_advance(i, j, T, n);
            while (i < n - 1) {
                f(i, j, acc[T]);
                handeye_pair_advance(i, j, HANDEYE_THREADS, n);
            }
        }
        reduce<N>(acc, out);
    }
    // the same over the views u = 0 .. n - 1
    template <int N, class F>
    void view_sum(int n, F f, double* out)
    {
        double acc[HANDEYE_THREADS][N];
        for (int T = 0; T < HANDEYE_THREADS; T++) {
            for (int k = 0; k < N; k++) acc[T][k] = 0.0;
            for (int u = T; u < n; u += HANDEYE_THREADS) f(u, acc[T]);
        }
        reduce<N>(acc, out);
    }
    template <class F> void lanes(int n, F f) { for (int i = 0; i < n; i++) f(i); }   // lane i < n runs f(i); then the wavefront meets
    template <class F> void wave0(F f) { f(); }                                       // wavefront 0 runs f; then a barrier
    template <class F> void each(int n, F f) { for (int i = 0; i < n; i++) f(i); }    // thread i < n runs f(i); then a barrier
};

// ---- one camera: c.nused and list (its used views, ascending) are set; stage: nused rows of HANDEYE_VIEW_LDS doubles; X says who runs what ----
template <class X>
CALIB_FN void handeye_camera(X& x, HandEyeCam& c, const int32_t* list, double* stage, const HandEyeJob& j, int cam)
{
    const int nused = c.nused;
    rmcv_handeye_result* res = j.results + cam;
    if (nused < HANDEYE_VIEWS_MIN || nused > CALIB_VIEWS_PER_CAMERA_MAX) {
        x.each(1, [&](int) {
            res->status = nused < HANDEYE_VIEWS_MIN ? RMCV_HANDEYE_TOO_FEW_VIEWS : RMCV_HANDEYE_TOO_MANY_VIEWS;
            res->views_used = nused;
            res->pairs_used = res->pairs_skipped = res->sweeps = 0;
        });
        return;
    }
    x.each(nused, [&](int u) { handeye_stage(j, list[u], stage + u * HANDEYE_VIEW_LDS); });
    const double min_w = j.min_w;
    // 1: the rotation
    {
        double m[12];
        x.template pair_sum<12>(nused, [&](int pi, int pj, double* acc) {
            double a[4], b[4];
            if (!handeye_pair(stage + pi * HANDEYE_VIEW_LDS, stage + pj * HANDEYE_VIEW_LDS, min_w, a, b)) {
                acc[11] = acc[11] + 1.0;
                return;
            }
            acc[10] = acc[10] + 1.0;
            const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2], d3 = a[3] - b[3], s1 = a[1] + b[1], s2 = a[2] + b[2], s3 = a[3] + b[3];
            const double D[16] = {d0, -d1, -d2, -d3, d1, d0, -s3, s2, d2, s3, d0, -s1, d3, -s2, s1, d0};
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int k = i; k < 4; k++) {
                    acc[n] = acc[n] + (((D[i] * D[k] + D[4 + i] * D[4 + k]) + D[8 + i] * D[8 + k]) + D[12 + i] * D[12 + k]);
                    n++;
                }
            }
        }, m);
        x.each(1, [&](int) {
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int k = i; k < 4; k++) {
                    c.A[i * 4 + k] = m[n];
                    c.A[k * 4 + i] = m[n];
                    n++;
                }
            }
            for (int i = 0; i < 16; i++) c.V[i] = (i / 4 == i % 4) ? 1.0 : 0.0;
            c.pairs_used = (int32_t)m[10];
            c.pairs_skipped = (int32_t)m[11];
        });
    }
    if (c.pairs_used == 0) {
        x.each(1, [&](int) {
            res->status = RMCV_HANDEYE_TOO_FEW_VIEWS;
            res->views_used = nused;
            res->pairs_used = 0;
            res->pairs_skipped = c.pairs_skipped;
            res->sweeps = 0;
        });
        return;
    }
    x.wave0([&]() {
        const int sweeps = calib_jacobi<4>(x, c.A, c.V);
        x.lanes(1, [&](int) {
            c.sweeps = sweeps;
            int m = 0;
            for (int i = 1; i < 4; i++)
                if (c.A[i * 5] < c.A[m * 5]) m = i;
            for (int i = 0; i < 4; i++) c.eig[i] = c.A[i * 5];
            for (int i = 1; i < 4; i++)   // (an insertion sort: ascending, equal values keep their order)
                for (int k = i; k > 0 && c.eig[k] < c.eig[k - 1]; k--) {
                    const double t = c.eig[k];
                    c.eig[k] = c.eig[k - 1];
                    c.eig[k - 1] = t;
                }
            const double q0 = c.V[m], q1 = c.V[4 + m], q2 = c.V[8 + m], q3 = c.V[12 + m];
            const double nq = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
            c.q[0] = q0 / nq; c.q[1] = q1 / nq; c.q[2] = q2 / nq; c.q[3] = q3 / nq;
            int f = 0;
            while (f < 3 && c.q[f] == 0.0) f++;
            if (c.q[f] < 0.0)
                for (int i = 0; i < 4; i++) c.q[i] = 0.0 - c.q[i];
            handeye_rot9(c.q, c.RX);
        });
    });
    // 2: the translation
    {
        double RX[9], s[9];
#pragma unroll
        for (int i = 0; i < 9; i++) RX[i] = c.RX[i];
        x.template pair_sum<9>(nused, [&](int pi, int pj, double* acc) {
            const double* si = stage + pi * HANDEYE_VIEW_LDS;
            const double* sj = stage + pj * HANDEYE_VIEW_LDS;
            double a[4], b[4], Cm[9], g[3];
            if (!handeye_pair(si, sj, min_w, a, b)) return;
            handeye_pair_trans(si, sj, a, b, RX, Cm, g);
            int n = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int k = i; k < 3; k++) {
                    acc[n] = acc[n] + ((Cm[i] * Cm[k] + Cm[3 + i] * Cm[3 + k]) + Cm[6 + i] * Cm[6 + k]);
                    n++;
                }
            }
#pragma unroll
            for (int i = 0; i < 3; i++) acc[6 + i] = acc[6 + i] + ((Cm[i] * g[0] + Cm[3 + i] * g[1]) + Cm[6 + i] * g[2]);
        }, s);
        x.each(1, [&](int) {
            c.L[0] = s[0];
            c.L[3] = s[1]; c.L[4] = s[3];
            c.L[6] = s[2]; c.L[7] = s[4]; c.L[8] = s[5];
            c.L[1] = c.L[2] = c.L[5] = 0.0;
            c.r[0] = s[6]; c.r[1] = s[7]; c.r[2] = s[8];
            bool ok = true;
            for (int i = 0; i < 3; i++) c.piv[i] = 0.0;
            for (int i = 0; i < 3 && ok; i++)
                for (int k = 0; k <= i && ok; k++) {
                    double v = c.L[i * 3 + k];
                    for (int m = 0; m < k; m++) v = v - c.L[i * 3 + m] * c.L[k * 3 + m];
                    if (i == k) {
                        c.piv[i] = v;
                        if (!(v > 0.0) || !calib_finite(v)) ok = false;
                        else c.L[i * 3 + i] = sqrt(v);
                    } else
                        c.L[i * 3 + k] = v / c.L[k * 3 + k];
                }
            if (ok) calib_chol_solve(c.L, 3, c.r, c.t);
            else c.t[0] = c.t[1] = c.t[2] = 0.0;
            c.status = ok ? RMCV_HANDEYE_OK : RMCV_HANDEYE_T_UNOBSERVABLE;
            att_homogeneous(c.RX, c.t, c.G);
        });
    }
    // 3: the check loop
    {
        double G[16], s[3];
#pragma unroll
        for (int i = 0; i < 16; i++) G[i] = c.G[i];
        x.template view_sum<3>(nused, [&](int u, double* acc) {
            double w[3];
            handeye_world(G, stage + u * HANDEYE_VIEW_LDS, w);
            rmcv_handeye_view* o = j.views_out + list[u];
            o->world[0] = w[0]; o->world[1] = w[1]; o->world[2] = w[2];
            o->used = 1;
            o->reserved = 0;
            acc[0] = acc[0] + w[0]; acc[1] = acc[1] + w[1]; acc[2] = acc[2] + w[2];
        }, s);
        x.each(1, [&](int) {
            for (int i = 0; i < 3; i++) c.mean[i] = s[i] / (double)nused;
        });
        // 4: the residuals
        const double mean[3] = {c.mean[0], c.mean[1], c.mean[2]}, t[3] = {c.t[0], c.t[1], c.t[2]};
        double RX[9], ws[1], ts[1];
#pragma unroll
        for (int i = 0; i < 9; i++) RX[i] = c.RX[i];
        x.template view_sum<1>(nused, [&](int u, double* acc) {
            double w[3];
            handeye_world(G, stage + u * HANDEYE_VIEW_LDS, w);
            const double e0 = w[0] - mean[0], e1 = w[1] - mean[1], e2 = w[2] - mean[2];
            acc[0] = acc[0] + ((e0 * e0 + e1 * e1) + e2 * e2);
        }, ws);
        x.template pair_sum<1>(nused, [&](int pi, int pj, double* acc) {
            const double* si = stage + pi * HANDEYE_VIEW_LDS;
            const double* sj = stage + pj * HANDEYE_VIEW_LDS;
            double a[4], b[4], Cm[9], g[3];
            if (!handeye_pair(si, sj, min_w, a, b)) return;
            handeye_pair_trans(si, sj, a, b, RX, Cm, g);
            const double e0 = HANDEYE_ROW3(Cm, 0, t) - g[0], e1 = HANDEYE_ROW3(Cm, 1, t) - g[1], e2 = HANDEYE_ROW3(Cm, 2, t) - g[2];
            acc[0] = acc[0] + ((e0 * e0 + e1 * e1) + e2 * e2);
        }, ts);
        x.each(1, [&](int) {
            c.world_ss = ws[0];
            c.trans_ss = ts[0];
        });
    }
    x.each(1, [&](int) {
        const double np = (double)c.pairs_used;
        for (int i = 0; i < 16; i++) res->cam2gripper[i] = att_canon(c.G[i]);
        for (int i = 0; i < 4; i++) res->q[i] = att_canon(c.q[i]);
        for (int i = 0; i < 3; i++) res->t[i] = att_canon(c.t[i]);
        for (int i = 0; i < 4; i++) res->eig[i] = att_canon(c.eig[i]);
        for (int i = 0; i < 3; i++) res->pivots[i] = att_canon(c.piv[i]);
        res->rot_rms = att_canon(sqrt((c.eig[0] > 0.0 ? c.eig[0] : 0.0) / np));
        res->trans_rms = att_canon(sqrt(c.trans_ss / np));
        for (int i = 0; i < 3; i++) res->world_mean[i] = att_canon(c.mean[i]);
        res->world_rms = att_canon(sqrt(c.world_ss / (double)nused));
        res->views_used = nused;
        res->pairs_used = c.pairs_used;
        res->pairs_skipped = c.pairs_skipped;
        res->sweeps = c.sweeps;
        res->status = c.status;
        res->reserved[0] = res->reserved[1] = res->reserved[2] = 0;
    });
}

// ---- the sequential form: camera by camera.  stage: CALIB_VIEWS_PER_CAMERA_MAX x HANDEYE_VIEW_LDS doubles ----
static inline void handeye_solve_host(const HandEyeJob& j, double* stage)
{
    HandEyeHostExec x;
    int32_t list[CALIB_VIEWS_PER_CAMERA_MAX];
    for (int cam = 0; cam < j.n_cameras; cam++) {
        HandEyeCam c;
        c.nused = 0;
        for (int v = 0; v < j.n_views; v++)
            if (handeye_view_used(j, v, cam)) {
                if (c.nused < CALIB_VIEWS_PER_CAMERA_MAX) list[c.nused] = v;
                c.nused++;
            }
        handeye_camera(x, c, list, stage, j, cam);
    }
}

} // namespace rmcv
