/*
 * device_track.h -- one step of the device-resident tracker for ONE camera stream, host and device from the same source:
 *   rm::armour::max_IoU                       /root/reference/src/core.cpp:144-162
 *   rm::armour::reset / update / update(int64) /root/reference/src/core.cpp:51-122   (cv::KalmanFilter(6, 6, 0, CV_64F))
 *   the tracking thread's association loop     /root/reference/executable/main.cpp:60-85
 *   rm::utils::GetROI + the window's origin    /root/reference/src/core.cpp:218-263
 * The arithmetic is that of oracle/rmcv_oracle_track.c, operation for operation (sequential k-sums, one-sided Jacobi SVD with at
 * most 30 sweeps, SVBkSb, the general sums: nothing is made of H = I or of the diagonal noise matrices) with ONE difference: the
 * Jacobi rotation's hypot is TRK_HYPOT, by default pm_hypot (pinned_math.h, correctly rounded) -- a libm's is neither portable to the
 * GPU nor the same from one machine to the next.  That default is the device tracker's (k_track.hip, rmcv_tracker_step_host).  The
 * host-side rmcv_track_* functions (rmcv_track.hip) run this same filter with TRK_HYPOT defined as libm's hypot, as the oracle they are
 * compared with does: the macro is the only thing that differs between the two forms.  Compile with -ffp-contract=off, no fast-math.
 *
 * Execution model.  A step of a stream is  trk_plan  (one lane: the association, on indices only -- the matching depends on bounding
 * boxes that update() never touches and on the lost counts, so the pass can be walked before anything is changed: that walk IS the
 * dry run that decides RMCV_TRACKER_OVF),  trk_apply_slot  for every slot of the list the pass leaves behind (independent of each
 * other: each reads its source record from the current list and writes the next one), and  trk_commit  (one lane: length, the
 * current/next flip, the target rule, the next window's origin).  trk_apply_slot is written for ONE WAVEFRONT per slot: the record
 * and every 6x6 matrix live in a workspace (LDS on the device), a loop over the elements of a matrix is TRK_EACH (lane e takes element
 * e; the host runs it as a plain loop), scalars (the Jacobi's p, beta, gamma, c, s, the thresholds) are computed by every lane from
 * the workspace, so control flow is uniform; TRK_SYNC separates a phase that writes the workspace from one that reads it.  Inside
 * a phase no element reads what another element writes.  Every loop is bounded; a NaN state (dt = 0 on a matched update) runs the
 * Jacobi's 30 sweeps and comes out NaN, as in the oracle.
 */
#ifndef RMCV_DEVICE_TRACK_H
#define RMCV_DEVICE_TRACK_H

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "pinned_math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TRK_EACH(e, n) for (int e = lane; e < (n); e += 64)
#define TRK_ONE if (lane == 0)
#define TRK_SYNC()                                               \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)
#else
#if defined(TRK_HOST_REVERSED) /* a test build: the elements of every phase in the opposite order -- a phase in which one element read what
                                  another wrote would give other bytes (tests/test_tracker_cpu.py) */
#define TRK_EACH(e, n) for (int e = (n) - 1; e >= 0; e--)
#else
#define TRK_EACH(e, n) for (int e = 0; e < (n); e++)
#endif
#define TRK_ONE
#define TRK_SYNC() do { } while (0)
#endif

#ifndef TRK_HYPOT
#define TRK_HYPOT pm_hypot /* the Jacobi rotation's hypot (see the head of this file) */
#endif

#define TRK_MAX_CAP 64                   /* rmcv_tracker_config::track_cap at most */
#define TRK_MAX_OBS (2 * TRK_MAX_CAP)    /* more observations than targets + cap cannot fit whatever they match */
#define TRK_WORDS ((int)(sizeof(rmcv_track) / 8))

/* rmcv_tracker_config as the step reads it */
typedef struct {
    int32_t track_cap, frame_w, frame_h, win_w, win_h;
    float   roi_scale_w, roi_scale_h;
    double  process_noise, measurement_noise, error, tick_frequency;
} trk_cfg;

/* this frame's detections of one stream, as the batch left them (window coordinates) */
typedef struct {
    const rmcv_armour* armours;   /* [n] */
    const int32_t*     identity;  /* [n], or NULL: -1 (core.h:117) */
    const double*      pos;       /* world position of armour k at pos[k * pos_stride .. + 2], or NULL: (0, 0, 0) */
    int32_t            pos_stride;
    int32_t            n;
    float              fx, fy;    /* (float)x_eff, (float)y_eff: window -> frame, one f32 add each (rmcv_armours_to_frame) */
    int64_t            timestamp;
} trk_obs;

#define TRK_KEEP 0   /* the target that moved into an erased one's slot: skipped by the reference's loop, untouched */
#define TRK_MATCH 1
#define TRK_COAST 2
typedef struct {
    int32_t apply;                 /* 1: the lists change; 0: no observation (nothing happens) or refused */
    int32_t ovf;                   /* 1: refused -- RMCV_TRACKER_OVF */
    int32_t n_src, n_new;          /* surviving targets, unmatched observations */
    int16_t src[TRK_MAX_CAP];      /* [n_src] their indices in the current list, in order */
    int16_t fresh[TRK_MAX_CAP];    /* [n_new] the unmatched observations, in order */
    int16_t mobs[TRK_MAX_CAP];     /* per current target: the observation it took */
    uint8_t act[TRK_MAX_CAP];      /* per current target: TRK_* */
    uint8_t alive[TRK_MAX_OBS];
} trk_plan_t;

/* what one wavefront works in */
typedef struct {
    rmcv_track rec;
    float      side[8];
    double     t1[36], t2[36], t3[36], t4[36], at[36], vt[36], buf[36];
    double     wd[6], v6[6], v6b[6];
} trk_ws;

/* ---- rm::utils::GetROI and the window's origin: the bodies of rmcv_get_roi / rmcv_window_origin (rmcv_abi.h has the contract) ---- */
PM_FN void trk_get_roi(const float* points, int n, float scale_w, float scale_h, int frame_w, int frame_h, const int32_t* previous, int32_t* out)
{
    int x = 0, y = 0, w = 0, h = 0; /* cv::boundingRect of no points: the empty rect */
    if (n > 0) {                    /* :227, SURVEY A.8: min / max in float, then floor */
        float minx = points[0], maxx = points[0], miny = points[1], maxy = points[1];
        for (int i = 1; i < n; i++) {
            const float px = points[2 * i], py = points[2 * i + 1];
            minx = px < minx ? px : minx;
            maxx = px > maxx ? px : maxx;
            miny = py < miny ? py : miny;
            maxy = py > maxy ? py : maxy;
        }
        const int ix = (int)__builtin_floorf(minx), iy = (int)__builtin_floorf(miny), ax = (int)__builtin_floorf(maxx), ay = (int)__builtin_floorf(maxy);
        x = ix; y = iy; w = ax - ix + 1; h = ay - iy + 1;
    }
    if (previous) { x += previous[0]; y += previous[1]; } /* :228-229 */
    if (scale_w != 1.0f || scale_h != 1.0f) {             /* :230 */
        const int sw = (int)((double)w * scale_w / 2.0), sh = (int)((double)h * scale_h / 2.0); /* :232-233 */
        x -= sw;
        y -= sh;
        w += sw * 2;
        h += sw * 2; /* :238, as written: the WIDTH's margin */
    }
    if (x < 0) x = 0;                           /* :240-247 (the size is not reduced by what the corner moved) */
    if (y < 0) y = 0;
    if (x + w >= frame_w) w = frame_w - x - 1;  /* :248-255 */
    if (y + h >= frame_h) h = frame_h - y - 1;
    if (w < 0 || h < 0) x = y = w = h = 0;      /* :257-260 */
    out[0] = x; out[1] = y; out[2] = w; out[3] = h;
}

PM_FN void trk_window_origin(const int32_t* rect, int win_w, int win_h, int32_t* out_xy)
{
    /* the window centred on the rect: rect centre (x + w / 2, y + h / 2) minus half the window, integer division truncating */
    out_xy[0] = rect[0] + rect[2] / 2 - win_w / 2;
    out_xy[1] = rect[1] + rect[3] / 2 - win_h / 2;
}

/* ---- rm::armour::max_IoU's arithmetic for one pair of boxes (x, y, w, h): cv::Rect2f operator& (the overflow-safe form), area() ---- */
PM_FN float trk_iou(const float* a, const float* b)
{
    float iw = 0, ih = 0;
    if (!(a[2] <= 0 || a[3] <= 0 || b[2] <= 0 || b[3] <= 0)) {
        const int ax_first = a[0] < b[0], ay_first = a[1] < b[1];
        const float xmin_x = ax_first ? a[0] : b[0], xmin_w = ax_first ? a[2] : b[2], xmax_x = ax_first ? b[0] : a[0], xmax_w = ax_first ? b[2] : a[2];
        const float ymin_y = ay_first ? a[1] : b[1], ymin_h = ay_first ? a[3] : b[3], ymax_y = ay_first ? b[1] : a[1], ymax_h = ay_first ? b[3] : a[3];
        if (!((xmin_x < 0 && xmin_x + xmin_w < xmax_x) || (ymin_y < 0 && ymin_y + ymin_h < ymax_y))) {
            const float w1 = xmin_w - (xmax_x - xmin_x), h1 = ymin_h - (ymax_y - ymin_y);
            const float ow = xmax_w < w1 ? xmax_w : w1, oh = ymax_h < h1 ? ymax_h : h1;
            if (!(ow <= 0 || oh <= 0)) { iw = ow; ih = oh; }
        }
    }
    const float union_area = a[2] * a[3] + b[2] * b[3] - iw * ih;
    return iw * ih / union_area;
}

/* ---- the association (executable/main.cpp:60-85) on indices: ONE lane ----------------------------------------------------------- */
PM_FN void trk_plan(trk_plan_t* pl, const rmcv_track* cur, int nt, const trk_obs* ob, const trk_cfg* cfg)
{
    const int no = ob->n;
    pl->apply = 0;
    pl->ovf = 0;
    pl->n_src = 0;
    pl->n_new = 0;
    if (no <= 0) return;                                       /* :61 -- not even ageing */
    if (no > nt + cfg->track_cap) { pl->ovf = 1; return; }      /* each target takes one observation at most: the rest cannot fit */
    for (int k = 0; k < no; k++) pl->alive[k] = 1;
    int len = nt, ovf = 0;
    for (int i = 0; i < nt; i++) pl->src[i] = (int16_t)i;
    for (int i = 0; i < len; i++) {                            /* :69-81 */
        const int t = pl->src[i];
        int index = -1;
        float max = 0;
        for (int k = 0; k < no; k++) {                         /* max_IoU over the observations that are left, in their order */
            if (!pl->alive[k]) continue;
            float box[4];
            box[0] = ob->armours[k].bbox[0] + ob->fx;
            box[1] = ob->armours[k].bbox[1] + ob->fy;
            box[2] = ob->armours[k].bbox[2];
            box[3] = ob->armours[k].bbox[3];
            const float iou = trk_iou(cur[t].armour.bbox, box);
            if (iou > max) { max = iou; index = k; }           /* the first of equal maxima */
        }
        if (max > 0.5f) {
            pl->act[t] = TRK_MATCH;
            pl->mobs[t] = (int16_t)index;
            pl->alive[index] = 0;
            /* identity_history[identity]++ needs the identity present or a free entry (RMCV_TRACK_IDS) */
            const int32_t id = ob->identity ? ob->identity[index] : -1;
            const int n_ids = cur[t].n_ids;
            int known = 0;
            for (int q = 0; q < RMCV_TRACK_IDS; q++) known |= (q < n_ids && cur[t].ids[q] == id);
            if (!known && n_ids >= RMCV_TRACK_IDS) ovf = 1;
        } else if (cur[t].lost_count > 25) {                    /* lost_count++ > 25: erased ... */
            for (int k = i; k + 1 < len; k++) pl->src[k] = pl->src[k + 1];
            len--;
            if (i < len) pl->act[pl->src[i]] = TRK_KEEP;        /* ... and the loop's i++ skips the target that moved into slot i */
        } else {
            pl->act[t] = TRK_COAST;
        }
    }
    int n_new = 0;
    for (int k = 0; k < no; k++)
        if (pl->alive[k]) {
            if (n_new < TRK_MAX_CAP) pl->fresh[n_new] = (int16_t)k;
            n_new++;
        }
    if (ovf || len + n_new > cfg->track_cap) { pl->ovf = 1; return; }
    pl->n_src = len;
    pl->n_new = n_new;
    pl->apply = 1;
}

/* ---- cv::KalmanFilter on the workspace's record ---------------------------------------------------------------------------------- */
/* C = A * B (6x6 by 6xp, row-major); every entry a sequential sum over k ([OCV] GEMMSingleMul) */
PM_FN void trk_mul(const double* A, const double* B, double* C, int p, int lane)
{
    TRK_EACH(e, 6 * p) {
        const int i = e / p, j = e - i * p;
        double s = 0;
        for (int k = 0; k < 6; k++) s += A[i * 6 + k] * B[k * p + j];
        C[e] = s;
    }
    TRK_SYNC();
}
/* C = A * B^T + D  ([OCV] gemm(A, B, 1, D, 1, C, GEMM_2_T)) */
PM_FN void trk_mul_bt_add(const double* A, const double* B, const double* D, double* C, int lane)
{
    TRK_EACH(e, 36) {
        const int i = e / 6, j = e - i * 6;
        double s = 0;
        for (int k = 0; k < 6; k++) s += A[i * 6 + k] * B[j * 6 + k];
        C[e] = s + D[e];
    }
    TRK_SYNC();
}

/* [OCV] JacobiSVDImpl_<double> on ws->at (6 rows of 6: the transpose of the matrix): one-sided Jacobi (Hestenes), eps = DBL_EPSILON * 10,
 * at most 30 sweeps, singular values (ws->wd) sorted descending; at's rows become the left singular vectors, vt's the right ones */
PM_FN void trk_jacobi_svd(trk_ws* ws, int lane)
{
    const double eps = 2.220446049250313e-16 * 10, minval = 2.2250738585072014e-308;
    double* At = ws->at;
    double* Vt = ws->vt;
    double* Wd = ws->wd;
    TRK_EACH(i, 6) {
        double sd = 0;
        for (int k = 0; k < 6; k++) sd += At[i * 6 + k] * At[i * 6 + k];
        Wd[i] = sd;
    }
    TRK_EACH(e, 36) Vt[e] = (e / 6 == e % 6) ? 1.0 : 0.0;
    TRK_SYNC();
    for (int iter = 0; iter < 30; iter++) {
        int changed = 0;
        for (int i = 0; i < 5; i++)
            for (int j = i + 1; j < 6; j++) {
                double a = Wd[i], p = 0, b = Wd[j];
                for (int k = 0; k < 6; k++) p += At[i * 6 + k] * At[j * 6 + k];
                if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = TRK_HYPOT(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = __builtin_sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = __builtin_sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                TRK_SYNC(); /* (every lane has read rows i and j) */
                TRK_EACH(e, 12) {
                    double* M = e < 6 ? At : Vt;
                    const int k = e < 6 ? e : e - 6;
                    const double x0 = M[i * 6 + k], x1 = M[j * 6 + k];
                    const double t0 = c * x0 + s * x1, t1 = -s * x0 + c * x1;
                    M[i * 6 + k] = t0;
                    M[j * 6 + k] = t1;
                }
                TRK_SYNC();
                a = b = 0;
                for (int k = 0; k < 6; k++) {
                    const double t0 = At[i * 6 + k], t1 = At[j * 6 + k];
                    a += t0 * t0;
                    b += t1 * t1;
                }
                TRK_ONE { Wd[i] = a; Wd[j] = b; }
                TRK_SYNC();
                changed = 1;
            }
        if (!changed) break;
    }
    TRK_EACH(i, 6) {
        double sd = 0;
        for (int k = 0; k < 6; k++) sd += At[i * 6 + k] * At[i * 6 + k];
        Wd[i] = __builtin_sqrt(sd);
    }
    TRK_SYNC();
    TRK_ONE {
        for (int i = 0; i < 5; i++) {
            int j = i;
            for (int k = i + 1; k < 6; k++)
                if (Wd[j] < Wd[k]) j = k;
            if (i != j) {
                { const double t_ = Wd[i]; Wd[i] = Wd[j]; Wd[j] = t_; }
                for (int k = 0; k < 6; k++) { const double t_ = At[i * 6 + k]; At[i * 6 + k] = At[j * 6 + k]; At[j * 6 + k] = t_; }
                for (int k = 0; k < 6; k++) { const double t_ = Vt[i * 6 + k]; Vt[i * 6 + k] = Vt[j * 6 + k]; Vt[j * 6 + k] = t_; }
            }
        }
    }
    TRK_SYNC();
    TRK_EACH(e, 36) {
        /* [OCV] a null singular value gets a random unit vector here; a 6x6 innovation covariance H P H^T + R with R > 0 has none */
        const double w = Wd[e / 6];
        const double s = w > minval ? 1 / w : 0.;
        At[e] *= s;
    }
    TRK_SYNC();
}

/* X = A^-1 * B for 6x6 A, B: [OCV] cv::solve(A, B, X, DECOMP_SVD) = JacobiSVD of A^T's rows + SVBkSb (threshold 2 eps * sum w) */
PM_FN void trk_solve_svd(trk_ws* ws, const double* A, const double* B, double* X, int lane)
{
    TRK_EACH(e, 36) ws->at[e] = A[(e % 6) * 6 + e / 6];
    TRK_SYNC();
    trk_jacobi_svd(ws, lane);
    double threshold = 0;
    for (int i = 0; i < 6; i++) threshold += ws->wd[i];
    threshold *= 2.220446049250313e-16 * 2;
    TRK_EACH(e, 36) { /* buffer of singular triple i = e / 6, column j: MatrAXPY over u_i[k] * B[k][:], then * 1 / w_i */
        const int i = e / 6, j = e - i * 6;
        double wi = ws->wd[i], b = 0;
        if (!(__builtin_fabs(wi) <= threshold)) {
            wi = 1 / wi;
            for (int k = 0; k < 6; k++) b += ws->at[i * 6 + k] * B[k * 6 + j];
            b *= wi;
        }
        ws->buf[e] = b;
    }
    TRK_SYNC();
    TRK_EACH(e, 36) { /* X[k][j] += v_i[k] * buffer_i[j], i ascending */
        const int k = e / 6, j = e - k * 6;
        double x = 0;
        for (int i = 0; i < 6; i++) {
            if (__builtin_fabs(ws->wd[i]) <= threshold) continue;
            x += ws->vt[i * 6 + k] * ws->buf[i * 6 + j];
        }
        X[e] = x;
    }
    TRK_SYNC();
}

/* [OCV] KalmanFilter::predict() without control */
PM_FN void trk_kf_predict(trk_ws* ws, int lane)
{
    rmcv_track* t = &ws->rec;
    trk_mul(t->transition, t->state_post, t->state_pre, 1, lane);
    trk_mul(t->transition, t->error_cov_post, ws->t1, 6, lane);
    trk_mul_bt_add(ws->t1, t->transition, t->process_noise_cov, t->error_cov_pre, lane);
    TRK_EACH(e, 6) t->state_post[e] = t->state_pre[e];
    TRK_EACH(e, 36) t->error_cov_post[e] = t->error_cov_pre[e];
    TRK_SYNC();
}

/* [OCV] KalmanFilter::correct(measurement) */
PM_FN void trk_kf_correct(trk_ws* ws, int lane)
{
    rmcv_track* t = &ws->rec;
    trk_mul(t->measurement_matrix, t->error_cov_pre, ws->t2, 6, lane);
    trk_mul_bt_add(ws->t2, t->measurement_matrix, t->measurement_noise_cov, ws->t3, lane);
    trk_solve_svd(ws, ws->t3, ws->t2, ws->t4, lane);
    TRK_EACH(e, 36) t->gain[e] = ws->t4[(e % 6) * 6 + e / 6];
    TRK_SYNC();
    trk_mul(t->measurement_matrix, t->state_pre, ws->v6, 1, lane);
    TRK_EACH(e, 6) ws->v6b[e] = t->measurement[e] - ws->v6[e];
    TRK_SYNC();
    trk_mul(t->gain, ws->v6b, ws->v6, 1, lane);
    TRK_EACH(e, 6) t->state_post[e] = t->state_pre[e] + ws->v6[e];
    trk_mul(t->gain, ws->t2, ws->t1, 6, lane);
    TRK_EACH(e, 36) t->error_cov_post[e] = t->error_cov_pre[e] - ws->t1[e];
    TRK_SYNC();
}

/* src/core.cpp:74-108: update(const armour& new_observation); the plan has made sure the identity fits */
PM_FN void trk_update(trk_ws* ws, int32_t identity, int64_t timestamp, double px, double py, double pz, double tick, int lane)
{
    rmcv_track* t = &ws->rec;
    const int initialized = t->initialized;
    const double dt = (double)(timestamp - t->timestamp) / tick;
    TRK_SYNC();
    TRK_ONE { /* identity_history[identity]++ (a std::map: ids stay ascending) */
        const int n = t->n_ids;
        int k = 0;
        while (k < n && t->ids[k] < identity) k++;
        if (k < n && t->ids[k] == identity) t->counts[k]++;
        else if (n < RMCV_TRACK_IDS) {
            for (int j = n; j > k; j--) { t->ids[j] = t->ids[j - 1]; t->counts[j] = t->counts[j - 1]; }
            t->ids[k] = identity;
            t->counts[k] = 1;
            t->n_ids = n + 1;
        }
        if (initialized) {
            t->transition[0 * 6 + 3] = dt;
            t->transition[1 * 6 + 4] = dt;
            t->transition[2 * 6 + 5] = dt;
        }
    }
    TRK_SYNC();
    if (initialized) {
        trk_kf_predict(ws, lane);
        TRK_ONE {
            t->measurement[3] = (px - t->measurement[0]) / dt;
            t->measurement[4] = (py - t->measurement[1]) / dt;
            t->measurement[5] = (pz - t->measurement[2]) / dt;
        }
    }
    TRK_ONE {
        t->measurement[0] = px;
        t->measurement[1] = py;
        t->measurement[2] = pz;
    }
    TRK_SYNC();
    trk_kf_correct(ws, lane); /* the first one comes without a prediction: errorCovPre is still zero (as in the reference) */
    TRK_ONE {
        t->initialized = 1;
        t->timestamp = timestamp;
    }
    TRK_SYNC();
}

/* the miss of main.cpp:78-81 for a target that stays: lost_count++, then update(own timestamp) (src/core.cpp:110-122), dt = 0 */
PM_FN void trk_coast(trk_ws* ws, double tick, int lane)
{
    rmcv_track* t = &ws->rec;
    const int initialized = t->initialized;
    const double dt = (double)(t->timestamp - t->timestamp) / tick;
    TRK_SYNC();
    TRK_ONE {
        t->lost_count++;
        if (initialized) {
            t->transition[0 * 6 + 3] = dt;
            t->transition[1 * 6 + 4] = dt;
            t->transition[2 * 6 + 5] = dt;
        }
    }
    TRK_SYNC();
    if (initialized) trk_kf_predict(ws, lane);
}

/* rmcv_track_init + rmcv_track_reset of observation k (executable/main.cpp:178-195), in frame coordinates, into the workspace */
PM_FN void trk_fresh(trk_ws* ws, const trk_obs* ob, int k, const trk_cfg* cfg, int lane)
{
    rmcv_track* t = &ws->rec;
    uint64_t* w = (uint64_t*)t;
    TRK_EACH(e, TRK_WORDS) w[e] = 0;
    TRK_SYNC();
    TRK_EACH(e, 8) {
        const float add = (e & 1) ? ob->fy : ob->fx;
        (&t->armour.icon[0][0])[e] = (&ob->armours[k].icon[0][0])[e] + add;
        (&t->armour.vertices[0][0])[e] = (&ob->armours[k].vertices[0][0])[e] + add;
    }
    TRK_EACH(e, 6) {
        t->transition[e * 7] = 1.0;
        if (e < 3) t->transition[e * 6 + e + 3] = 1.0;
        t->measurement_matrix[e * 7] = 1.0;
        t->process_noise_cov[e * 7] = cfg->process_noise;
        t->measurement_noise_cov[e * 7] = cfg->measurement_noise;
        t->error_cov_post[e * 7] = cfg->error;
    }
    TRK_ONE {
        t->armour.bbox[0] = ob->armours[k].bbox[0] + ob->fx;
        t->armour.bbox[1] = ob->armours[k].bbox[1] + ob->fy;
        t->armour.bbox[2] = ob->armours[k].bbox[2];
        t->armour.bbox[3] = ob->armours[k].bbox[3];
        t->armour.blob_i = ob->armours[k].blob_i;
        t->armour.blob_j = ob->armours[k].blob_j;
        t->timestamp = ob->timestamp;
        t->identity = ob->identity ? ob->identity[k] : -1;
        for (int q = 0; q < 3; q++) t->position[q] = ob->pos ? ob->pos[(int64_t)k * ob->pos_stride + q] : 0.0;
    }
    TRK_SYNC();
}

/* slot j of the list the pass leaves behind: one wavefront (or the host's loop) */
PM_FN void trk_apply_slot(trk_ws* ws, const trk_plan_t* pl, int j, const rmcv_track* cur, const float* side_cur, rmcv_track* nxt, float* side_nxt,
                          const trk_obs* ob, const trk_cfg* cfg, int lane)
{
    int k = -1; /* the observation whose vertices the side record takes */
    if (j < pl->n_src) {
        const int t = pl->src[j];
        const uint64_t* s = (const uint64_t*)&cur[t];
        uint64_t* w = (uint64_t*)&ws->rec;
        TRK_EACH(e, TRK_WORDS) w[e] = s[e];
        TRK_EACH(e, 8) ws->side[e] = side_cur[t * 8 + e];
        TRK_SYNC();
        const int act = pl->act[t];
        if (act == TRK_MATCH) {
            k = pl->mobs[t];
            const double* q = ob->pos ? ob->pos + (int64_t)k * ob->pos_stride : (const double*)0;
            const double px = q ? q[0] : 0.0, py = q ? q[1] : 0.0, pz = q ? q[2] : 0.0;
            trk_update(ws, ob->identity ? ob->identity[k] : -1, ob->timestamp, px, py, pz, cfg->tick_frequency, lane);
        } else if (act == TRK_COAST) {
            trk_coast(ws, cfg->tick_frequency, lane);
        }
    } else {
        k = pl->fresh[j - pl->n_src];
        trk_fresh(ws, ob, k, cfg, lane);
    }
    if (k >= 0) {
        TRK_EACH(e, 8) ws->side[e] = (&ob->armours[k].vertices[0][0])[e] + ((e & 1) ? ob->fy : ob->fx);
    }
    TRK_SYNC();
    {
        const uint64_t* r = (const uint64_t*)&ws->rec;
        uint64_t* d = (uint64_t*)&nxt[j];
        TRK_EACH(e, TRK_WORDS) d[e] = r[e];
        TRK_EACH(e, 8) side_nxt[j * 8 + e] = ws->side[e];
    }
    TRK_SYNC();
}

/* the target rule and the next window: the track with the greatest timestamp (lowest index on ties), its side record through GetROI and
 * the window's origin; no tracks, or win_w == 0: the origin stays.  ONE lane. */
PM_FN void trk_next_window(const rmcv_track* tracks, const float* side, int n, const trk_cfg* cfg, rmcv_point* origin)
{
    if (n <= 0 || cfg->win_w <= 0) return;
    int best = 0;
    for (int i = 1; i < n; i++)
        if (tracks[i].timestamp > tracks[best].timestamp) best = i;
    float v[8];
    for (int e = 0; e < 8; e++) v[e] = side[best * 8 + e];
    int32_t rect[4], xy[2];
    trk_get_roi(v, 4, cfg->roi_scale_w, cfg->roi_scale_h, cfg->frame_w, cfg->frame_h, (const int32_t*)0, rect);
    trk_window_origin(rect, cfg->win_w, cfg->win_h, xy);
    origin->x = xy[0];
    origin->y = xy[1];
}

#endif /* RMCV_DEVICE_TRACK_H */
