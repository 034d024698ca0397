// rmcv_track.hip -- tracker state of rm::armour with everything readable: rm::armour::reset / update(const armour&) /
// update(int64) (/root/reference/src/core.cpp:51-122) and the association loop of the tracking thread
// (executable/main.cpp:57-88).  The HOST-SIDE form, over caller memory: one target or one list at a time, for a host that tracks a
// single camera itself.  The device-resident form for a batch of streams is k_track.hip / device_track.h; both exist.
//
// The filter -- cv::KalmanFilter(6, 6, 0, CV_64F) (core.cpp:21): predict and correct as sequential k-sums, the gain through a one-sided
// Jacobi SVD and back substitution -- is device_track.h's trk_kf_predict / trk_kf_correct, the source the device tracker compiles, run
// here as plain loops on a workspace whose record is the caller's, copied in and out.  ONE thing differs between the two forms: this one
// is compared with the unmodified CPU oracle and keeps libm's hypot in the Jacobi rotation (TRK_HYPOT below); the device tracker uses the
// correctly rounded pm_hypot, so the filter fields of the two may differ in the last bits (include/rmcv_abi.h).  What is
// this file's own: init and reset, the identity history, and rmcv_track_step with its dry run and capacity rule.
#include <math.h>
#include <string.h>

#include <vector>

#include <algorithm>

#include "../../include/rmcv_abi.h"
#define TRK_HYPOT hypot
#include "device_track.h"

namespace {

void set_identity(double* M, double v)
{
    for (int i = 0; i < 36; i++) M[i] = 0;
    for (int i = 0; i < 6; i++) M[i * 7] = v;
}

// a filter step of device_track.h on the caller's record: the workspace (5 KB, on the stack) lives for the call
template <typename Step>
void on_workspace(rmcv_track* t, Step step)
{
    trk_ws ws;
    ws.rec = *t;
    step(&ws, 0);
    *t = ws.rec;
}
void kf_predict(rmcv_track* t) { on_workspace(t, trk_kf_predict); } // [OCV] KalmanFilter::predict() without control
void kf_correct(rmcv_track* t) { on_workspace(t, trk_kf_correct); } // [OCV] KalmanFilter::correct(measurement)

} // namespace

extern "C" {

void rmcv_track_init(rmcv_track* t, const rmcv_armour* a, int32_t identity, int64_t timestamp, const double position[3])
{
    if (!t) return;
    memset(t, 0, sizeof(*t));
    if (a) t->armour = *a;
    t->identity = identity; // executable/main.cpp:181
    t->timestamp = timestamp;
    if (position)
        for (int i = 0; i < 3; i++) t->position[i] = position[i];
    // cv::KalmanFilter::init(6, 6, 0, CV_64F): transition and both noise covariances identity, everything else zero
    set_identity(t->transition, 1.0);
    set_identity(t->process_noise_cov, 1.0);
    set_identity(t->measurement_noise_cov, 1.0);
}

void rmcv_track_reset(rmcv_track* t, double process_noise, double measurement_noise, double error)
{ // src/core.cpp:51-72
    if (!t) return;
    set_identity(t->measurement_matrix, 1.0);
    set_identity(t->process_noise_cov, process_noise);
    set_identity(t->measurement_noise_cov, measurement_noise);
    set_identity(t->error_cov_post, error);
    for (int i = 0; i < 6; i++) t->measurement[i] = 0;
    set_identity(t->transition, 1.0);
    t->transition[0 * 6 + 3] = t->transition[1 * 6 + 4] = t->transition[2 * 6 + 5] = 1.0;
    t->initialized = 0;
}

int rmcv_track_update(rmcv_track* t, const rmcv_track* obs, double tick_frequency)
{ // src/core.cpp:74-108: update(const armour& new_observation)
    if (!t || !obs || !(tick_frequency > 0)) return RMCV_ERR_BAD_ARG;
    { // identity_history[new_observation.identity]++ (a std::map: ids stay ascending)
        int k = 0;
        while (k < t->n_ids && t->ids[k] < obs->identity) k++;
        if (k < t->n_ids && t->ids[k] == obs->identity) t->counts[k]++;
        else {
            if (t->n_ids >= RMCV_TRACK_IDS) return RMCV_ERR_CAPACITY;
            for (int j = t->n_ids; j > k; j--) { t->ids[j] = t->ids[j - 1]; t->counts[j] = t->counts[j - 1]; }
            t->ids[k] = obs->identity;
            t->counts[k] = 1;
            t->n_ids++;
        }
    }
    if (t->initialized) {
        const int64_t delta_tick = obs->timestamp - t->timestamp;
        const double dt = (double)delta_tick / tick_frequency;
        t->transition[0 * 6 + 3] = dt;
        t->transition[1 * 6 + 4] = dt;
        t->transition[2 * 6 + 5] = dt;
        kf_predict(t);
        t->measurement[3] = (obs->position[0] - t->measurement[0]) / dt;
        t->measurement[4] = (obs->position[1] - t->measurement[1]) / dt;
        t->measurement[5] = (obs->position[2] - t->measurement[2]) / dt;
        t->measurement[0] = obs->position[0];
        t->measurement[1] = obs->position[1];
        t->measurement[2] = obs->position[2];
        kf_correct(t);
    } else {
        t->measurement[0] = obs->position[0];
        t->measurement[1] = obs->position[1];
        t->measurement[2] = obs->position[2];
        kf_correct(t); // no predict yet: errorCovPre is still zero, so this correction leaves the state at zero (as in the reference)
        t->initialized = 1;
    }
    t->timestamp = obs->timestamp;
    return RMCV_OK;
}

int rmcv_track_predict(rmcv_track* t, int64_t new_timestamp, double tick_frequency)
{ // src/core.cpp:110-122: update(int64 new_timestamp)
    if (!t || !(tick_frequency > 0)) return RMCV_ERR_BAD_ARG;
    if (!t->initialized) return RMCV_OK;
    const int64_t delta_tick = new_timestamp - t->timestamp;
    const double dt = (double)delta_tick / tick_frequency;
    t->transition[0 * 6 + 3] = dt;
    t->transition[1 * 6 + 4] = dt;
    t->transition[2 * 6 + 5] = dt;
    kf_predict(t);
    return RMCV_OK;
}

int rmcv_track_step(rmcv_track* tracking, int32_t* n_tracking, int cap, rmcv_track* obs, int32_t* n_obs, double tick_frequency)
{ // executable/main.cpp:60-85, one pass of the tracking thread's loop
    if (!tracking || !n_tracking || !n_obs || *n_tracking < 0 || *n_obs < 0 || (*n_obs > 0 && !obs) || !(tick_frequency > 0)) return RMCV_ERR_BAD_ARG;
    int nt = *n_tracking, no = *n_obs;
    if (no == 0) return RMCV_OK; // :61
    // The reference's vectors grow without bound; here `cap` is the caller's.  What the pass will leave behind is counted FIRST, on
    // indices only: the matching depends on the bounding boxes (which update() never touches) and on the lost counts, so a dry run
    // of the loop below tells exactly how many targets survive and how many observations stay unmatched.  Only if those do not fit
    // is RMCV_ERR_CAPACITY returned -- before anything is changed.  (A steady state of N targets matched by N observations needs
    // cap >= N, as the reference's loop does, not 2 N.)
    if (nt + no > cap) {
        std::vector<int> tg((size_t)nt), ob((size_t)no);
        for (int i = 0; i < nt; i++) tg[(size_t)i] = i;
        for (int k = 0; k < no; k++) ob[(size_t)k] = k;
        if (nt > 0)
            for (size_t i = 0; i < tg.size(); i++) {
                int index = -1;
                float iou = 0;
                for (size_t k = 0; k < ob.size(); k++) {
                    int32_t hit = -1;
                    float v = 0;
                    rmcv_max_iou(&tracking[tg[i]].armour, &obs[ob[k]].armour, 1, &hit, &v);
                    if (hit == 0 && v > iou) { iou = v; index = (int)k; }
                }
                if (iou > 0.5f) ob.erase(ob.begin() + index);
                else if (tracking[tg[i]].lost_count > 25) tg.erase(tg.begin() + (long)i); // (and the loop's i++ skips the one that moved in)
            }
        if ((int)(tg.size() + ob.size()) > cap) return RMCV_ERR_CAPACITY;
    }
    if (nt == 0) { // :63-67
        memcpy(tracking, obs, (size_t)no * sizeof(rmcv_track));
        *n_tracking = no;
        return RMCV_OK;
    }
    for (int i = 0; i < nt; i++) { // :69-81
        int32_t index = -1;
        float iou = 0;
        for (int k = 0; k < no; k++) { // armour::max_IoU over the remaining observations (src/core.cpp:144-162), any number of them
            int32_t hit = -1;
            float v = 0;
            rmcv_max_iou(&tracking[i].armour, &obs[k].armour, 1, &hit, &v);
            if (hit == 0 && v > iou) { // `iou > max` with max starting at 0: the first of equal maxima wins, as in the reference's loop
                iou = v;
                index = k;
            }
        }
        if (iou > 0.5f) {
            const int rc = rmcv_track_update(&tracking[i], &obs[index], tick_frequency);
            if (rc) { // only the identity table can overflow (RMCV_TRACK_IDS), and it does before the target is touched: hand back
                *n_tracking = nt; // consistent lists -- what has been processed so far stays processed, nothing is duplicated
                *n_obs = no;
                return rc;
            }
            for (int k = index; k + 1 < no; k++) obs[k] = obs[k + 1]; // armours->erase(begin() + index)
            no--;
        } else if (tracking[i].lost_count++ > 25) {
            for (int k = i; k + 1 < nt; k++) tracking[k] = tracking[k + 1]; // tracking.erase(begin() + i) ...
            nt--; // ... and the loop's i++ then SKIPS the target that moved into slot i (the reference does)
        } else {
            rmcv_track_predict(&tracking[i], tracking[i].timestamp, tick_frequency);
        }
    }
    memcpy(tracking + nt, obs, (size_t)no * sizeof(rmcv_track)); // tracking.insert(end(), armours...)
    *n_tracking = nt + no;
    *n_obs = 0;
    return RMCV_OK;
}

} // extern "C"
