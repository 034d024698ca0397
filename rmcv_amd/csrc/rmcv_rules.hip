// rmcv_rules.hip -- the entry points of include/rmcv_abi.h that take no context and touch no device: the defaults, and the rules the
// kernels and the reference's tracker apply, for a host to apply them too (each through the function the device compiles).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "../../include/rmcv_abi.h"
#include "bind_plan.h"
#include "enhance_math.h"
#include "model_plan.h"
#include "device_track.h"

using namespace rmcv;

extern "C" {

void rmcv_default_params(rmcv_params* p)
{ // the literals of executable/main.cpp:172-176
    memset(p, 0, sizeof(*p));
    p->camp = RMCV_CAMP_BLUE;
    p->lower_bound = 80;
    p->morph = RMCV_MORPH_CLOSE;
    p->tilt_max = 70.0f;
    p->ratio_lo = 1.5f;
    p->ratio_hi = 80.0f;
    p->area_lo = 10.0;
    p->area_hi = 99999.0;
    p->angle_diff_max = 12.0f;
    p->shear_max = 22.0f;
    p->length_ratio_max = 0.4f;
}

void rmcv_default_limits(rmcv_limits* l)
{
    memset(l, 0, sizeof(*l));
    l->max_frames = 256;
    l->max_width = 1920;
    l->max_height = 1200;
    l->max_contours = 2048;
    l->max_points = 65536;
    l->max_blobs = 256;
    l->max_armours = 256;
}

void rmcv_default_pnp_config(rmcv_pnp_config* c)
{
    if (!c) return;
    // executable/main.cpp:7-19: every literal carries an `f` suffix, i.e. it is a float widened to double
    const float K[9] = {1782.672144409928f, 0.0f, 598.8983414505224f, 0.0f, 1783.860175007369f, 523.4209809658056f, 0.0f, 0.0f, 1.0f};
    const float D[5] = {-0.03436366268485048f, 0.1953669264956857f, 0.0001485060439399386f, -0.003814875777013483f,
                        -0.3181808766352414f};
    const float G[16] = {0.0007941130268316332f, 0.009683274185178004f, -0.9999528006788897f, -27.25811584661768f,
                         0.9989588796104363f, 0.04560298009571095f, 0.001234930707386894f, -51.46996511920027f,
                         0.04561278583864914f, -0.9989127101040636f, -0.009636978810429797f, 77.11760876626687f,
                         0.0f, 0.0f, 0.0f, 1.0f};
    for (int i = 0; i < 9; i++) c->camera_matrix[i] = K[i];
    for (int i = 0; i < 5; i++) c->dist[i] = D[i];
    for (int i = 0; i < 16; i++) c->gripper2camera[i] = G[i];
    c->square_w = 27.0f; // executable/main.cpp:184
    c->square_h = 27.0f;
}

/* the rule from a raw index to the table entry k_pnp uses (frame_camera_eff, the function it runs): host-side, no context, no device */
int rmcv_frame_camera(int32_t idx, int32_t n_cameras) { return frame_camera_eff(idx, n_cameras); }

/* ... and to the model-table entry k_classify_models uses (frame_model_eff, model_plan.h) */
int rmcv_frame_model(int32_t idx, int32_t n_models) { return frame_model_eff(idx, n_models); }

// ---- tracker bookkeeping: host-side, see include/rmcv_abi.h --------------------------------------------------
namespace {
struct RectF { float x, y, w, h; };
inline bool rect_empty(const RectF& r) { return r.w <= 0 || r.h <= 0; }
// cv::Rect_<float>::operator& (the overflow-safe form of OpenCV >= 4.5)
inline RectF rect_and(const RectF& a, const RectF& b)
{
    const RectF zero = {0, 0, 0, 0};
    if (rect_empty(a) || rect_empty(b)) return zero;
    const RectF& rx_min = (a.x < b.x) ? a : b;
    const RectF& rx_max = (a.x < b.x) ? b : a;
    const RectF& ry_min = (a.y < b.y) ? a : b;
    const RectF& ry_max = (a.y < b.y) ? b : a;
    if ((rx_min.x < 0 && rx_min.x + rx_min.w < rx_max.x) || (ry_min.y < 0 && ry_min.y + ry_min.h < ry_max.y)) return zero;
    RectF o;
    o.w = std::min(rx_min.w - (rx_max.x - rx_min.x), rx_max.w);
    o.h = std::min(ry_min.h - (ry_max.y - ry_min.y), ry_max.h);
    o.x = rx_max.x;
    o.y = ry_max.y;
    return rect_empty(o) ? zero : o;
}
} // namespace

int rmcv_max_iou(const rmcv_armour* self, const rmcv_armour* list, int n, int32_t* index, float* iou_out)
{
    if (!self || !index || !iou_out || n < 0 || (n > 0 && !list)) return RMCV_ERR_BAD_ARG;
    int idx = -1;
    float max = 0;
    const RectF me = {self->bbox[0], self->bbox[1], self->bbox[2], self->bbox[3]};
    for (int i = 0; i < n; i++) { // src/core.cpp:148-160
        const RectF other = {list[i].bbox[0], list[i].bbox[1], list[i].bbox[2], list[i].bbox[3]};
        const RectF in = rect_and(me, other);
        const float union_area = me.w * me.h + other.w * other.h - in.w * in.h;
        const float iou = in.w * in.h / union_area;
        if (iou > max) {
            max = iou;
            idx = i;
        }
    }
    *index = idx;
    *iou_out = max;
    return RMCV_OK;
}

int rmcv_identity_max(const int32_t* ids, const int32_t* counts, int n, int32_t* max_id, double* prob_out)
{
    if (!max_id || !prob_out || n < 0 || (n > 0 && (!ids || !counts))) return RMCV_ERR_BAD_ARG;
    for (int i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1]) return RMCV_ERR_BAD_ARG; // std::map order
    double sum = 0;
    for (int i = 0; i < n; i++) sum += exp((double)counts[i]); // src/core.cpp:127
    double max = 0;
    int id = -1;
    for (int i = 0; i < n; i++) {
        const double prob = exp((double)counts[i]) / sum; // :133
        if (prob > max) {
            max = prob;
            id = ids[i];
        }
    }
    *max_id = id;
    *prob_out = max;
    return RMCV_OK;
}

int rmcv_gamma_lut(float gamma, uint8_t lut[256])
{
    if (!lut || !(gamma >= 0.0f) || !std::isfinite(gamma)) return RMCV_ERR_BAD_ARG;
    for (int i = 0; i < 256; i++) lut[i] = enh_lut_entry(i, gamma);
    return RMCV_OK;
}

int rmcv_enhance_gamma(const uint64_t sums_bgr[3], int64_t n_pixels, float max_gain, float min_gain, float* gamma)
{
    if (!sums_bgr || !gamma || n_pixels <= 0 || !gains_ok(max_gain, min_gain)) return RMCV_ERR_BAD_ARG;
    *gamma = enh_gamma(sums_bgr, n_pixels, max_gain, min_gain);
    return RMCV_OK;
}

/* the rule from raw camp and lower bound to what the kernels use (frame_key_eff, the function k_frame_keys runs): host-side, no context, no device */
int rmcv_frame_key(int32_t camp, int32_t lower_bound, int32_t out[4])
{
    if (!out) return RMCV_ERR_BAD_ARG;
    const FrameKey k = frame_key_eff(camp, lower_bound);
    out[0] = k.ca;
    out[1] = k.cb;
    out[2] = k.lb;
    out[3] = k.all_pass;
    return RMCV_OK;
}

/* rm::utils::GetROI (src/core.cpp:224-263), verbatim: host-side, no context, no device */
int rmcv_get_roi(const float* points, int n, float scale_w, float scale_h, int frame_w, int frame_h, const int32_t previous[4], int32_t out[4])
{
    if (!out || n < 0 || (n > 0 && !points)) return RMCV_ERR_BAD_ARG;
    trk_get_roi(points, n, scale_w, scale_h, frame_w, frame_h, previous, out); // (device_track.h: the device tracker compiles the same body)
    return RMCV_OK;
}

int rmcv_window_origin(const int32_t rect[4], int win_w, int win_h, int32_t out_xy[2])
{
    if (!rect || !out_xy || win_w < 1 || win_h < 1) return RMCV_ERR_BAD_ARG;
    trk_window_origin(rect, win_w, win_h, out_xy); // (device_track.h)
    return RMCV_OK;
}

int rmcv_armours_to_frame(rmcv_armour* armours, int n, int x, int y)
{
    if (n < 0 || (n > 0 && !armours)) return RMCV_ERR_BAD_ARG;
    const float fx = (float)x, fy = (float)y;
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 4; k++) {
            armours[i].icon[k][0] += fx;
            armours[i].icon[k][1] += fy;
            armours[i].vertices[k][0] += fx;
            armours[i].vertices[k][1] += fy;
        }
        armours[i].bbox[0] += fx;
        armours[i].bbox[1] += fy;
    }
    return RMCV_OK;
}

int rmcv_lightblob_overlap(const rmcv_lightblob* lb, int n, int left, int right, int32_t* overlap)
{
    if (!overlap || (n > 0 && !lb)) return RMCV_ERR_BAD_ARG;
    *overlap = 0;
    if (left < 0 || right > n || right - left < 2) return RMCV_OK; // src/objdetect.cpp:91
    if (right == n) return RMCV_ERR_BAD_ARG;                       // the reference reads lightBlobs[size()] here
    if (lb[left].target != lb[right].target) return RMCV_OK;       // :92
    const float lower_y = std::min(std::min(lb[left].vertices[1][1], lb[left].vertices[2][1]),
                                   std::min(lb[right].vertices[1][1], lb[right].vertices[2][1])); // :94-96
    const float upper_y = std::max(std::max(lb[left].vertices[0][1], lb[left].vertices[3][1]),
                                   std::max(lb[right].vertices[0][1], lb[right].vertices[3][1])); // :97-99
    for (int i = left; i < right; i++) {
        if (lb[i].target != lb[left].target) continue;
        if (lb[i].center[0] > lb[left].center[0] && lb[i].center[0] < lb[right].center[0] && lb[i].center[1] > lower_y &&
            lb[i].center[1] < upper_y) {
            *overlap = 1;
            return RMCV_OK;
        }
    }
    return RMCV_OK;
}

} // extern "C"
