// k_track.hip -- the device-resident tracker: the tracking state of a batch of camera streams in HBM, stepped behind a
// batch without the host, and the next batch's window origins written from it.
//   the tracking thread        /root/reference/executable/main.cpp:57-88
//   rm::armour::reset / update /root/reference/src/core.cpp:51-122
//   rm::utils::GetROI          /root/reference/src/core.cpp:218-263
// The step itself is device_track.h, the same source rmcv_tracker_step_host (below) runs on the CPU.  The object behind the ABI's handle --
// lifetime, tables, setters and getters -- is rmcv_tracker.hip; this unit sees a TrackerBufs and a config.
//
// Mapping (gfx950, wave64).  The work is latency-bound: per stream a tiny sequential association, then one dependent chain of 6x6 fp64
// operations per track that matched or coasts.  ONE WORKGROUP PER STREAM, 8 wavefronts: lane 0 walks the association into a plan in LDS
// (indices only: that walk is the dry run), the wavefronts then take the slots of the list the pass leaves behind, one wavefront per
// track -- the record and every matrix in LDS, one matrix element per lane (36 of 64 busy), scalars computed by every lane from LDS so
// that control flow is uniform -- and lane 0 commits: length, the current/next flip, the target rule, the next window's origin (ordinary
// vector stores).  No inter-workgroup waits; nothing is indexed dynamically in registers (no scratch).  256 streams are 256 workgroups:
// one per CU.
#include <string.h>

#include <vector>

#include "rmcv_internal.h"
#include "device_track.h"

namespace rmcv {

static constexpr int TRACK_WAVES = 8;

static trk_cfg step_cfg(const rmcv_tracker_config& c)
{
    trk_cfg k;
    k.track_cap = c.track_cap;
    k.frame_w = c.frame_w;
    k.frame_h = c.frame_h;
    k.win_w = c.win_w;
    k.win_h = c.win_h;
    k.roi_scale_w = c.roi_scale_w;
    k.roi_scale_h = c.roi_scale_h;
    k.process_noise = c.process_noise;
    k.measurement_noise = c.measurement_noise;
    k.error = c.error;
    k.tick_frequency = c.tick_frequency;
    return k;
}

__global__ __launch_bounds__(TRACK_WAVES * 64) void k_track(trk_cfg cfg, TrackerBufs tb, int n_streams, const rmcv_armour* __restrict__ armours,
                                                            const int32_t* __restrict__ n_armours, const int32_t* __restrict__ identity,
                                                            const double* __restrict__ poses, int max_armours,
                                                            const rmcv_point* __restrict__ win_eff, int64_t timestamp)
{
    __shared__ trk_plan_t plan;
    __shared__ trk_ws ws[TRACK_WAVES];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (f >= n_streams) return;
    const int cap = cfg.track_cap;
    const int sel = tb.sel[f] & 1;
    int nt = tb.n_tracking[f];
    nt = nt < 0 ? 0 : (nt > cap ? cap : nt);
    const size_t cur_at = ((size_t)sel * n_streams + f) * cap, nxt_at = ((size_t)(sel ^ 1) * n_streams + f) * cap;
    const rmcv_track* cur = tb.tracks + cur_at;
    rmcv_track* nxt = tb.tracks + nxt_at;
    const float* side_cur = tb.side + cur_at * 8;
    float* side_nxt = tb.side + nxt_at * 8;
    trk_obs ob;
    ob.armours = armours + (size_t)f * max_armours;
    ob.identity = identity ? identity + (size_t)f * max_armours : nullptr;
    ob.pos = poses ? poses + (size_t)f * max_armours * 9 + 6 : nullptr;
    ob.pos_stride = 9;
    const int na = n_armours[f];
    ob.n = na < 0 ? 0 : (na > max_armours ? max_armours : na);
    ob.fx = win_eff ? (float)win_eff[f].x : 0.0f;
    ob.fy = win_eff ? (float)win_eff[f].y : 0.0f;
    ob.timestamp = timestamp;
    if (tid == 0) trk_plan(&plan, cur, nt, &ob, &cfg);
    __syncthreads();
    const int apply = plan.apply, n_out = plan.n_src + plan.n_new;
    if (apply)
        for (int j = wave; j < n_out; j += TRACK_WAVES) trk_apply_slot(&ws[wave], &plan, j, cur, side_cur, nxt, side_nxt, &ob, &cfg, lane);
    __syncthreads();
    if (tid == 0) {
        if (plan.ovf) tb.status[f] |= RMCV_TRACKER_OVF;
        if (apply) {
            tb.n_tracking[f] = n_out;
            tb.sel[f] = sel ^ 1;
        }
        if (!plan.ovf) trk_next_window(apply ? nxt : cur, apply ? side_nxt : side_cur, apply ? n_out : nt, &cfg, &tb.origins[f]);
    }
}

hipError_t launch_track(const rmcv_tracker_config& cfg, const TrackerBufs& tb, const Bufs& b, const Limits& lim, bool identity, bool pose,
                        const rmcv_point* win_eff, int64_t timestamp, hipStream_t s)
{
    return launch(k_track, dim3(cfg.n_streams), dim3(TRACK_WAVES * 64), 0, s, step_cfg(cfg), tb, cfg.n_streams, (const rmcv_armour*)b.armours,
                  (const int32_t*)b.n_armours, (const int32_t*)(identity ? b.identity : nullptr), (const double*)(pose ? b.poses : nullptr),
                  lim.max_armours, win_eff, timestamp);
}

} // namespace rmcv

using namespace rmcv;

extern "C" {

void rmcv_default_tracker_config(rmcv_tracker_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->n_streams = 256;
    c->track_cap = 64;
    c->process_noise = 5e-5; // executable/main.cpp:195
    c->measurement_noise = 0.5;
    c->error = 0.05;
    c->tick_frequency = 1e9;  // cv::getTickFrequency() on Linux
    c->roi_scale_w = c->roi_scale_h = 1.0f;
    c->frame_w = 1280;
    c->frame_h = 1024;
}

int rmcv_tracker_step_host(const rmcv_tracker_config* cfg, rmcv_track* tracks, float* last_vertices, int32_t* n_tracking, int32_t* status,
                           rmcv_point* origin, const rmcv_armour* armours, int n_obs, const int32_t* identities, const double* positions,
                           int x_eff, int y_eff, int64_t timestamp)
{
    if (!cfg || !tracks || !last_vertices || !n_tracking || !status || !origin || n_obs < 0 || (n_obs > 0 && !armours)) return RMCV_ERR_BAD_ARG;
    if (tracker_config_refusal(*cfg, false) || *n_tracking < 0 || *n_tracking > cfg->track_cap) return RMCV_ERR_BAD_ARG;
    const trk_cfg k = step_cfg(*cfg);
    trk_obs ob;
    ob.armours = armours;
    ob.identity = identities;
    ob.pos = positions;
    ob.pos_stride = 3;
    ob.n = n_obs;
    ob.fx = (float)x_eff;
    ob.fy = (float)y_eff;
    ob.timestamp = timestamp;
    std::vector<trk_plan_t> plan(1);
    trk_plan(&plan[0], tracks, *n_tracking, &ob, &k);
    const trk_plan_t& pl = plan[0];
    if (pl.ovf) {
        *status |= RMCV_TRACKER_OVF;
        return RMCV_OK;
    }
    if (pl.apply) {
        const int n_out = pl.n_src + pl.n_new;
        std::vector<rmcv_track> nxt((size_t)n_out);
        std::vector<float> side_nxt((size_t)n_out * 8);
        std::vector<trk_ws> ws(1);
        for (int j = 0; j < n_out; j++) trk_apply_slot(&ws[0], &pl, j, tracks, last_vertices, nxt.data(), side_nxt.data(), &ob, &k, 0);
        memcpy(tracks, nxt.data(), (size_t)n_out * sizeof(rmcv_track));
        memcpy(last_vertices, side_nxt.data(), (size_t)n_out * 8 * sizeof(float));
        *n_tracking = n_out;
    }
    trk_next_window(tracks, last_vertices, *n_tracking, &k, origin);
    return RMCV_OK;
}

} // extern "C"
