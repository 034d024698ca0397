// k_binary_camp.hip -- the pixel kernel with PER-FRAME detection keys (rmcv_batch_set_frame_camps: a mixed fleet's batch, frame f the next
// frame of stream f, every stream hunting its own colour at its own exposure).  k_binary_kernel.inc compiled with K1_CAMP: the same loaders,
// planes, morphology and stores under the name k_binary_camp; a strip reads its frame's key (Bufs::key_eff: channel pair, bound, all-pass flag)
// once, wave-uniform, and enters phase 1 in the thresh16<CA, CB> / K1_PASS instantiation of that pair -- the v_perm selectors and register
// indices stay compile-time.  All three loaders (byte-wise, row-quad, linear); k_binary's shape, never k_binary_ws.  Its own translation unit,
// so that the kernels of k_binary.hip, k_binary_enh.hip and k_binary_win.hip are not touched by it.  With windows: k_binary_camp_win.hip.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "k_binary_device.h"

namespace rmcv {

#define K1_ENH 0
#define K1_CAMP 1
#define K1_KERNEL k_binary_camp
#define K1_THRESH(d) thresh16<CA, CB>(d, lb)
#define K1_PASS(a, b) ((a) - (b) >= lb)
#include "k_binary_kernel.inc"

#define K1_LAUNCH_T launch_binary_camp_t
// the launch's slice of the key table (launches are chunks of frames: f0, nf)
#define K1_EXTRA , b.key_eff + f0
#include "k_binary_launch.inc"

hipError_t launch_binary_camp(const Geom& g, const Bufs& b, int morph, bool image, const RunPlan& plan, hipStream_t s)
{
    return launch_binary_camp_t(g, b, 0, morph, image, plan, s);
}

// The prologue of a run with per-frame keys: raw camps and lower bounds (any int32 values: a device-side producer may write them, the host
// may never have seen them) -> effective keys, the ONE place the rule is applied on the device (frame_key_eff).  The pixel kernel reads
// key_eff, the sparse stage key_enemy, rmcv_batch_get_frame_keys key_eff.  lbs null: the run's bound for every frame.
__global__ __launch_bounds__(256) void k_frame_keys(const int32_t* __restrict__ camps, const int32_t* __restrict__ lbs, int run_lb,
                                                   FrameKey* __restrict__ eff, int32_t* __restrict__ enemy, int n_frames)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_frames) {
        const int32_t camp = camps[f];
        eff[f] = frame_key_eff(camp, lbs ? lbs[f] : run_lb);
        enemy[f] = camp; // objdetect.cpp:83, :124-129: the label verbatim
    }
}

hipError_t launch_frame_keys(const Geom& g, const Bufs& b, int run_lower_bound, hipStream_t s)
{
    return launch(k_frame_keys, dim3((g.n_frames + 255) / 256), dim3(256), 0, s, b.key_camps, b.key_lbs, run_lower_bound, b.key_eff, b.key_enemy,
                  g.n_frames);
}

} // namespace rmcv
