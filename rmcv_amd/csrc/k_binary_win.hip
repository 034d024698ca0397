// k_binary_win.hip -- the pixel kernel reading a WINDOW of every frame (rmcv_batch_set_windows: tracked-ROI detection, the reference's
// extract_color(image(roi))).  k_binary_kernel.inc compiled with K1_WIN: the same loaders, planes, morphology and stores under the name
// k_binary_win; w and h are the window's, and frame f is read from its effective origin (Bufs::win_eff) on -- fbase / frame gain
// y_eff * stride + 3 * x_eff, the raw-buffer extent covers the whole frames.  Byte image, bit planes and row masks are window-sized, so
// everything behind the pixel pass runs on a batch of win_w x win_h images and never knows.  Its own translation unit, so that k_binary.hip's
// and k_binary_enh.hip's kernels are not touched by it.  Window rows are not contiguous in memory: the row-quad loader (FAST 1) when
// win_w % 64 == 0 and stride, pitch and base are 16-byte aligned, the byte-wise loader otherwise; never the linear loader, never k_binary_ws.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "k_binary_device.h"

namespace rmcv {

#define K1_ENH 0
#define K1_WIN 1
#define K1_KERNEL k_binary_win
#define K1_THRESH(d) thresh16<CA, CB>(d, lb)
#define K1_PASS(a, b) ((a) - (b) >= lb)
#include "k_binary_kernel.inc"

#define K1_LAUNCH_T launch_binary_win_t
// the launch's slice of the effective-origin table, and the bytes its whole frames span (launches are chunks of frames: f0, nf)
#define K1_EXTRA , b.win_eff + f0, (int)((int64_t)(nf - 1) * g.frame_pitch + (int64_t)(g.frame_h - 1) * g.stride + 3 * (int64_t)g.frame_w)
#include "k_binary_launch.inc"

hipError_t launch_binary_win(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s)
{
    return with_channel_pair(frame_key_eff(camp, lower_bound), [&](auto ca, auto cb) { return launch_binary_win_t<ca, cb>(g, b, lower_bound, morph, image, plan, s); });
}

// The prologue of a windowed run: requested origins (any int32 values: they come from a tracker on the device, the host may never have
// seen them) -> effective origins, the ONE place the rule is applied on the device (window_origin_eff).  Every consumer -- the pixel
// kernel, the classifier, the legacy matcher's camp vote, the pose stage, rmcv_batch_get_windows -- reads the table this writes.
__global__ __launch_bounds__(256) void k_window_origins(const rmcv_point* __restrict__ req, rmcv_point* __restrict__ eff, int n_frames,
                                                       int frame_w, int frame_h, int win_w, int win_h)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_frames) eff[f] = window_origin_eff(req[f], frame_w, frame_h, win_w, win_h);
}

hipError_t launch_window_origins(const Geom& g, const Bufs& b, hipStream_t s)
{
    return launch(k_window_origins, dim3((g.n_frames + 255) / 256), dim3(256), 0, s, b.win_req, b.win_eff, g.n_frames, g.frame_w, g.frame_h, g.w, g.h);
}

} // namespace rmcv
