// k_binary_camp_win.hip -- per-frame detection keys AND windows: k_binary_kernel.inc compiled with K1_CAMP and K1_WIN under the name
// k_binary_camp_win.  What k_binary_win.hip says of windows (effective origins, the extent of whole frames, row-quad or byte-wise loader, never
// the linear one) and what k_binary_camp.hip says of keys (read once per strip, phase 1 in the pair's instantiation) both hold.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "k_binary_device.h"

namespace rmcv {

#define K1_ENH 0
#define K1_WIN 1
#define K1_CAMP 1
#define K1_KERNEL k_binary_camp_win
#define K1_THRESH(d) thresh16<CA, CB>(d, lb)
#define K1_PASS(a, b) ((a) - (b) >= lb)
#include "k_binary_kernel.inc"

#define K1_LAUNCH_T launch_binary_camp_win_t
// the launch's slices of the effective-origin and key tables, and the bytes its whole frames span (launches are chunks of frames: f0, nf)
#define K1_EXTRA , b.win_eff + f0, (int)((int64_t)(nf - 1) * g.frame_pitch + (int64_t)(g.frame_h - 1) * g.stride + 3 * (int64_t)g.frame_w), b.key_eff + f0
#include "k_binary_launch.inc"

hipError_t launch_binary_camp_win(const Geom& g, const Bufs& b, int morph, bool image, const RunPlan& plan, hipStream_t s)
{
    return launch_binary_camp_win_t(g, b, 0, morph, image, plan, s);
}

} // namespace rmcv
