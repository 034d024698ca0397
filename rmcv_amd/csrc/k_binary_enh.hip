// k_binary_enh.hip -- the pixel kernel reading through a frame's gamma table (RMCV_OPT_ENHANCE: rm::AutoEnhance fused into the
// pixel pass).  k_binary_kernel.inc compiled with K1_ENH: the same loaders, planes, morphology and stores under the name k_binary_enh,
// with thresh16_m -- one lookup of the frame's threshold table per pixel -- in place of thresh16.  Its own translation unit, so that
// k_binary.hip's kernels are not touched by it; never the wave-specialised shape.
// Three items per wave in flight (12 loads) instead of four: the lookups' addresses and results live beside the loaded dwords, and
// with four the kernel passes the 80 VGPRs of k_binary's budget (74-77 with three, no scratch).
#define RMCV_K1_UNROLL 3
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "k_binary_device.h"

namespace rmcv {

#define K1_ENH 1
#define K1_KERNEL k_binary_enh
#define K1_THRESH(d) thresh16_m<CA, CB>(d, s_m)
#define K1_PASS(a, b) ((a) >= (int)s_m[b])
#include "k_binary_kernel.inc"

#define K1_LAUNCH_T launch_binary_enh_t
#define K1_EXTRA , b.enh_m + (int64_t)f0 * 256
#include "k_binary_launch.inc"

hipError_t launch_binary_enh(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s)
{
    return with_channel_pair(frame_key_eff(camp, lower_bound), [&](auto ca, auto cb) { return launch_binary_enh_t<ca, cb>(g, b, lower_bound, morph, image, plan, s); });
}

} // namespace rmcv
