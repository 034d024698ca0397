// k_binary.hip -- K1: the pixel-streaming part of rm::extract_color
// (/root/reference/src/imgproc.cpp:52-69): split + saturating channel subtract + inRange + 3x3
// MORPH_CLOSE, fused into ONE pass over the BGR frame.
//
// HBM-bound (no MFMA: there is no contraction here).  Algorithmic traffic: 3 B/px read +
// 1 B/px written (the reference returns `binary`, imgproc.cpp:74) = 4 B/px; the bit plane the
// contour stage consumes adds 1/8 B/px.  The reference's CPU path makes ~8 full-frame passes
// (split x3, subtract, inRange, dilate, erode, findContours' copy); here every intermediate lives
// in registers or LDS:
//
//   phase 1  a wave loads a 256-px block of four rows with four coalesced dwordx3 (lane i: pixels 4i..4i+3 of each
//            row), thresholds its 16 px to a 16-bit mask, a lane quad transposes its 4x4 nibbles (2 DPP exchanges) and
//            each lane writes 16 bits of one row of the strip's bit plane T in LDS
//   phase 2  dilate on the bit plane  D = hdil(T[y-1] | T[y] | T[y+1])          (64 px / lane-op)
//   phase 3  erode                    E = hero(D[y-1] & D[y] & D[y+1])
//   phase 4  E -> 0/255 bytes, 16 px per lane, one coalesced dwordx4 store; E word -> bit plane
//
// A workgroup owns a strip of SR rows of one frame (+2 halo rows per side for CLOSE); strips are
// mapped so that consecutive strips of a frame land on the same XCD (blockIdx % 8 groups), where the
// halo rows they share are L2 hits.  Border semantics (OpenCV morphologyDefaultBorderValue): samples
// outside the image never win, i.e. they read 0 for the dilate and 1 for the erode.
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "k_binary_device.h"

namespace rmcv {

#define K1_ENH 0
#define K1_KERNEL k_binary
#define K1_THRESH(d) thresh16<CA, CB>(d, lb)
#define K1_PASS(a, b) ((a) - (b) >= lb)
#include "k_binary_kernel.inc"

#include "k_binary_ws.inc"

static std::atomic<int64_t> g_ws_launches{0};
int64_t pixel_ws_launches() { return g_ws_launches.load(std::memory_order_relaxed); }
static std::atomic<int64_t> g_image_delta_launches{0};
int64_t pixel_image_delta_launches() { return g_image_delta_launches.load(std::memory_order_relaxed); }
static std::atomic<int64_t> g_plane_delta_launches{0};
int64_t pixel_plane_delta_launches() { return g_plane_delta_launches.load(std::memory_order_relaxed); }
#define K1_LAUNCH_T launch_binary_t
#define K1_EXTRA
#include "k_binary_launch.inc"

hipError_t launch_binary(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s,
                         ImageState* img, int* plane)
{
    const PixelVariant v = pixel_variant(g.input_format, g.enhance, g.win, g.keys);
    // imgproc.cpp:56-65: GUIDELIGHT G-R; BLUE B-R; everything else (RED, NEUTRAL) R-B.  BGR byte order.
    if (v == PIXEL_BGR)
        return with_channel_pair(frame_key_eff(camp, lower_bound), [&](auto ca, auto cb) { return launch_binary_t<ca, cb>(g, b, lower_bound, morph, image, plan, s, img, plane); });
    // the other kernels store every byte of the image and know nothing of its mask (image_plan.h: IMAGE_KERNEL_OTHER)
    const ImageLaunch l = {IMAGE_KERNEL_OTHER, image, g.w, g.h, g.ww, g.n_frames};
    const ImageState before = img ? *img : IMAGE_STATE_UNKNOWN;
    if (img) *img = image_step(before, l, false).next;
    if (plane) *plane = 0; // (plane_step: no other kernel keeps the plane in step with the image)
    hipError_t e = hipSuccess;
    switch (v) {
    case PIXEL_BGR: break;
    // a Bayer mosaic (RMCV_OPT_INPUT_FORMAT): its own kernel (k_binary_bayer.hip)
    case PIXEL_BAYER: e = launch_binary_bayer(g, b, camp, lower_bound, morph, image, s); break;
    // through the frames' gamma tables (RMCV_OPT_ENHANCE): the same kernel with a lookup in its compare (k_binary_enh.hip)
    case PIXEL_ENH: e = launch_binary_enh(g, b, camp, lower_bound, morph, image, plan, s); break;
    // a window of every frame (rmcv_batch_set_windows): the same kernel reading from the frames' effective origins (k_binary_win.hip)
    case PIXEL_WIN: e = launch_binary_win(g, b, camp, lower_bound, morph, image, plan, s); break;
    // per-frame detection keys (rmcv_batch_set_frame_camps): the same kernel reading camp and bound per strip (k_binary_camp.hip), windows or not
    case PIXEL_CAMP: e = launch_binary_camp(g, b, morph, image, plan, s); break;
    case PIXEL_CAMP_WIN: e = launch_binary_camp_win(g, b, morph, image, plan, s); break;
    }
    if (img && e == hipSuccess) *img = image_step(before, l, true).next;
    return e;
}

// binary (0 / non-zero bytes) -> padded bit plane; used when a caller hands in its own binary image
__global__ void k_pack_bits(const uint8_t* __restrict__ binary, int w, int h, int ww, uint64_t* __restrict__ bits, int prow,
                            int64_t plane_pitch, uint32_t* __restrict__ rowmask)
{
    const int f = blockIdx.y;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= h * ww) return;
    const int y = item / ww, k = item % ww;
    const uint8_t* row = binary + (int64_t)f * w * h + (int64_t)y * w;
    uint64_t word = 0;
    for (int bqt = 0; bqt < 64; bqt++) {
        int x = k * 64 + bqt;
        if (x < w && row[x]) word |= 1ull << bqt;
    }
    bits[(int64_t)f * plane_pitch + (int64_t)(y + 1) * prow + 1 + k] = word;
    if (word && k < 32) atomicOr(&rowmask[(int64_t)f * h + y], 1u << k); // caller zeroes the masks first
}

// (the image then is the caller's: whoever fills Bufs::binary for this sets the context's ImageState to IMAGE_STATE_UNKNOWN)
hipError_t launch_pack_bits(const Geom& g, const Bufs& b, hipStream_t s)
{
    const int items = g.h * g.ww;
    hipError_t e = hipMemsetAsync(b.rowmask, 0, (size_t)g.n_frames * g.h * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    return launch(k_pack_bits, dim3((items + 255) / 256, g.n_frames), dim3(256), 0, s, b.binary, g.w, g.h, g.ww, b.bits,
                       g.prow, g.plane_pitch, b.rowmask);
}

} // namespace rmcv
