// pixel_plan.h -- what a run's pixel stage launches: which of the six kernel variants a batch takes, which combinations of modes are
// refused, and the launch shape of k_binary_launch.inc (loader, chunks of frames below 4 GiB, persistent grid, taper, k_binary_ws or not).
// Pure functions of plain values, without HIP types, so that a host compiler alone can check them (tests/test_pixel_plan.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/rmcv_abi.h"

#ifdef __HIPCC__
#define RMCV_PLAN_FN __host__ __device__ inline
#else
#define RMCV_PLAN_FN inline
#endif

namespace rmcv {

#ifndef RMCV_SR
#define RMCV_SR 32
#endif
static constexpr int STRIP_ROWS = RMCV_SR;   // rows of a k_binary strip (k_binary.hip: SR); the sparse kernel's frame queues follow its strip order

// ---- the variant: which pixel kernel a batch takes (the table of variants) ----
enum PixelVariant { PIXEL_BGR = 0, PIXEL_BAYER, PIXEL_ENH, PIXEL_WIN, PIXEL_CAMP, PIXEL_CAMP_WIN };
struct PixelVariantInfo {
    const char* kernel; // what a failed launch is reported as
    const char* step;   // a pipeline's name for the whole step, prologue kernels included
    bool ws;            // the variant can take the wave-specialised shape (k_binary_ws) when the plan asks for it
};
static constexpr PixelVariantInfo PIXEL_VARIANTS[6] = {
    {"k_binary", "the pixel kernel (k_binary / k_binary_ws)", true},
    {"k_binary_bayer", "the pixel kernel (k_binary_bayer)", false},
    {"k_binary_enh", "k_frame_sums, k_enhance_table, the pixel kernel (k_binary_enh)", false},
    {"k_binary_win", "k_window_origins, the pixel kernel (k_binary_win)", false},
    {"k_binary_camp", "k_frame_keys, the pixel kernel (k_binary_camp / k_binary_camp_win)", false},
    {"k_binary_camp_win", "k_frame_keys, the pixel kernel (k_binary_camp / k_binary_camp_win)", false},
};
// input_format: RMCV_OPT_INPUT_FORMAT of the frames; enhance: RMCV_OPT_ENHANCE; win: read through windows; keys: per-frame detection keys
constexpr PixelVariant pixel_variant(int input_format, int enhance, int win, int keys)
{
    return input_format != RMCV_INPUT_BGR ? PIXEL_BAYER : enhance ? PIXEL_ENH : keys ? (win ? PIXEL_CAMP_WIN : PIXEL_CAMP) : win ? PIXEL_WIN : PIXEL_BGR;
}

// ---- the refusals: the message a combination of modes fails with, or null.  windows / keys / legacy: what the caller is about to bind
// or run; input_format / enhance: what the frames are (or are about to be) read as.  One order for every caller: the legacy matcher's
// own, per-frame keys', windows', the two options against each other; format before enhancement in each.
inline const char* pixel_refusal(int input_format, int enhance, bool windows, bool keys, bool legacy)
{
    const bool bayer = input_format != RMCV_INPUT_BGR;
    if (legacy) {
        if (bayer) return "the legacy matcher votes camps from BGR means: not for Bayer frames (RMCV_OPT_INPUT_FORMAT)";
        if (enhance) return "the legacy matcher votes camps from BGR means: not with RMCV_OPT_ENHANCE";
        if (keys) return "the legacy matcher votes a camp per blob from BGR means: not with per-frame camps (rmcv_batch_set_frame_camps)";
    }
    if (keys) {
        if (bayer) return "per-frame camps with a Bayer input format (RMCV_OPT_INPUT_FORMAT): the mosaic kernel takes one camp per run; not supported";
        if (enhance) return "per-frame camps with RMCV_OPT_ENHANCE: the threshold table folds one lower bound per run; not supported";
    }
    if (windows) {
        if (bayer) return "windows with a Bayer input format (RMCV_OPT_INPUT_FORMAT): crop-then-demosaic has other border semantics; not supported";
        if (enhance) return "windows with RMCV_OPT_ENHANCE: the mean of a crop is not the frame's; not supported";
    }
    if (bayer && enhance) return "RMCV_OPT_ENHANCE with a Bayer input format: the mean of a demosaiced frame is not a function of the mosaic's sums";
    return nullptr;
}

// ---- the effective detection key of a frame, the one place it is computed -- by k_frame_keys on the device, by
// rmcv_frame_key and by every pixel launcher on the host: raw camp and lower bound, any int32 (a device-side producer may write them),
// -> what the pixel kernels use.
//   channel pair (imgproc.cpp:56-65, BGR byte order): GUIDELIGHT G-R; BLUE B-R; every other value R-B
//   bound (inRange(gray, lb, 255) on a saturated u8 difference): lb <= 0 every pixel passes; lb > 255 none; otherwise a - b >= lb
struct FrameKey {
    int32_t ca, cb;   // byte of channel A / channel B inside a BGR pixel
    int32_t lb;       // effective bound, 1 .. 256
    int32_t all_pass; // 1: every pixel passes (lb is 1 then)
};
RMCV_PLAN_FN FrameKey frame_key_eff(int32_t camp, int32_t lower_bound)
{
    FrameKey k;
    k.ca = camp == RMCV_CAMP_GUIDELIGHT ? 1 : (camp == RMCV_CAMP_BLUE ? 0 : 2);
    k.cb = (camp == RMCV_CAMP_GUIDELIGHT || camp == RMCV_CAMP_BLUE) ? 2 : 0;
    k.all_pass = lower_bound <= 0 ? 1 : 0;
    k.lb = lower_bound <= 0 ? 1 : (lower_bound > 256 ? 256 : lower_bound);
    return k;
}
// ---- the effective camera of a frame, the one place it is computed -- by k_pnp on the device, by rmcv_frame_camera and the
// host setter on the host: a raw index, any int32 (a device-side producer may write it), -> an entry of the context's camera table.
// Every value outside 0 .. n_cameras - 1 is camera 0.
RMCV_PLAN_FN int32_t frame_camera_eff(int32_t idx, int32_t n_cameras) { return (uint32_t)idx < (uint32_t)n_cameras ? idx : 0; }

// A key's channel pair as compile-time values: fn(CA, CB) with std::integral_constants, for the launchers whose kernels are templates
// over the pair.  The three pairs frame_key_eff can give: <1, 2>, <0, 2>, <2, 0>.
template <typename Fn>
inline auto with_channel_pair(const FrameKey& k, Fn&& fn)
{
    if (k.ca == 1) return fn(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
    if (k.ca == 0) return fn(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
    return fn(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
}

// ---- the shape of k_binary_launch.inc's launches (every variant but PIXEL_BAYER, whose loader and strips are its own) ----
struct PixelBatch {
    PixelVariant variant;
    int n_frames, w, h, ww, stride;     // Geom's (a windowed batch: the window's w, h, ww; the frames' stride and pitch)
    int64_t frame_pitch, plane_pitch;
    int n_cu, pixel_rowquad;
    bool base_aligned;                  // the first frame starts on a 16-byte boundary
    int lower_bound;                    // the run's (the keyed variants read every frame's own and ignore it)
    int pixel_ws, pixel_groups;         // RunPlan's
};
struct PixelShape {
    int strips;               // strips of a frame
    int lb, all_pass;         // frame_key_eff of the run's bound; the keyed variants are handed lb = 1, all_pass = 1, which their kernels ignore
    int chunk;                // frames per launch: every extent (input, byte image, bit plane) of a launch below 4 GiB - 4 KiB
    int mode;                 // the loader, the kernels' FAST: 0 byte-wise, 1 row quads, 2 linear (rows contiguous; never with windows)
    size_t planes, planes_ws; // dynamic LDS of k_binary's shape and of k_binary_ws
    int n_cu, groups;         // compute units and workgroups per CU the persistent grid is sized for
    bool ws_wanted;           // everything k_binary_ws asks of the batch; a chunk takes it unless it is tapered (pixel_chunk)
    bool ws_full;             // the batch is ONE launch of k_binary_ws with a workgroup on every CU (a pipeline holds a burst's second launch back for it)
};
struct PixelChunk {
    int n_blocks;               // strips of the launch
    int grid;                   // workgroups of k_binary's shape
    int taper_head, taper_tail; // strips handed out as four 8-row pieces
    bool ws;                    // the launch is k_binary_ws ...
    int grid_ws;                // ... with this many 1024-thread workgroups
};

// nf: the frames of one launch (PixelShape::chunk of them; the last launch of a batch may have fewer)
inline PixelChunk pixel_chunk(const PixelShape& s, int nf)
{
    PixelChunk c{};
    c.n_blocks = nf * s.strips;
    const int cap = (c.n_blocks + 7) & ~7;
    // persistent grid: RMCV_OPT_PIXEL_GROUPS workgroups per CU: alone the kernel is equally fast with 2 and 3 and slower with 4 and
    // more; 2 leaves room on every CU for the kernels of the other batches in flight
    c.grid = s.n_cu * s.groups;
    if (c.grid > cap) c.grid = cap;
    c.grid = (c.grid + 7) & ~7;
    // A launch with fewer strips than half the CUs (one camera frame = 32 strips on 256 CUs: the per-frame drop-in chain) hands
    // EVERY strip out as four 8-row pieces: four times the workgroups, a quarter of the rows each (15 -> 7 us for one frame).
    if (c.n_blocks * 2 <= s.n_cu) {
        c.taper_head = (c.n_blocks + 7) >> 3; // strips per XCD
        c.taper_tail = 0;
        c.grid = (4 * c.n_blocks + 7) & ~7;
    }
    // whole batches with contiguous rows, when the caller asks for it (RMCV_OPT_PIXEL_SHAPE; a pipeline does for its calm batches):
    // the wave-specialised kernel, ONE 1024-thread workgroup per CU
    c.ws = s.ws_wanted && c.taper_head == 0;
    c.grid_ws = (s.n_cu + 7) & ~7;
    if (c.grid_ws > cap) c.grid_ws = cap;
    return c;
}

inline PixelShape pixel_shape(const PixelBatch& b)
{
    const auto max64 = [](int64_t x, int64_t y) { return x > y ? x : y; };
    const bool win = b.variant == PIXEL_WIN || b.variant == PIXEL_CAMP_WIN, keyed = b.variant == PIXEL_CAMP || b.variant == PIXEL_CAMP_WIN;
    PixelShape s{};
    s.strips = (b.h + STRIP_ROWS - 1) / STRIP_ROWS;
    const FrameKey key = frame_key_eff(0, keyed ? 0 : b.lower_bound);
    s.lb = key.lb;
    s.all_pass = key.all_pass;
    s.planes = (size_t)2 * (STRIP_ROWS + 4) * b.ww * sizeof(uint64_t);
    s.planes_ws = ((size_t)2 * (STRIP_ROWS + 4) + STRIP_ROWS) * b.ww * sizeof(uint64_t);
    const bool aligned = (b.w % 64 == 0) && (b.stride % 16 == 0) && (b.frame_pitch % 16 == 0) && b.base_aligned;
    // The FAST path addresses its buffers with 32-bit offsets, so one launch covers at most as many frames as keep every extent
    // (input, byte image, bit plane) below 4 GiB - 256; a larger batch (288 GB of HBM hold 70 000 frames) is a few launches in a
    // row on the same stream, each with its pointers advanced -- not a fall-back to the byte-wise loader.
    const int64_t lim = 0xFFFFF000ll;
    const int64_t per_frame = max64(max64(b.frame_pitch, b.plane_pitch * 8), (int64_t)b.w * b.h);
    const int64_t fit = max64(1, (lim - 1) / per_frame);
    s.chunk = aligned && fit < b.n_frames ? (int)fit : b.n_frames;
    const bool fast = aligned && (int64_t)s.chunk * per_frame < lim;
    // rows contiguous in memory: the linear loader (Geom::pixel_rowquad, hidden option 1001: the row-quad loader everywhere -- for A/B
    // runs).  Window rows are not contiguous: never the linear loader.
    const bool linear = fast && !win && !b.pixel_rowquad && b.stride == 3 * b.w;
    s.mode = fast ? (linear ? 2 : 1) : 0;
    s.n_cu = b.n_cu > 0 ? b.n_cu : 256; // n_cu: of the context's own device
    s.groups = b.pixel_groups > 0 ? b.pixel_groups : 4;
    s.ws_wanted = PIXEL_VARIANTS[b.variant].ws && b.pixel_ws && linear && !s.all_pass && s.planes_ws <= 60 * 1024;
    const PixelChunk whole = pixel_chunk(s, b.n_frames);
    s.ws_full = s.chunk == b.n_frames && whole.ws && whole.n_blocks >= s.n_cu;
    return s;
}

} // namespace rmcv
