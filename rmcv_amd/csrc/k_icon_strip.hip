// k_icon_strip.hip -- the labeler's icon strip: for n chosen frames of a batch, what executable/svm/labeler.cpp:93-106 shows the
// person labelling -- rm::affine_correction(frame, tmp, armour.icon, {side, side}) of every armour, side by side -- written into the caller's
// device memory.  The rule is icon_image (device_icon_image.h), icon_row at a run-time output size; rmcv_icon_strip_host (icon_host.h) states
// it on the CPU.
//
// Mapping (gfx950, wave64), one launch:
//   k_icon_strip*   one wavefront per (view k, slot j < cap), four to a workgroup; the grid is fixed by n x cap, never by data.  The wavefront
//                   of a slot below the frame's armour count, clampi(n_armours[f], 0, min(max_armours, cap)), computes the icon of armour j --
//                   the lane owns the output pixel, as in icon_row -- and stores it at columns [j side, (j + 1) side) of rows [0, side) of
//                   strip k; every other slot's wavefront stores zeros there.  The cap wavefronts of a view share the zeros of the strip's
//                   remainder [cap side, strip_w): the kernel defines every byte of the strip, with no memset in front of it.
// Stores: three bytes per lane and pixel, 192 consecutive bytes per wavefront and step.  Staging a step's pixels in LDS and storing 48 dwords
// was built and measured (profiles/icon_strip_bench.json): 1.2 % slower at side 20, 1.5 % faster at side 80 -- the kernel's time is
// the warp's arithmetic, not its stores -- so the variant without LDS and with one store path stays.  The armour table is only read.  No
// scratch, no LDS.
#include "device_icon_image.h"

namespace rmcv {

__device__ inline int clampis(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// BAYER as device_classify.h: 0 BGR (WIN: through the frame's window origin), 1 mosaics (pattern, lay), 2 through the gamma tables (luts)
template <int BAYER, bool WIN>
__device__ __forceinline__ void icon_strip(const IconStripJob& S, int pattern, int lay, const uint8_t* __restrict__ luts)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= S.n * S.cap) return;
    const int k = g / S.cap, j = g - k * S.cap, side = S.side;
    const int f = S.view_frames ? S.view_frames[k] : k;
    const int na = clampis(S.n_armours[f], 0, S.max_armours < S.cap ? S.max_armours : S.cap);
    uint8_t* __restrict__ strip = S.out + (int64_t)k * S.out_pitch;
    uint8_t* __restrict__ slot = strip + 3 * (int64_t)j * side;
    if (j < na) {
        const rmcv_armour* A = S.armours + (int64_t)f * S.max_armours + j;
        const uint8_t* frame = S.frames + (int64_t)f * S.frame_pitch + (WIN ? frame_origin_offset(S.win_eff, f, S.stride) : 0);
        float ic[4][2];
        icon_image<BAYER>(frame, f, lane, A, S.w, S.h, S.stride, pattern, lay, luts, side, side, ic, [&](int o, const int (&res)[3]) __attribute__((always_inline)) {
            const int dy = o / side, dx = o - dy * side;
            uint8_t* p = slot + (int64_t)dy * S.out_stride + 3 * dx;
#pragma unroll
            for (int c = 0; c < 3; c++) p[c] = (uint8_t)res[c];
        });
    } else {
        const int row_bytes = 3 * side;
        for (int o = lane; o < side * row_bytes; o += 64) {
            const int dy = o / row_bytes;
            slot[(int64_t)dy * S.out_stride + (o - dy * row_bytes)] = 0;
        }
    }
    // the remainder of the strip's rows, a share per slot: bytes [rem * j / cap, rem * (j + 1) / cap) behind the last slot
    const int rem = 3 * (S.strip_w - S.cap * side);
    const int r0 = (int)((int64_t)rem * j / S.cap), r1 = (int)((int64_t)rem * (j + 1) / S.cap);
    uint8_t* __restrict__ tail = strip + 3 * (int64_t)S.cap * side;
    for (int dy = 0; dy < side; dy++)
        for (int b = r0 + lane; b < r1; b += 64) tail[(int64_t)dy * S.out_stride + b] = 0;
    if (S.counts && j == 0 && lane == 0) S.counts[k] = na;
}

__global__ __launch_bounds__(256) void k_icon_strip(IconStripJob S) { icon_strip<0, false>(S, 0, 0, nullptr); }
__global__ __launch_bounds__(256) void k_icon_strip_win(IconStripJob S) { icon_strip<0, true>(S, 0, 0, nullptr); }
__global__ __launch_bounds__(256) void k_icon_strip_bayer(IconStripJob S, int pattern, int lay) { icon_strip<1, false>(S, pattern, lay, nullptr); }
__global__ __launch_bounds__(256) void k_icon_strip_enh(IconStripJob S, const uint8_t* __restrict__ luts) { icon_strip<2, false>(S, 0, 0, luts); }

static dim3 strip_grid(const IconStripJob& S) { return dim3((unsigned)(((int64_t)S.n * S.cap + 3) / 4)); }

hipError_t launch_icon_strip(const IconStripJob& S, hipStream_t s) { return launch(k_icon_strip, strip_grid(S), dim3(256), 0, s, S); }

// the strips of the batch bound to (g, b): the kernel by the batch's kind, as launch_harvest dispatches (k_harvest.hip)
hipError_t launch_icon_strip(const Geom& g, const Bufs& b, const Limits& lim, const int32_t* d_frames, int n, int side, int cap, int strip_w, uint8_t* d_out,
                             int out_stride, int64_t out_pitch, int32_t* d_counts, hipStream_t s)
{
    IconStripJob S{};
    S.frames = b.frames, S.frame_pitch = g.frame_pitch, S.stride = g.stride, S.w = g.w, S.h = g.h, S.max_armours = lim.max_armours;
    S.armours = b.armours, S.n_armours = b.n_armours, S.win_eff = g.win ? b.win_eff : nullptr, S.view_frames = d_frames;
    S.n = n, S.side = side, S.cap = cap, S.strip_w = strip_w, S.out = d_out, S.out_stride = out_stride, S.out_pitch = out_pitch, S.counts = d_counts;
    if (g.input_format != RMCV_INPUT_BGR)
        return launch(k_icon_strip_bayer, strip_grid(S), dim3(256), 0, s, S, g.input_format, raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient));
    if (g.enhance) return launch(k_icon_strip_enh, strip_grid(S), dim3(256), 0, s, S, b.enh_lut);
    if (g.win) return launch(k_icon_strip_win, strip_grid(S), dim3(256), 0, s, S);
    return launch(k_icon_strip, strip_grid(S), dim3(256), 0, s, S);
}

} // namespace rmcv

// ---- the host side (icon_host.h): no context, no device ----
#include "icon_host.h"

static_assert(rmcv::ICON_IMAGE_MAX == rmcv::ICON_SIDE_MAX, "the plan refuses what icon_image cannot take");

extern "C" {

int rmcv_affine_correction_host(const uint8_t* bgr, int w, int h, int stride, float icon[4][2], int ow, int oh, uint8_t* out, int out_stride,
                                int32_t* degenerate)
{
    if (rmcv::affine_host_refusal(bgr, icon, out, w, h, stride, ow, oh, out_stride)) return RMCV_ERR_BAD_ARG;
    const bool deg = rmcv::icon_affine_host(bgr, w, h, stride, icon, ow, oh, out, out_stride);
    if (degenerate) *degenerate = deg ? 1 : 0;
    return RMCV_OK;
}

int rmcv_icon_strip_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_armour* armours, int n, int side, int cap, uint8_t* out, int out_stride)
{
    if (rmcv::icon_strip_image_refusal(bgr, out, w, h, stride, armours, n, side, cap, out_stride)) return RMCV_ERR_BAD_ARG;
    rmcv::icon_strip_host(bgr, w, h, stride, armours, n, side, cap, cap * side, out, out_stride);
    return RMCV_OK;
}

int rmcv_sheet_size(int vw, int vh, int side, int32_t* sheet_w, int32_t* sheet_h)
{
    if (!sheet_w || !sheet_h || rmcv::sheet_size_refusal(vw, vh, side)) return RMCV_ERR_BAD_ARG;
    *sheet_w = 2 * vw;
    *sheet_h = vh + side;
    return RMCV_OK;
}

int rmcv_labeler_sheet_host(const uint8_t* bgr, int w, int h, int stride, const uint8_t* binary, int binary_stride, const rmcv_lightblob* blobs,
                            int n_blobs, const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours,
                            int vw, int vh, int side, int flags, uint8_t* out, int out_stride)
{
    if (!binary || binary_stride < w || rmcv::source_image_refusal(bgr, out, w, h, stride) || rmcv::sheet_size_refusal(vw, vh, side)) return RMCV_ERR_BAD_ARG;
    if (out_stride < 6 * (int64_t)vw) return RMCV_ERR_BAD_ARG;
    if (view_check_lists(w, h, w, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out_stride)) return RMCV_ERR_BAD_ARG;
    rmcv::labeler_sheet_host(bgr, w, h, stride, binary, binary_stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, vw, vh, side,
                             RMCV_ICON_STRIP_CAP_MAX, flags, out, out_stride);
    return RMCV_OK;
}

} // extern "C"
