// frame_source.h -- SRC(f), the BGR image a frame's results are defined on (source_view_plan.h: SourceKind), described once for every kernel
// that reads it: the source view (k_view_source.hip), the corner refinement (k_corner.hip) and the chessboard detector (k_chess.hip).  What a
// launch is told (FrameSource), its two fillers -- a bound batch, one packed image --, what a kernel makes of it for one frame (FramePixels,
// frame_pixels) and the choice of a kernel's instantiation by kind (with_source_kind).  The pixel readers stay with their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/rmcv_abi.h"
#include "bind_plan.h"
#include "device_bayer.h"
#include "source_view_plan.h"

namespace rmcv {

// Byte offset of what frame f's consumers read inside the frame: its window's effective origin; a null table is whole frames (0).
// Shared by the pixel kernel (k_binary_win), the classifier and the legacy matcher's camp vote; k_pnp adds the same origin as floats.
__host__ __device__ inline int64_t frame_origin_offset(const rmcv_point* __restrict__ win_eff, int f, int stride)
{
    return win_eff ? (int64_t)win_eff[f].y * stride + 3 * (int64_t)win_eff[f].x : 0;
}

// SRC(f) of every frame of a launch
struct FrameSource {
    int kind;                    // SourceKind (source_view_plan.h)
    const uint8_t* src;          // [frame] the frames as bound: BGR or mosaic, rows `stride` bytes apart, frames `frame_pitch`
    const uint8_t* src_end;      // one past the last byte bound: no load of k_view_source's reaches outside src .. src_end
    int stride;
    int64_t frame_pitch;
    int w, h;                    // the extent of SRC (a windowed batch's: the window's)
    int rx, ry, lay;             // a mosaic's R site and layout word (device_bayer.h: raw_rx, raw_ry, raw_layout of T(r))
    const uint8_t* lut;          // [frame][256] SOURCE_BGR_LUT: Bufs::enh_lut
    const rmcv_point* win_eff;   // [frame]      SOURCE_BGR_WIN: Bufs::win_eff
};

// the batch bound to g at `frames`, read as the run read it (enh_lut, win_eff: Bufs'; each is taken only by the kind that reads it)
inline FrameSource frame_source_of(const Geom& g, const uint8_t* frames, const uint8_t* enh_lut, const rmcv_point* win_eff)
{
    FrameSource s{};
    s.kind = source_kind(g);
    s.src = frames;
    s.src_end = frames + (int64_t)(g.n_frames - 1) * g.frame_pitch + (int64_t)(g.frame_h - 1) * g.stride + (int64_t)geom_pixel_bytes(g) * g.frame_w;
    s.stride = g.stride; s.frame_pitch = g.frame_pitch; s.w = g.w; s.h = g.h;
    if (g.input_format) {
        s.lay = raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient);
        s.rx = raw_rx(g.input_format, s.lay, g.w);
        s.ry = raw_ry(g.input_format, s.lay, g.h);
    }
    s.lut = s.kind == SOURCE_BGR_LUT ? enh_lut : nullptr;
    s.win_eff = s.kind == SOURCE_BGR_WIN ? win_eff : nullptr;
    return s;
}
// one BGR image of w x h at d, rows dstride bytes apart (a stage-wise helper's upload): the last row ends with its pixels
inline FrameSource frame_source_packed(const uint8_t* d, int w, int h, int dstride)
{
    FrameSource s{};
    s.kind = SOURCE_BGR;
    s.src = d;
    s.src_end = d + (size_t)dstride * (h - 1) + (size_t)3 * w;
    s.stride = dstride; s.frame_pitch = (int64_t)dstride * h; s.w = w; s.h = h;
    return s;
}

// One frame of a FrameSource as a kernel reads it.  frame: the frame's first byte, a windowed batch's at its effective origin; lut: the
// frame's table (SOURCE_BGR_LUT, null otherwise)
struct FramePixels {
    const uint8_t* frame;
    const uint8_t* lut;
    int stride, w, h, rx, ry, lay;
};
template <int SRC>
__device__ inline FramePixels frame_pixels(const FrameSource& s, int f)
{
    FramePixels P;
    P.frame = s.src + (int64_t)f * s.frame_pitch + (SRC == SOURCE_BGR_WIN ? frame_origin_offset(s.win_eff, f, s.stride) : 0);
    P.lut = SRC == SOURCE_BGR_LUT ? s.lut + (int64_t)f * 256 : nullptr;
    P.stride = s.stride; P.w = s.w; P.h = s.h; P.rx = s.rx; P.ry = s.ry; P.lay = s.lay;
    return P;
}

// fn(std::integral_constant<int, kind>{}) for the five kinds: the one place a kernel's instantiation is chosen
template <class Fn>
inline hipError_t with_source_kind(int kind, Fn fn)
{
    switch (kind) {
    case SOURCE_BGR: return fn(std::integral_constant<int, SOURCE_BGR>{});
    case SOURCE_BGR_WIN: return fn(std::integral_constant<int, SOURCE_BGR_WIN>{});
    case SOURCE_MOSAIC: return fn(std::integral_constant<int, SOURCE_MOSAIC>{});
    case SOURCE_MOSAIC_RAW: return fn(std::integral_constant<int, SOURCE_MOSAIC_RAW>{});
    case SOURCE_BGR_LUT: return fn(std::integral_constant<int, SOURCE_BGR_LUT>{});
    }
    return hipErrorInvalidValue; // (no kernel for the kind: an error, never another path)
}

} // namespace rmcv
