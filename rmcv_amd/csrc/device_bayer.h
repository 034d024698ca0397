// device_bayer.h -- D(m), the library's demosaic of an 8-bit Bayer mosaic (include/rmcv_abi.h: RMCV_OPT_INPUT_FORMAT), one pixel at a
// time: rmcv_demosaic's kernel and the icon classifier's pixel accessor (device_classify.h) read the mosaic through it (a frame in the
// sensor's own layout -- 16-bit samples, mirror, flip -- through bayer_bgr_raw below).  The pixel
// kernel (k_binary_bayer.hip) computes the same values sixteen pixels per lane and has to agree with this restatement bit for bit.
//
// Bilinear, in integers (OpenCV's 8-bit COLOR_Bayer*2BGR as recalled, not pinned):
//   own colour        m(x, y)
//   G at an R / B site                    (left + right + up + down + 2) >> 2
//   at a G site: the colour of its row    (left + right + 1) >> 1;   the colour of its column   (up + down + 1) >> 1
//   B at an R site / R at a B site        (four diagonal neighbours + 2) >> 2
// Border: D(m)(x, y) = D(m)(clamp(x, 1, w - 2), clamp(y, 1, h - 2)) -- the outer rows and columns repeat their interior neighbour,
// colour phase included.  w, h >= 3.
#pragma once
#include <stdint.h>

#include "../../include/rmcv_abi.h"

namespace rmcv {

// the R site of a pattern's top-left 2x2 block (RMCV_BAYER_RG 1: (0,0), GB 2: (0,1), GR 3: (1,0), BG 4: (1,1))
__host__ __device__ inline int bayer_rx(int pattern) { return (pattern == RMCV_BAYER_GR || pattern == RMCV_BAYER_BG) ? 1 : 0; }
__host__ __device__ inline int bayer_ry(int pattern) { return (pattern == RMCV_BAYER_GB || pattern == RMCV_BAYER_BG) ? 1 : 0; }

// out = {B, G, R} of D(m) at (x, y); m = the frame's first byte, rows `stride` bytes apart
__device__ inline void bayer_bgr(const uint8_t* __restrict__ m, int stride, int w, int h, int rx, int ry, int x, int y, int out[3])
{
    x = x < 1 ? 1 : (x > w - 2 ? w - 2 : x);
    y = y < 1 ? 1 : (y > h - 2 ? h - 2 : y);
    const uint8_t* r1 = m + (int64_t)y * stride;
    const uint8_t* r0 = r1 - stride;
    const uint8_t* r2 = r1 + stride;
    const int own = r1[x], hs = r1[x - 1] + r1[x + 1], vs = r0[x] + r2[x];
    const int ds = r0[x - 1] + r0[x + 1] + r2[x - 1] + r2[x + 1];
    const int px = (x ^ rx) & 1, py = (y ^ ry) & 1;
    int b, g, r;
    if (!px && !py) { r = own; g = (hs + vs + 2) >> 2; b = (ds + 2) >> 2; }      // R site
    else if (px && py) { b = own; g = (hs + vs + 2) >> 2; r = (ds + 2) >> 2; }   // B site
    else if (!py) { g = own; r = (hs + 1) >> 1; b = (vs + 1) >> 1; }             // G on an R row
    else { g = own; b = (hs + 1) >> 1; r = (vs + 1) >> 1; }                      // G on a B row
    out[0] = b;
    out[1] = g;
    out[2] = r;
}

// ---- the frame as the sensor delivers it (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT) ----
// A delivered buffer r is read as the 8-bit mosaic T(r)(x, y) = n(r(mirror ? w-1-x : x, flip ? h-1-y : y)), n(s) = (s >> valid_bit) & 0xFF
// for 2-byte samples.  The layout travels as one int: bit 0 = 2-byte samples, bit 1 = mirror, bit 2 = flip, bits 4..6 = the valid bit.
// 0 is the plain 8-bit mosaic.  Everything above the loaders works in ORIENTED coordinates with the pattern of T(r).
constexpr int LAY_S16 = 1, LAY_MIRROR = 2, LAY_FLIP = 4, LAY_VBIT_SHIFT = 4;
__host__ __device__ inline int raw_layout(int sample_bits, int valid_bit, int orient)
{
    return (sample_bits == 16 ? LAY_S16 | (valid_bit << LAY_VBIT_SHIFT) : 0) | ((orient & RMCV_ORIENT_MIRROR) ? LAY_MIRROR : 0) |
           ((orient & RMCV_ORIENT_FLIP) ? LAY_FLIP : 0);
}
__host__ __device__ inline int lay_bytes(int lay) { return (lay & LAY_S16) ? 2 : 1; }
__host__ __device__ inline int lay_vbit(int lay) { return (lay >> LAY_VBIT_SHIFT) & 7; }
// the R site of T(r) from the pattern of r as delivered: a mirrored column x is source column w-1-x, a flipped row y source row h-1-y
__host__ __device__ inline int raw_rx(int pattern, int lay, int w) { const int rx = bayer_rx(pattern); return (lay & LAY_MIRROR) ? (w - 1 - rx) & 1 : rx; }
__host__ __device__ inline int raw_ry(int pattern, int lay, int h) { const int ry = bayer_ry(pattern); return (lay & LAY_FLIP) ? (h - 1 - ry) & 1 : ry; }

// T(r)(x, y); r = the frame's first byte, rows `stride` BYTES apart (even, and r 2-byte aligned, with 2-byte samples)
__device__ inline int raw_px(const uint8_t* __restrict__ r, int stride, int w, int h, int lay, int x, int y)
{
    const int sx = (lay & LAY_MIRROR) ? w - 1 - x : x, sy = (lay & LAY_FLIP) ? h - 1 - y : y;
    const uint8_t* row = r + (int64_t)sy * stride;
    if (lay & LAY_S16) return (reinterpret_cast<const uint16_t*>(row)[sx] >> lay_vbit(lay)) & 0xFF;
    return row[sx];
}

// bayer_bgr of T(r): out = {B, G, R} of D(T(r)) at the oriented (x, y); rx, ry = the R site of T(r) (raw_rx, raw_ry)
__device__ inline void bayer_bgr_raw(const uint8_t* __restrict__ r, int stride, int w, int h, int rx, int ry, int lay, int x, int y, int out[3])
{
    x = x < 1 ? 1 : (x > w - 2 ? w - 2 : x);
    y = y < 1 ? 1 : (y > h - 2 ? h - 2 : y);
    int t[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) t[j][i] = raw_px(r, stride, w, h, lay, x - 1 + i, y - 1 + j);
    const int own = t[1][1], hs = t[1][0] + t[1][2], vs = t[0][1] + t[2][1];
    const int ds = t[0][0] + t[0][2] + t[2][0] + t[2][2];
    const int px = (x ^ rx) & 1, py = (y ^ ry) & 1;
    int b, g, rr;
    if (!px && !py) { rr = own; g = (hs + vs + 2) >> 2; b = (ds + 2) >> 2; }      // R site
    else if (px && py) { b = own; g = (hs + vs + 2) >> 2; rr = (ds + 2) >> 2; }   // B site
    else if (!py) { g = own; rr = (hs + 1) >> 1; b = (vs + 1) >> 1; }             // G on an R row
    else { g = own; b = (hs + 1) >> 1; rr = (vs + 1) >> 1; }                      // G on a B row
    out[0] = b;
    out[1] = g;
    out[2] = rr;
}

} // namespace rmcv
