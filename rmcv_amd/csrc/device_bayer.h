// device_bayer.h -- D(m), the library's demosaic of an 8-bit Bayer mosaic (include/rmcv_abi.h: RMCV_OPT_INPUT_FORMAT), one pixel at a
// time: rmcv_demosaic's kernel and the icon classifier's pixel accessor (device_classify.h) read the mosaic through it.  The pixel
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

} // namespace rmcv
