// k_binary_bayer.hip -- K1 for raw Bayer frames (RMCV_OPT_INPUT_FORMAT 1..4; 8-bit mosaics, or the sensor's own layout -- 16-bit samples,
// mirror, flip: RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT, read as the oriented 8-bit mosaic T(r) by the loader): demosaic + split + saturating channel subtract
// + inRange + 3x3 MORPH_CLOSE in ONE pass over the mosaic.  The contract (include/rmcv_abi.h): every output for a mosaic m equals
// what k_binary gives for the BGR frame D(m) (device_bayer.h), so this kernel writes exactly what k_binary writes -- the byte image
// (unless RMCV_STAGE_NO_IMAGE), the padded plane F and the row masks -- and everything downstream is the BGR path's.
//
// Traffic: 1 B/px read + 1 B/px written (+ 1/8 for the plane) = 2.125 B/px, 1.125 with RMCV_STAGE_NO_IMAGE, against k_binary's 4.
// Only the two channels the camp subtracts are estimated (R and B; G and R for the guide light), never a colour frame.
//
//   phase 1  a lane owns 16 pixels of a column group and walks down a band of rows.  It holds three mosaic rows (y-1, y, y+1) of
//            its 16 pixels in registers -- one coalesced dwordx4 per row, the +-1-column bytes from the neighbouring lanes
//            (ds_bpermute), a wave's edge lanes load theirs -- so every mosaic row of the band is read once.  The two estimates are
//            thresholded to a 16-bit mask that goes to the strip's bit plane T in LDS.
//   phase 2-4  dilate, erode, bytes + plane + row masks: k_binary's generic path.
//
// A workgroup owns a strip of `sr` rows of one frame (32; 8 when a launch has fewer strips than half the CUs: one camera frame).
// The close needs 2 halo rows per side, the demosaic one more: the third is the window's extra row and is only read.  Border rule:
// D clamps the SITE (x, y) to [1, w-2] x [1, h-2]; the row window is centred on the clamped row and the edge columns copy the mask
// bit of their interior neighbour -- a raw-buffer load past the edge returns 0, which is not what D says.
#include <algorithm>

#include "rmcv_internal.h"
#include "device_bayer.h"

namespace rmcv {

namespace {

constexpr int BSR = STRIP_ROWS;             // strip rows of a workgroup (at most)
constexpr uint32_t B_OOB = 0xFFFFFFF0u;     // voffset of a lane that loads nothing (extents are kept below 4 GiB - 4 KiB)
constexpr int B_RSRC3 = 0x00020000;         // raw buffer descriptor word 3, gfx9 family

typedef uint32_t u32x4b __attribute__((ext_vector_type(4)));

struct Row { // 16 mosaic bytes of a lane (4 dwords) + the bytes left and right of them
    uint32_t d[4];
    int l, r;
};

__device__ __forceinline__ int rbyte(const Row& R, int i)
{
    if (i < 0) return R.l;
    if (i > 15) return R.r;
    return (int)((R.d[i >> 2] >> (8 * (i & 3))) & 0xFFu);
}

// 16 pixels of the row window (a, b, c) = mosaic rows (y-1, y, y+1), pixel 0 at an even column: bit i = (ch CA - ch CB >= lb) of D.
// RX: the R column parity, PY: 1 if row y is a B row.  All site kinds are compile-time here.
template <int CA, int CB, int RX, int PY>
__device__ __forceinline__ uint32_t bayer_mask16(const Row& a, const Row& b, const Row& c, int lb)
{
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int px = (i & 1) ^ RX;
        const int own = rbyte(b, i), hs = rbyte(b, i - 1) + rbyte(b, i + 1), vs = rbyte(a, i) + rbyte(c, i);
        const int ds = rbyte(a, i - 1) + rbyte(a, i + 1) + rbyte(c, i - 1) + rbyte(c, i + 1);
        int v[3]; // B, G, R
        if (!px && !PY) { v[2] = own; v[1] = (hs + vs + 2) >> 2; v[0] = (ds + 2) >> 2; }
        else if (px && PY) { v[0] = own; v[1] = (hs + vs + 2) >> 2; v[2] = (ds + 2) >> 2; }
        else if (!PY) { v[1] = own; v[2] = (hs + 1) >> 1; v[0] = (vs + 1) >> 1; }
        else { v[1] = own; v[0] = (hs + 1) >> 1; v[2] = (vs + 1) >> 1; }
        m |= (uint32_t)(v[CA] - v[CB] >= lb) << i;
    }
    return m;
}

} // namespace

// VEC: w a multiple of 16 (a lane's 16 bytes are all inside the row or all beyond it), rows and frames 16-byte aligned, every extent
// below 4 GiB: unconditional raw-buffer loads (dwordx4 per lane); otherwise bounds-checked byte loads (any w and stride, e.g. 5-pixel
// rows).
// Register budget as k_binary's (k_binary.hip: at most 80 VGPRs, so that the sparse kernel of the previous batch fits beside it).
//
// LD, the phase-1 loader.  0 and 1 read a plain 8-bit mosaic as delivered (1 = VEC above, 0 = byte-wise).  2 and 4..7 read the sensor's
// own layout (device_bayer.h: 2-byte samples narrowed to their valid window, mirror, flip) and hand phases 1-4 the same Row of the
// ORIENTED mosaic T(r); the launcher passes the R site of T(r) and the layout word in the bits of `ry` above bit 0:
//   flip    the source row is h-1-y: run-time in all of them
//   2       byte-wise, any width, stride and layout (all run-time; with mirror the ragged end of a row sits in the first lane)
//   4 | MIR | S16 << 1   dwordx4 loads under the same alignment rules as 1.  MIR: a lane's 16 oriented pixels are 16 consecutive source
//           samples read backwards -- loaded at the mirrored offset, the dwords swapped and byte-reversed (v_perm_b32).  S16: two
//           dwordx4 per lane and row, each dword shifted by the (wave-uniform) valid bit and the two window bytes of each pair of
//           dwords packed by one v_perm_b32.  The neighbour exchange and the wave-edge loads work in oriented coordinates.
template <int CA, int CB, int LD>
__global__ __launch_bounds__(256, 6) void k_binary_bayer(const uint8_t* __restrict__ frames, int64_t frame_pitch, int stride, int n_frames,
                                                         int w, int h, int ww, int rx, int ry, int lb, int all_pass, int morph,
                                                         uint8_t* __restrict__ binary, uint64_t* __restrict__ bits, int prow,
                                                         int64_t plane_pitch, int strips, int sr, uint32_t* __restrict__ rowmask)
{
    constexpr bool VEC = LD == 1 || LD >= 4, RAW = LD >= 2, MIR = LD >= 4 && (LD & 1), S16 = LD >= 4 && (LD & 2);
    const int lay = RAW ? ry >> 1 : 0; // (RAW only: the layout word; bit 0 of ry is the row parity of the R site everywhere below)
    extern __shared__ uint64_t smem[];
    const int halo = morph; // NONE 0, DILATE 1, CLOSE 2
    uint64_t* T = smem;
    uint64_t* D = smem + (size_t)(BSR + 4) * ww;
    const int tid = threadIdx.x, lane = tid & 63;
    const int L = blockIdx.x;
    const int f = L / strips, strip = L - f * strips;
    const int y0 = strip * sr;
    if (y0 >= h) return; // (uniform: the whole workgroup)
    const int srh = sr + 2 * halo;
    const int wq = ww * 4; // 16-pixel groups per row
    const uint8_t* frame = frames + (int64_t)f * frame_pitch;

    // ---------------- phase 1: demosaic + threshold -> T
    {
        // bands of rows: nb bands side by side (wq * nb <= 256 threads), RB rows each, RB even so that the lanes of a wave that sit in
        // different bands are on rows of the same colour phase (the site kinds stay wave-uniform away from the clamped border rows)
        const int nb = wq >= 256 ? 1 : min(srh, 256 / wq);
        const int RB = (((srh + nb - 1) / nb) + 1) & ~1;
        const int items = nb * wq;
        uint16_t* T16 = reinterpret_cast<uint16_t*>(T);
        const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(frames), 0, VEC ? (int)((int64_t)(n_frames - 1) * frame_pitch + (int64_t)(h - 1) * stride + (S16 ? 2 * w : w)) : 0, B_RSRC3);
        const uint32_t fbase = VEC ? (uint32_t)((int64_t)f * frame_pitch) : 0u;
        for (int it0 = tid - lane; it0 < items; it0 += 256) { // wave-uniform loop: every lane takes part in the exchanges
            const int it = it0 + lane;
            const bool live = it < items;
            const int band = live ? it / wq : 0, q = live ? it - band * wq : 0;
            const int x0 = q * 16;
            const int rr0 = band * RB;
            // one mosaic row of this lane's 16 pixels + its two neighbours; yrow < 0: nothing (zeros, no traffic)
            auto load_row = [&](int yrow) -> Row {
                Row R;
                if constexpr (RAW && VEC) {
                    const bool ok = yrow >= 0 && live && x0 < w;
                    const uint32_t rowoff = fbase + (uint32_t)((lay & LAY_FLIP) ? h - 1 - yrow : yrow) * (uint32_t)stride;
                    const uint32_t off = ok ? rowoff + (uint32_t)(MIR ? w - 16 - x0 : x0) * (S16 ? 2u : 1u) : B_OOB;
                    if constexpr (S16) {
                        const u32x4b v0 = __builtin_amdgcn_raw_buffer_load_b128(r_in, off, 0, 0);
                        const u32x4b v1 = __builtin_amdgcn_raw_buffer_load_b128(r_in, ok ? off + 16u : B_OOB, 0, 0);
                        const int vb = lay_vbit(lay);
                        const uint32_t t[8] = {v0.x >> vb, v0.y >> vb, v0.z >> vb, v0.w >> vb, v1.x >> vb, v1.y >> vb, v1.z >> vb, v1.w >> vb};
#pragma unroll
                        for (int k = 0; k < 4; k++) // bytes 0 and 2 of a shifted dword are the windows of its two samples
                            R.d[k] = MIR ? __builtin_amdgcn_perm(t[7 - 2 * k], t[6 - 2 * k], 0x00020406u) : __builtin_amdgcn_perm(t[2 * k + 1], t[2 * k], 0x06040200u);
                    } else {
                        const u32x4b v = __builtin_amdgcn_raw_buffer_load_b128(r_in, off, 0, 0);
                        if (MIR) {
                            R.d[0] = __builtin_amdgcn_perm(0u, v.w, 0x00010203u); R.d[1] = __builtin_amdgcn_perm(0u, v.z, 0x00010203u);
                            R.d[2] = __builtin_amdgcn_perm(0u, v.y, 0x00010203u); R.d[3] = __builtin_amdgcn_perm(0u, v.x, 0x00010203u);
                        } else { R.d[0] = v.x; R.d[1] = v.y; R.d[2] = v.z; R.d[3] = v.w; }
                    }
                    // the neighbours, in oriented coordinates as below: from the lanes beside, the wave's edge lanes load one sample
                    const int from_l = __shfl((int)(R.d[3] >> 24), lane - 1 < 0 ? 0 : lane - 1);
                    const int from_r = __shfl((int)(R.d[0] & 0xFFu), lane + 1 > 63 ? 63 : lane + 1);
                    int xc = -1; // the oriented column an edge lane loads (columns -1 and >= w: nothing)
                    if (ok && lane == 0 && x0 > 0) xc = x0 - 1;
                    if (ok && lane == 63 && x0 + 16 < w) xc = x0 + 16;
                    const uint32_t eo = xc >= 0 ? rowoff + (uint32_t)(MIR ? w - 1 - xc : xc) * (S16 ? 2u : 1u) : B_OOB;
                    int edge;
                    if constexpr (S16) edge = ((int)__builtin_amdgcn_raw_buffer_load_b16(r_in, eo, 0, 0) >> lay_vbit(lay)) & 0xFF;
                    else edge = (int)__builtin_amdgcn_raw_buffer_load_b8(r_in, eo, 0, 0);
                    R.l = lane == 0 ? edge : from_l;
                    R.r = lane == 63 ? edge : from_r;
                } else if constexpr (RAW) {
                    const bool ok = yrow >= 0 && live;
                    const uint8_t* p = frame + (int64_t)(yrow < 0 ? 0 : (lay & LAY_FLIP) ? h - 1 - yrow : yrow) * stride;
                    // the sample of oriented column x: source column x, or w-1-x mirrored; sgn / xm and the shifts are wave-uniform
                    const int vb = lay_vbit(lay), sh = (lay & LAY_S16) ? 1 : 0, sgn = (lay & LAY_MIRROR) ? -1 : 1, xm = (lay & LAY_MIRROR) ? w - 1 : 0;
                    auto px = [&](int x) -> uint32_t {
                        const uint8_t* q = p + ((xm + sgn * x) << sh);
                        return sh ? (uint32_t)(*reinterpret_cast<const uint16_t*>(q) >> vb) & 0xFFu : (uint32_t)*q;
                    };
                    // (rolled, the dwords rotating through: this loader is the fallback for odd geometry and has to stay inside the
                    // register budget with three rows live)
                    uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll 1
                    for (int k = 0; k < 4; k++) {
                        uint32_t dw = 0;
#pragma unroll 1
                        for (int j = 0; j < 4; j++) {
                            const int x = x0 + 4 * k + j;
                            if (ok && x < w) dw |= px(x) << (8 * j);
                        }
                        d0 = d1; d1 = d2; d2 = d3; d3 = dw;
                    }
                    R.d[0] = d0; R.d[1] = d1; R.d[2] = d2; R.d[3] = d3;
                    R.l = (ok && x0 > 0 && x0 - 1 < w) ? (int)px(x0 - 1) : 0;
                    R.r = (ok && x0 + 16 < w) ? (int)px(x0 + 16) : 0;
                } else if (VEC) {
                    const uint32_t off = (yrow >= 0 && live) ? fbase + (uint32_t)yrow * (uint32_t)stride + (uint32_t)x0 : B_OOB;
                    const u32x4b v = __builtin_amdgcn_raw_buffer_load_b128(r_in, off, 0, 0);
                    R.d[0] = v.x; R.d[1] = v.y; R.d[2] = v.z; R.d[3] = v.w;
                    // neighbours from the lanes beside (pixel -1 = byte 15 of lane - 1, pixel 16 = byte 0 of lane + 1) ...
                    const int from_l = __shfl((int)(R.d[3] >> 24), lane - 1 < 0 ? 0 : lane - 1);
                    const int from_r = __shfl((int)(R.d[0] & 0xFFu), lane + 1 > 63 ? 63 : lane + 1);
                    // ... except at the wave's edges: lane 0 loads its left byte, lane 63 its right one (one instruction, the others
                    // load nothing).  Columns -1 and >= w are never used (the edge columns take their neighbour's bit).
                    uint32_t eo = B_OOB;
                    if (yrow >= 0 && live && lane == 0 && x0 > 0) eo = fbase + (uint32_t)yrow * (uint32_t)stride + (uint32_t)(x0 - 1);
                    if (yrow >= 0 && live && lane == 63) eo = fbase + (uint32_t)yrow * (uint32_t)stride + (uint32_t)(x0 + 16);
                    const int edge = (int)__builtin_amdgcn_raw_buffer_load_b8(r_in, eo, 0, 0);
                    R.l = lane == 0 ? edge : from_l;
                    R.r = lane == 63 ? edge : from_r;
                } else {
                    const uint8_t* p = frame + (int64_t)(yrow < 0 ? 0 : yrow) * stride;
                    const bool ok = yrow >= 0 && live;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        uint32_t dw = 0;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int x = x0 + 4 * k + j;
                            if (ok && x < w) dw |= (uint32_t)p[x] << (8 * j);
                        }
                        R.d[k] = dw;
                    }
                    R.l = (ok && x0 > 0) ? p[x0 - 1] : 0;
                    R.r = (ok && x0 + 16 < w) ? p[x0 + 16] : 0;
                }
                return R;
            };
            // the window: rows (cy - 1, cy, cy + 1) of the mosaic, cy the clamped site row of the last output row computed
            const int yb = y0 - halo + rr0; // image row of the band's first row
            const int yfirst = max(yb, 0);
            const int yc_first = min(max(yfirst, 1), h - 2);
            const bool any = live && rr0 < srh && yfirst < h && yfirst < yb + RB; // the band has a row inside the image
            Row a, b = load_row(any ? yc_first - 1 : -1), c = load_row(any ? yc_first : -1);
            a = b;
            int cy = yc_first - 1;
            for (int r = 0; r < RB; r++) {
                const int rr = rr0 + r, y = yb + r;
                const bool in = live && rr < srh && y >= 0 && y < h;
                const int yc = min(max(y, 1), h - 2);
                const bool step = in && yc == cy + 1;
                const Row n = load_row(step ? yc + 1 : -1); // (every lane: the exchanges inside are wave-wide)
                if (step) { a = b; b = c; c = n; cy = yc; }
                uint32_t m;
                if (all_pass) m = 0xFFFFu;
                else {
                    const int py = (yc ^ ry) & 1;
                    if (rx == 0) m = py ? bayer_mask16<CA, CB, 0, 1>(a, b, c, lb) : bayer_mask16<CA, CB, 0, 0>(a, b, c, lb);
                    else m = py ? bayer_mask16<CA, CB, 1, 1>(a, b, c, lb) : bayer_mask16<CA, CB, 1, 0>(a, b, c, lb);
                    // border columns: x = 0 takes the bit of x = 1, x = w - 1 that of x = w - 2 (possibly the left lane's bit 15)
                    if (x0 == 0) m = (m & ~1u) | ((m >> 1) & 1u);
                    const uint32_t left15 = (uint32_t)__shfl((int)m, lane - 1 < 0 ? 0 : lane - 1) >> 15 & 1u;
                    const int xl = w - 1 - x0; // position of the last column in this lane's 16
                    if (xl >= 1 && xl < 16) m = (m & ~(1u << xl)) | (((m >> (xl - 1)) & 1u) << xl);
                    else if (xl == 0) {
                        // the left neighbour pixel w - 2 is bit 15 of lane - 1 -- or of another wave when lane == 0 (recompute it)
                        uint32_t nb15 = left15;
                        if (lane == 0) {
                            int px3[3];
                            if constexpr (RAW) bayer_bgr_raw(frame, stride, w, h, rx, ry & 1, lay, w - 2, y, px3);
                            else bayer_bgr(frame, stride, w, h, rx, ry, w - 2, y, px3);
                            nb15 = (uint32_t)(px3[CA] - px3[CB] >= lb);
                        }
                        m = (m & ~1u) | nb15;
                    }
                }
                if (x0 + 16 > w) m &= x0 < w ? (1u << (w - x0)) - 1u : 0u; // columns >= w
                if (!in) m = 0;                                                                      // rows outside the image
                if (live && rr < srh) T16[rr * wq + q] = (uint16_t)m;
            }
        }
    }
    __syncthreads();

    const uint64_t last_valid = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull; // valid bits of the last word
    uint64_t* R = T; // plane holding the result rows, result row s at R[(s + halo) * ww + k]

    if (morph != RMCV_MORPH_NONE) {
        // ---------------- phase 2: dilate -> D (rows 1 .. srh-2)   (k_binary.hip phase 2)
        const int items = (srh - 2) * ww;
        for (int it = tid; it < items; it += 256) {
            const int rr = 1 + it / ww, k = it - (rr - 1) * ww;
            const int y = y0 - halo + rr;
            const int row = rr * ww;
            uint64_t d;
            if (y < 0 || y >= h) {
                d = ~0ull; // outside the image: never wins the erode
            } else {
                const uint64_t* t0 = T + row - ww;
                const uint64_t* t1 = T + row;
                const uint64_t* t2 = T + row + ww;
                uint64_t cc = t0[k] | t1[k] | t2[k];
                uint64_t l = (k > 0) ? (t0[k - 1] | t1[k - 1] | t2[k - 1]) >> 63 : 0;
                uint64_t r = (k < ww - 1) ? (t0[k + 1] | t1[k + 1] | t2[k + 1]) & 1 : 0;
                d = cc | (cc << 1) | l | (cc >> 1) | (r << 63);
                if (k == ww - 1) {
                    d &= last_valid;
                    if (morph == RMCV_MORPH_CLOSE) d |= ~last_valid; // columns >= w never win the erode
                }
            }
            D[row + k] = d;
        }
        __syncthreads();
        R = D;
        if (morph == RMCV_MORPH_CLOSE) {
            // ---------------- phase 3: erode -> T (rows 2 .. srh-3 = the strip)
            const int items3 = sr * ww;
            for (int it = tid; it < items3; it += 256) {
                const int rr = 2 + it / ww, k = it - (rr - 2) * ww;
                const int row = rr * ww;
                const uint64_t* d0 = D + row - ww;
                const uint64_t* d1 = D + row;
                const uint64_t* d2 = D + row + ww;
                uint64_t cc = d0[k] & d1[k] & d2[k];
                uint64_t l = (k > 0) ? (d0[k - 1] & d1[k - 1] & d2[k - 1]) >> 63 : 1;
                uint64_t r = (k < ww - 1) ? (d0[k + 1] & d1[k + 1] & d2[k + 1]) & 1 : 1;
                uint64_t e = cc & ((cc << 1) | l) & ((cc >> 1) | (r << 63));
                if (k == ww - 1) e &= last_valid;
                T[row + k] = e;
            }
            __syncthreads();
            R = T;
        }
    }

    // ---------------- row masks for the contour stage: bit k = word k of the row is non-zero
    if (ww <= 32 && tid < sr && y0 + tid < h) {
        uint32_t m = 0;
        for (int k = 0; k < ww; k++) m |= (uint32_t)(R[(tid + halo) * ww + k] != 0) << k;
        rowmask[(int64_t)f * h + y0 + tid] = m;
    }
    // ---------------- phase 4: the plane's words, then the byte image (16 pixels per item, one dwordx4 where the row allows it)
    {
        uint64_t* plane = bits + (int64_t)f * plane_pitch;
        const int nw = sr * ww;
        for (int it = tid; it < nw; it += 256) {
            const int s = it / ww, k = it - s * ww, y = y0 + s;
            if (y < h) plane[(int64_t)(y + 1) * prow + 1 + k] = R[(s + halo) * ww + k];
        }
    }
    if (binary) { // RMCV_STAGE_NO_IMAGE: the 0/255 byte image is not wanted
        const uint16_t* R16 = reinterpret_cast<const uint16_t*>(R + halo * ww);
        uint8_t* bin = binary + (int64_t)f * w * h;
        const bool vec_out = ((w & 15) == 0) && (((uintptr_t)binary & 15) == 0);
        const int items = min(sr, h - y0) * wq;
        for (int it = tid; it < items; it += 256) {
            const int s = it / wq, q = it - s * wq, x0 = q * 16;
            if (x0 >= w) continue;
            const uint32_t m = R16[s * wq + q];
            uint8_t* dst = bin + (int64_t)(y0 + s) * w + x0;
            if (vec_out) { // (written once, read by nobody here: non-temporal)
                const u32x4b o = {(((m & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu, ((((m >> 4) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu,
                                  ((((m >> 8) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu, ((((m >> 12) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu};
                __builtin_nontemporal_store(o, reinterpret_cast<u32x4b*>(dst));
            } else {
                const int n = min(16, w - x0);
                for (int p = 0; p < n; p++) dst[p] = ((m >> p) & 1u) ? 255 : 0;
            }
        }
    }
}

// the stage-wise demosaic (rmcv_demosaic): D(m) as B, G, R bytes, one thread per pixel
__global__ __launch_bounds__(256) void k_demosaic(const uint8_t* __restrict__ raw, int stride, int w, int h, int rx, int ry,
                                                  uint8_t* __restrict__ out, int out_stride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    int v[3];
    bayer_bgr(raw, stride, w, h, rx, ry, x, y, v);
    uint8_t* o = out + (int64_t)y * out_stride + 3 * x;
    o[0] = (uint8_t)v[0];
    o[1] = (uint8_t)v[1];
    o[2] = (uint8_t)v[2];
}

// the same of a delivered buffer: D(T(r)) (rmcv_demosaic_raw)
__global__ __launch_bounds__(256) void k_demosaic_raw(const uint8_t* __restrict__ raw, int stride, int w, int h, int rx, int ry, int lay,
                                                      uint8_t* __restrict__ out, int out_stride)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    int v[3];
    bayer_bgr_raw(raw, stride, w, h, rx, ry, lay, x, y, v);
    uint8_t* o = out + (int64_t)y * out_stride + 3 * x;
    o[0] = (uint8_t)v[0];
    o[1] = (uint8_t)v[1];
    o[2] = (uint8_t)v[2];
}

hipError_t launch_demosaic(const uint8_t* d_raw, int stride, int w, int h, int pattern, int lay, uint8_t* d_out, int out_stride, hipStream_t s)
{
    if (lay)
        return launch(k_demosaic_raw, dim3((w + 255) / 256, h), dim3(256), 0, s, d_raw, stride, w, h, raw_rx(pattern, lay, w), raw_ry(pattern, lay, h), lay,
                      d_out, out_stride);
    return launch(k_demosaic, dim3((w + 255) / 256, h), dim3(256), 0, s, d_raw, stride, w, h, bayer_rx(pattern), bayer_ry(pattern), d_out, out_stride);
}

template <int CA, int CB>
static hipError_t launch_bayer_t(const Geom& g, const Bufs& b, int lb, int all_pass, int morph, bool image, hipStream_t s)
{
    // one camera frame (fewer strips than half the CUs): 8-row strips, four times the workgroups
    const int n_cu = g.n_cu > 0 ? g.n_cu : 256;
    const int sr = (int64_t)g.n_frames * ((g.h + BSR - 1) / BSR) * 2 <= n_cu ? BSR / 4 : BSR;
    const int strips = (g.h + sr - 1) / sr;
    const size_t planes = (size_t)2 * (BSR + 4) * g.ww * sizeof(uint64_t);
    const bool aligned = (g.w % 16 == 0) && (g.stride % 16 == 0) && (g.frame_pitch % 16 == 0) && ((uintptr_t)b.frames % 16 == 0);
    // (32-bit buffer offsets: a batch beyond 4 GiB of mosaic is a few launches in a row)
    const int64_t lim = 0xFFFFF000ll;
    const int64_t per_frame = std::max<int64_t>(g.frame_pitch, 1);
    const int chunk = aligned ? (int)std::min<int64_t>(g.n_frames, std::max<int64_t>(1, (lim - 1) / per_frame)) : g.n_frames;
    const bool vec = aligned && (int64_t)chunk * per_frame < lim;
    // the loader (k_binary_bayer's LD): a plain 8-bit mosaic keeps 0 / 1; the sensor's own layout takes 2 or 4 | mirror | 16-bit << 1
    const int lay = raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient);
    const int ld = !lay ? (vec ? 1 : 0) : !vec ? 2 : 4 | ((lay & LAY_MIRROR) ? 1 : 0) | ((lay & LAY_S16) ? 2 : 0);
    static size_t lds_set[MAX_DEVICES][8] = {};
    if (planes > 60 * 1024 && planes > lds_set[g.device][ld]) {
        const void* const fns[8] = {reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 0>), reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 1>),
                                    reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 2>), nullptr,
                                    reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 4>), reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 5>),
                                    reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 6>), reinterpret_cast<const void*>(k_binary_bayer<CA, CB, 7>)};
        const hipError_t ea = hipFuncSetAttribute(fns[ld], hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes);
        if (ea != hipSuccess) return ea;
        lds_set[g.device][ld] = planes;
    }
    // the R site of what phases 1-4 see: the mosaic itself, or T(r) with the layout word riding above the row parity
    const int rx = lay ? raw_rx(g.input_format, lay, g.w) : bayer_rx(g.input_format);
    const int ry = lay ? raw_ry(g.input_format, lay, g.h) | (lay << 1) : bayer_ry(g.input_format);
    for (int f0 = 0; f0 < g.n_frames; f0 += chunk) {
        const int nf = std::min(chunk, g.n_frames - f0);
        const uint8_t* frames = b.frames + (int64_t)f0 * g.frame_pitch;
        uint8_t* binary = image ? b.binary + (int64_t)f0 * g.w * g.h : nullptr;
        uint64_t* bits = b.bits + (int64_t)f0 * g.plane_pitch;
        uint32_t* rowmask = b.rowmask + (int64_t)f0 * g.h;
#define RMCV_KB_LAUNCH(V)                                                                                                                  \
    launch(k_binary_bayer<CA, CB, V>, dim3(nf * strips), dim3(256), planes, s, frames, g.frame_pitch, g.stride, nf, g.w, g.h, g.ww, rx, ry, \
           lb, all_pass, morph, binary, bits, g.prow, g.plane_pitch, strips, sr, rowmask)
        hipError_t e;
        switch (ld) {
        case 0: e = RMCV_KB_LAUNCH(0); break;
        case 1: e = RMCV_KB_LAUNCH(1); break;
        case 2: e = RMCV_KB_LAUNCH(2); break;
        case 4: e = RMCV_KB_LAUNCH(4); break;
        case 5: e = RMCV_KB_LAUNCH(5); break;
        case 6: e = RMCV_KB_LAUNCH(6); break;
        default: e = RMCV_KB_LAUNCH(7); break;
        }
#undef RMCV_KB_LAUNCH
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_binary_bayer(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, hipStream_t s)
{
    // channel pair and effective bound as every pixel kernel's (pixel_plan.h: frame_key_eff)
    const FrameKey k = frame_key_eff(camp, lower_bound);
    return with_channel_pair(k, [&](auto ca, auto cb) { return launch_bayer_t<ca, cb>(g, b, k.lb, k.all_pass, morph, image, s); });
}

} // namespace rmcv
