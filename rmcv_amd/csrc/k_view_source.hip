// k_view_source.hip -- the source view: for n chosen frames of a batch, what executable/svm/labeler.cpp:108-111 draws on --
// the camera frame with rm::debug::draw_lightblobs and rm::debug::draw_armours over it -- resized to vw x vh and written into the caller's
// device memory.  Everything is the operator's view (k_view.hip) but the canvas: SRC(f), the BGR image the frame's results
// are defined on (the frame; its demosaic D(T(r)); the frame through its gamma table; its window), instead of GRAY2BGR(binary).  The
// arithmetic is device_view.h, the same source rmcv_source_view_host runs on the CPU; what is decided outside the kernels is
// source_view_plan.h.
//
// Mapping (gfx950, wave64), two launches:
//   k_view_overlay       k_view.hip's, launched as it is: the view's two colour planes (G, R).
//   k_view_source<SRC>   one 256-thread workgroup per 64 x 16 tile of a view, blockIdx.z = view.  The tile's 64 + 16 taps are computed once
//                        (LDS).  A tile whose source span fits the plan's byte budget is STAGED: the span is composited once into LDS as
//                        B, G, R triples -- BGR rows copied as the aligned dwords that hold them (through the frame's table, read from LDS,
//                        where there is one), a plain mosaic demosaiced from an LDS copy of the span's mosaic bytes plus one ring, a mosaic
//                        in a sensor layout through bayer_bgr_raw -- then the overlay colours are written over it, a lane per plane word
//                        (nearly all are zero); every lane then mixes its pixels from LDS.  Any other tile (a thumbnail) GATHERS: each
//                        tap reads its overlay bits and, where they are clear, its source pixel through the caches.  The pixels go to an
//                        LDS tile that is stored as whole dwords where the caller's layout is 4-byte aligned.
// Ordinary vector loads and stores; no scratch (nothing is indexed dynamically in registers); static LDS: 39 168 B at most.
#include <assert.h>

#include "rmcv_internal.h"
#include "device_view.h"

namespace rmcv {

__global__ void k_view_overlay(ViewJob j); // k_view.hip

static constexpr int VT_X = SOURCE_TILE_X, VT_Y = SOURCE_TILE_Y;

__device__ inline int clampsv(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// D's mix at one site (device_bayer.h: bayer_bgr) from the sums of its neighbours; px, py: the site's phase against the R site
__device__ inline void bayer_site(int own, int hs, int vs, int ds, int px, int py, int out[3])
{
    int b, g, r;
    if (!px && !py) { r = own; g = (hs + vs + 2) >> 2; b = (ds + 2) >> 2; }      // R site
    else if (px && py) { b = own; g = (hs + vs + 2) >> 2; r = (ds + 2) >> 2; }   // B site
    else if (!py) { g = own; r = (hs + 1) >> 1; b = (vs + 1) >> 1; }             // G on an R row
    else { g = own; b = (hs + 1) >> 1; r = (vs + 1) >> 1; }                      // G on a B row
    out[0] = b;
    out[1] = g;
    out[2] = r;
}

template <int SRC>
__global__ __launch_bounds__(256) void k_view_source(SourceViewJob sj)
{
    constexpr bool BGRISH = SRC == SOURCE_BGR || SRC == SOURCE_BGR_WIN || SRC == SOURCE_BGR_LUT;
    __shared__ uint32_t s_px[SOURCE_STAGE_BYTES / 4];
    __shared__ uint32_t s_ring[SRC == SOURCE_MOSAIC ? SOURCE_RING_BYTES / 4 : 1];
    __shared__ uint32_t s_lut[SRC == SOURCE_BGR_LUT ? 64 : 1];
    __shared__ uint32_t s_out[VT_Y * VT_X * 3 / 4];
    __shared__ view_tap s_tx[VT_X], s_ty[VT_Y];
    const ViewJob& j = sj.view;
    const FrameSource& fs = sj.src;
    const int v = blockIdx.z, tid = threadIdx.x;
    const FramePixels P = frame_pixels<SRC>(fs, j.frames ? j.frames[v] : v);
    const uint64_t* pa = j.overlay + (int64_t)v * 2 * j.plane_pitch;
    const uint64_t* pb = pa + j.plane_pitch;
    const uint8_t* frame = P.frame;
    const int mode = view_resize_mode(j.w, j.h, j.vw, j.vh);
    const int x0 = blockIdx.x * VT_X, y0 = blockIdx.y * VT_Y;
    const int nx = j.vw - x0 < VT_X ? j.vw - x0 : VT_X, ny = j.vh - y0 < VT_Y ? j.vh - y0 : VT_Y;
    // the tile's taps, once: a column's by lanes 0 .. 63, a row's by the next 16; the frame's table by the wavefront behind them
    if (tid < VT_X) {
        if (tid < nx) s_tx[tid] = view_tap_x(mode, x0 + tid, j.w, j.vw);
    } else if (tid < VT_X + VT_Y) {
        if (tid - VT_X < ny) s_ty[tid - VT_X] = view_tap_y(mode, y0 + tid - VT_X, j.h, j.vh);
    } else if (SRC == SOURCE_BGR_LUT && tid >= 128 && tid < 192) {
        s_lut[tid - 128] = reinterpret_cast<const uint32_t*>(P.lut)[tid - 128];
    }
    __syncthreads();
    const uint8_t* lut8 = reinterpret_cast<const uint8_t*>(s_lut);
    const SourceSpan sp = source_span(s_tx[0].s0, s_tx[nx - 1].s1, s_ty[0].s0, s_ty[ny - 1].s1);
    const bool staged = source_tile_staged(SRC, sp.rows, sp.cols);
    const int pitch = source_span_pitch(sp.cols);
    uint8_t* px8 = reinterpret_cast<uint8_t*>(s_px);
    // where pixel (row r of the span, its first column) lies in LDS: a BGR row keeps the byte phase it has in memory
    const uint8_t* span0 = frame + (int64_t)sp.r0 * fs.stride + 3 * (int64_t)sp.c0;
    auto row_at = [&](int r) { return r * pitch + (BGRISH ? (int)((uintptr_t)(span0 + (int64_t)r * fs.stride) & 3) : 0); };
    if (staged) {
        if constexpr (BGRISH) { // a wavefront per row: the aligned dwords that hold its 3 cols bytes
            const int nb = 3 * sp.cols;
            for (int r = tid >> 6; r < sp.rows; r += 4) {
                const uint8_t* a = span0 + (int64_t)r * fs.stride;
                const int lead = (int)((uintptr_t)a & 3);
                const int ndw = (lead + nb + 3) >> 2;
                for (int i = tid & 63; i < ndw; i += 64) {
                    const uint8_t* q = a - lead + 4 * i;
                    uint32_t d = 0;
                    if (q >= fs.src && q + 4 <= fs.src_end) d = *reinterpret_cast<const uint32_t*>(q);
                    else { // the dword reaches outside what is bound (the first or the last of a buffer): the span's own bytes alone
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (q + k >= a && q + k < a + nb) d |= (uint32_t)q[k] << (8 * k);
                    }
                    if constexpr (SRC == SOURCE_BGR_LUT)
                        d = (uint32_t)lut8[d & 255] | (uint32_t)lut8[(d >> 8) & 255] << 8 | (uint32_t)lut8[(d >> 16) & 255] << 16 | (uint32_t)lut8[d >> 24] << 24;
                    s_px[(r * pitch >> 2) + i] = d;
                }
            }
        } else if constexpr (SRC == SOURCE_MOSAIC) { // the span's mosaic bytes plus one ring, clamped as D clamps; then D from LDS
            const int w = j.w, h = j.h;
            const int mx0 = clampsv(sp.c0, 1, w - 2) - 1, mx1 = clampsv(sp.c0 + sp.cols - 1, 1, w - 2) + 1;
            const int my0 = clampsv(sp.r0, 1, h - 2) - 1, my1 = clampsv(sp.r0 + sp.rows - 1, 1, h - 2) + 1;
            const int mcols = mx1 - mx0 + 1, mrows = my1 - my0 + 1; // <= cols + 2, rows + 2: the clamp moves no two columns apart
            uint8_t* ring = reinterpret_cast<uint8_t*>(s_ring);
            for (int i = tid; i < mrows * mcols; i += 256) {
                const int r = i / mcols, c = i - r * mcols;
                ring[i] = frame[(int64_t)(my0 + r) * fs.stride + mx0 + c];
            }
            __syncthreads();
            for (int i = tid; i < sp.rows * sp.cols; i += 256) {
                const int r = i / sp.cols, c = i - r * sp.cols;
                const int x = clampsv(sp.c0 + c, 1, w - 2), y = clampsv(sp.r0 + r, 1, h - 2);
                const uint8_t* m = ring + (y - my0) * mcols + (x - mx0);
                int o[3];
                bayer_site(m[0], m[-1] + m[1], m[-mcols] + m[mcols], m[-mcols - 1] + m[-mcols + 1] + m[mcols - 1] + m[mcols + 1], (x ^ fs.rx) & 1, (y ^ fs.ry) & 1, o);
                uint8_t* p = px8 + r * pitch + 3 * c;
                p[0] = (uint8_t)o[0];
                p[1] = (uint8_t)o[1];
                p[2] = (uint8_t)o[2];
            }
        } else { // a sensor layout: D(T(r)) per span pixel
            for (int i = tid; i < sp.rows * sp.cols; i += 256) {
                const int r = i / sp.cols, c = i - r * sp.cols;
                int o[3];
                bayer_bgr_raw(frame, fs.stride, j.w, j.h, fs.rx, fs.ry, fs.lay, sp.c0 + c, sp.r0 + r, o);
                uint8_t* p = px8 + r * pitch + 3 * c;
                p[0] = (uint8_t)o[0];
                p[1] = (uint8_t)o[1];
                p[2] = (uint8_t)o[2];
            }
        }
        __syncthreads();
        // the overlay over it: a lane per plane word of the span; a set bit of G | R replaces the pixel (drawContours overwrites)
        const int c1 = sp.c0 + sp.cols - 1, k0 = sp.c0 >> 6, nw = (c1 >> 6) - k0 + 1;
        for (int i = tid; i < sp.rows * nw; i += 256) {
            const int r = i / nw, k = k0 + (i - r * nw);
            const int64_t idx = (int64_t)(sp.r0 + r + 1) * j.prow + (k + 1);
            const uint64_t a = pa[idx], b = pb[idx];
            uint64_t m = a | b;
            if (sp.c0 > 64 * k) m &= ~0ull << (sp.c0 - 64 * k);
            if (c1 < 64 * k + 63) m &= ~0ull >> (64 * k + 63 - c1);
            const int at = row_at(r);
            while (m) {
                const int bit = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                uint8_t* p = px8 + at + 3 * (64 * k + bit - sp.c0);
                p[0] = 0;
                p[1] = (a >> bit & 1) ? 255 : 0;
                p[2] = (b >> bit & 1) ? 255 : 0;
            }
        }
    }
    __syncthreads();
    // one tap of a gathered tile: the overlay's colour where a plane has the bit, the source pixel otherwise
    auto gather = [&](int x, int y, int o[3]) {
        const int64_t idx = (int64_t)(y + 1) * j.prow + (x >> 6) + 1;
        const int a = (int)(pa[idx] >> (x & 63)) & 1, b = (int)(pb[idx] >> (x & 63)) & 1;
        if (a | b) {
            o[0] = 0;
            o[1] = 255 * a;
            o[2] = 255 * b;
        } else if constexpr (BGRISH) {
            const uint8_t* q = frame + (int64_t)y * fs.stride + 3 * (int64_t)x;
#pragma unroll
            for (int c = 0; c < 3; c++) o[c] = SRC == SOURCE_BGR_LUT ? lut8[q[c]] : q[c];
        } else if constexpr (SRC == SOURCE_MOSAIC) {
            bayer_bgr(frame, fs.stride, j.w, j.h, fs.rx, fs.ry, x, y, o);
        } else {
            bayer_bgr_raw(frame, fs.stride, j.w, j.h, fs.rx, fs.ry, fs.lay, x, y, o);
        }
    };
    const int col = tid & 63;
    if (col < nx) {
        const view_tap tx = s_tx[col];
        uint8_t* o8 = reinterpret_cast<uint8_t*>(s_out);
        for (int row = tid >> 6; row < ny; row += 4) {
            const view_tap ty = s_ty[row];
            int p00[3], p01[3], p10[3], p11[3];
            if (staged) {
                const uint8_t* q0 = px8 + row_at(ty.s0 - sp.r0);
                const uint8_t* q1 = px8 + row_at(ty.s1 - sp.r0);
                const int ca = 3 * (tx.s0 - sp.c0), cb = 3 * (tx.s1 - sp.c0);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    p00[c] = q0[ca + c];
                    p01[c] = q0[cb + c];
                    p10[c] = q1[ca + c];
                    p11[c] = q1[cb + c];
                }
            } else {
                gather(tx.s0, ty.s0, p00);
                gather(tx.s1, ty.s0, p01);
                gather(tx.s0, ty.s1, p10);
                gather(tx.s1, ty.s1, p11);
            }
#pragma unroll
            for (int c = 0; c < 3; c++) o8[(row * VT_X + col) * 3 + c] = (uint8_t)view_mix(mode, p00[c], p01[c], p10[c], p11[c], tx, ty);
        }
    }
    __syncthreads();
    // the tile leaves as dwords where the caller's layout allows it (a tile starts at byte 192 * blockIdx.x of its rows): k_view_resize's stores
    uint8_t* out = j.out + (int64_t)v * j.out_pitch + (int64_t)y0 * j.out_stride + 3 * (int64_t)x0;
    const int nbytes = 3 * nx;
    const bool aligned = (((uintptr_t)j.out | (uintptr_t)j.out_stride | (uintptr_t)j.out_pitch) & 3) == 0;
    const int ndw = aligned ? nbytes >> 2 : 0, tail = nbytes - 4 * ndw;
    constexpr int ROW_DW = VT_X * 3 / 4;
    for (int i = tid; i < ny * ndw; i += 256) {
        const int row = i / ndw, d = i - row * ndw;
        *reinterpret_cast<uint32_t*>(out + (int64_t)row * j.out_stride + 4 * d) = s_out[row * ROW_DW + d];
    }
    const uint8_t* o8 = reinterpret_cast<const uint8_t*>(s_out);
    for (int i = tid; i < ny * tail; i += 256) {
        const int row = i / tail, b = 4 * ndw + (i - row * tail);
        out[(int64_t)row * j.out_stride + b] = o8[row * VT_X * 3 + b];
    }
}

hipError_t launch_source_view(const SourceViewJob& sj, hipStream_t s)
{
    const ViewJob& j = sj.view;
    assert(j.w == sj.src.w && j.h == sj.src.h); // (one extent: the overlay's planes and SRC)
    hipError_t e = launch(k_view_overlay, dim3(j.n), dim3(256), 0, s, j);
    if (e != hipSuccess) return e;
    const dim3 grid((j.vw + VT_X - 1) / VT_X, (j.vh + VT_Y - 1) / VT_Y, j.n), block(256);
    return with_source_kind(sj.src.kind, [&](auto K) { return launch(k_view_source<decltype(K)::value>, grid, block, 0, s, sj); });
}

} // namespace rmcv

extern "C" int rmcv_source_view_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
                                     const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh,
                                     uint8_t* out, int out_stride)
{
    if (rmcv::source_image_refusal(bgr, out, w, h, stride)) return RMCV_ERR_BAD_ARG;
    if (view_check_lists(w, h, w, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out_stride)) return RMCV_ERR_BAD_ARG;
    source_view_host(bgr, w, h, stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out, out_stride);
    return RMCV_OK;
}
