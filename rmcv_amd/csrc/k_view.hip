// k_view.hip -- the operator's debug view: for n chosen frames of a batch, what executable/main.cpp:200-207 builds from
// `binary` and :90-100 shows -- GRAY2BGR, rm::debug::draw_lightblobs, rm::debug::draw_armours (src/debug.cpp:43-93; no text), resized to
// vw x vh -- written into the caller's device memory from the frame's bit plane and its result tables.  The arithmetic is device_view.h,
// the same source rmcv_debug_view_host runs on the CPU.
//
// Mapping (gfx950, wave64), two launches:
//   k_view_overlay   one 256-thread workgroup per view.  Zeroes the view's two colour planes (G: the pixel is green or yellow, R: red or
//                    yellow; the padded word layout of Bufs::bits), then walks the frame's segments, one segment per lane, each pixel an
//                    atomic OR into a plane word.  Yellow (negatives, armours) is drawn last by the reference and is the OR of both
//                    planes, so it needs no order.  Positive blobs of ONE colour (every detector path but the legacy matcher's per-blob
//                    vote) need none either; where a frame's blobs differ in colour they are drawn blob by blob behind workgroup
//                    barriers, each setting its plane and clearing the other, which is the reference's overwrite.
//   k_view_resize    one workgroup per 64 x 16 tile of a view.  The tile's source rows of the three planes are combined into three
//                    channel planes (B, G, R: a set bit is 255) in LDS -- at most 1024 words a channel; a tile whose source span is
//                    larger (a view below about a seventh of the frame) reads the planes through the caches instead.  The tile's 64 + 16 taps
//                    are computed once (LDS); a lane computes four pixels of its column, the pixels go to an LDS tile, and the tile is stored as whole
//                    dwords where the caller's layout is 4-byte aligned, bytes at row tails and otherwise.  It reads 3 bits and writes
//                    3 bytes per output pixel, but is bound by its arithmetic (0.6 TB/s written).  Bufs::binary is never read
//                    (RMCV_STAGE_NO_IMAGE).
// Ordinary vector loads, stores and atomics; no scratch (nothing is indexed dynamically in registers).
#include "rmcv_internal.h"
#include "device_view.h"

namespace rmcv {

static constexpr int VT_X = 64, VT_Y = 16;    // output pixels of a tile
static constexpr int VT_WORDS = 1024;         // plane words per channel a tile stages in LDS

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct PutPlanes {
    uint64_t *pa, *pb;
    int prow, w, h, set, clr; // bit 0: plane G, bit 1: plane R
    __device__ void operator()(int x, int y) const
    {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return; // (the clip keeps every pixel inside: a guard, never taken)
        const int64_t idx = (int64_t)(y + 1) * prow + (x >> 6) + 1;
        const unsigned long long m = 1ull << (x & 63);
        if (set & 1) atomicOr((unsigned long long*)pa + idx, m);
        if (set & 2) atomicOr((unsigned long long*)pb + idx, m);
        if (clr & 1) atomicAnd((unsigned long long*)pa + idx, ~m);
        if (clr & 2) atomicAnd((unsigned long long*)pb + idx, ~m);
    }
};

__global__ __launch_bounds__(256) void k_view_overlay(ViewJob j)
{
    const int v = blockIdx.x, tid = threadIdx.x;
    const int f = j.frames ? j.frames[v] : v;
    const ViewLists& L = j.lists;
    uint64_t* pa = j.overlay + (int64_t)v * 2 * j.plane_pitch;
    uint64_t* pb = pa + j.plane_pitch;
    for (int64_t i = tid; i < 2 * j.plane_pitch; i += 256) pa[i] = 0;
    __syncthreads();

    PutPlanes put{pa, pb, j.prow, j.w, j.h, 0, 0};
    // ---- draw_lightblobs, the positives (debug.cpp:77-89): closed 4-gons, edges j -> j + 1, last -> 0
    const int nb = (j.flags & RMCV_VIEW_BLOBS) ? clampi(L.n_blobs[f], 0, L.max_blobs) : 0;
    const rmcv_lightblob* blobs = L.blobs + (int64_t)f * L.max_blobs;
    if (nb > 0) {
        const int first = view_blob_colour(blobs[0].target);
        int differs = 0;
        for (int i = tid; i < nb; i += 256) differs |= view_blob_colour(blobs[i].target) != first;
        if (!__syncthreads_or(differs)) {
            put.set = first == VIEW_GREEN ? 1 : 2;
            for (int e = tid; e < nb * 4; e += 256) {
                const float* vx = &blobs[e >> 2].vertices[0][0];
                view_edge_f(j.w, j.h, vx + 2 * (e & 3), vx + 2 * ((e + 1) & 3), put);
            }
        } else { // colours differ: the reference's order, one blob at a time
            for (int i = 0; i < nb; i++) {
                if (tid < 4) {
                    put.set = view_blob_colour(blobs[i].target) == VIEW_GREEN ? 1 : 2;
                    put.clr = 3 - put.set;
                    const float* vx = &blobs[i].vertices[0][0];
                    view_edge_f(j.w, j.h, vx + 2 * tid, vx + 2 * ((tid + 1) & 3), put);
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
    put.set = 3;
    put.clr = 0;
    // ---- draw_lightblobs, the negatives (:91-92): every contour closed through all its points
    if (j.flags & RMCV_VIEW_NEGATIVES) {
        const int nn = clampi(L.n_neg[f], 0, L.max_contours);
        const int nc = L.csr ? nn : clampi(L.n_contours[f], 0, L.max_contours);
        const rmcv_point* pts = L.points + (int64_t)f * L.max_points;
        for (int i = 0; i < nn; i++) {
            int start, len;
            if (L.csr) {
                start = L.neg_offs[i];
                len = L.neg_offs[i + 1] - start;
            } else { // the negative list holds findContours indices; the tables are in discovery order (the reverse)
                const int k = nc - 1 - L.neg_idx[(int64_t)f * L.max_contours + i];
                if (k < 0 || k >= nc) continue;
                start = L.cont_start[(int64_t)f * L.max_contours + k];
                len = L.cont_len[(int64_t)f * L.max_contours + k];
            }
            if (start < 0 || len <= 0 || start > L.max_points - len) continue;
            for (int e = tid; e < len; e += 256) view_edge_i(j.w, j.h, pts[start + e], pts[start + (e + 1 == len ? 0 : e + 1)], put);
        }
    }
    // ---- draw_armours (:43-70): per armour `vertices`, then `icon`
    if (j.flags & RMCV_VIEW_ARMOURS) {
        const int na = clampi(L.n_armours[f], 0, L.max_armours);
        const rmcv_armour* arm = L.armours + (int64_t)f * L.max_armours;
        for (int e = tid; e < na * 8; e += 256) {
            const rmcv_armour& a = arm[e >> 3];
            const float* vx = (e & 4) ? &a.icon[0][0] : &a.vertices[0][0];
            view_edge_f(j.w, j.h, vx + 2 * (e & 3), vx + 2 * ((e + 1) & 3), put);
        }
    }
}

// the B, G, R channel words of plane word `idx`: the binary where nothing is drawn, the colour planes where something is
__device__ inline void view_channels(const uint64_t* bits, const uint64_t* pa, const uint64_t* pb, int64_t idx, uint64_t ch[3])
{
    const uint64_t a = pa[idx], b = pb[idx], base = bits[idx] & ~(a | b);
    ch[0] = base;
    ch[1] = base | a;
    ch[2] = base | b;
}

__global__ __launch_bounds__(256) void k_view_resize(ViewJob j)
{
    __shared__ uint64_t s_ch[3][VT_WORDS];
    __shared__ uint32_t s_out[VT_Y * VT_X * 3 / 4];
    const int v = blockIdx.z, tid = threadIdx.x;
    const int f = j.frames ? j.frames[v] : v;
    const uint64_t* bits = j.bits + (int64_t)f * j.plane_pitch;
    const uint64_t* pa = j.overlay + (int64_t)v * 2 * j.plane_pitch;
    const uint64_t* pb = pa + j.plane_pitch;
    const int mode = view_resize_mode(j.w, j.h, j.vw, j.vh);
    const int x0 = blockIdx.x * VT_X, y0 = blockIdx.y * VT_Y;
    const int nx = j.vw - x0 < VT_X ? j.vw - x0 : VT_X, ny = j.vh - y0 < VT_Y ? j.vh - y0 : VT_Y;
    // the tile's taps, once: a column's by lanes 0 .. 63, a row's by the next 16 (the double division behind every tap costs as much as a pixel)
    __shared__ view_tap s_tx[VT_X], s_ty[VT_Y];
    if (tid < VT_X) {
        if (tid < nx) s_tx[tid] = view_tap_x(mode, x0 + tid, j.w, j.vw);
    } else if (tid < VT_X + VT_Y) {
        if (tid - VT_X < ny) s_ty[tid - VT_X] = view_tap_y(mode, y0 + tid - VT_X, j.h, j.vh);
    }
    __syncthreads();
    // the tile's source span (taps are monotone in the output coordinate)
    const int r0 = s_ty[0].s0, r1 = s_ty[ny - 1].s1;
    const int k0 = s_tx[0].s0 >> 6, k1 = s_tx[nx - 1].s1 >> 6;
    const int nr = r1 - r0 + 1, nw = k1 - k0 + 1;
    const bool staged = (int64_t)nr * nw <= VT_WORDS;
    if (staged) {
        for (int i = tid; i < nr * nw; i += 256) {
            const int r = i / nw, k = i - r * nw;
            uint64_t ch[3];
            view_channels(bits, pa, pb, (int64_t)(r0 + r + 1) * j.prow + (k0 + k + 1), ch);
            s_ch[0][i] = ch[0];
            s_ch[1][i] = ch[1];
            s_ch[2][i] = ch[2];
        }
    }
    __syncthreads();
    auto fetch = [&](int y, int k, uint64_t ch[3]) {
        if (staged) {
            const int i = (y - r0) * nw + (k - k0);
            ch[0] = s_ch[0][i];
            ch[1] = s_ch[1][i];
            ch[2] = s_ch[2][i];
        } else view_channels(bits, pa, pb, (int64_t)(y + 1) * j.prow + (k + 1), ch);
    };
    const int col = tid & 63;
    if (col < nx) {
        const view_tap tx = s_tx[col];
        const int ka = tx.s0 >> 6, kb = tx.s1 >> 6, ba = tx.s0 & 63, bb = tx.s1 & 63;
        uint8_t* o8 = reinterpret_cast<uint8_t*>(s_out);
        for (int row = tid >> 6; row < ny; row += 4) {
            const view_tap ty = s_ty[row];
            uint64_t t0a[3], t0b[3], t1a[3], t1b[3];
            fetch(ty.s0, ka, t0a);
            fetch(ty.s1, ka, t1a);
            if (kb != ka) { // the right tap is in the next word: one column in 64
                fetch(ty.s0, kb, t0b);
                fetch(ty.s1, kb, t1b);
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) { t0b[c] = t0a[c]; t1b[c] = t1a[c]; }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int p00 = 255 * (int)((t0a[c] >> ba) & 1), p01 = 255 * (int)((t0b[c] >> bb) & 1);
                const int p10 = 255 * (int)((t1a[c] >> ba) & 1), p11 = 255 * (int)((t1b[c] >> bb) & 1);
                o8[(row * VT_X + col) * 3 + c] = (uint8_t)view_mix(mode, p00, p01, p10, p11, tx, ty);
            }
        }
    }
    __syncthreads();
    // the tile leaves as dwords where the caller's layout allows it (a tile starts at byte 192 * blockIdx.x of its rows)
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

hipError_t launch_view(const ViewJob& j, hipStream_t s)
{
    hipError_t e = launch(k_view_overlay, dim3(j.n), dim3(256), 0, s, j);
    if (e != hipSuccess) return e;
    return launch(k_view_resize, dim3((j.vw + VT_X - 1) / VT_X, (j.vh + VT_Y - 1) / VT_Y, j.n), dim3(256), 0, s, j);
}

} // namespace rmcv

extern "C" int rmcv_debug_view_host(const uint8_t* binary, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs,
                                    const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours,
                                    int flags, int vw, int vh, uint8_t* out, int out_stride)
{
    if (!binary || !out) return RMCV_ERR_BAD_ARG;
    if (view_check_lists(w, h, stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out_stride)) return RMCV_ERR_BAD_ARG;
    view_host(binary, w, h, stride, blobs, n_blobs, neg_pts, neg_offs, n_neg, armours, n_armours, flags, vw, vh, out, out_stride);
    return RMCV_OK;
}
