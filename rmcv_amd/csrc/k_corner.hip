// k_corner.hip -- sub-pixel corner refinement: cornerSubPix of executable/calibration/hand_eye.cpp:121 for the corners of n
// chosen frames of a batch, refined in place in the caller's device table.  The arithmetic is device_corner.h, the same source
// rmcv_corner_subpix_host runs on the CPU; what is decided outside the kernel is corner_plan.h.
//
// Mapping (gfx950, wave64): one wavefront per (chosen frame, corner), four per 256-thread workgroup; the workgroup copies the mask into LDS
// once.  Per iteration a wavefront stages the (win_w + 3) x (win_h + 3) gray bytes around its iterate in LDS -- each a clamped read of
// SRC(f) through the caches: the frame's bytes, its table, or the demosaic of its mosaic; no gray image is ever materialised -- builds the
// (win_w + 2) x (win_h + 2) float patch in LDS from them, then every lane walks the window elements k = lane, lane + 64, .. into five double
// partial sums, which a butterfly of __shfl_xor (32, 16, .. 1) turns into the same five sums in every lane.  Every lane therefore takes
// the same step and leaves the loop in the same pass: nothing in it diverges.  Lane 0 stores the corner and its status word.
// Ordinary vector loads and stores; no scratch; static LDS 25 892 B (corner_plan.h).
#include "rmcv_internal.h"
#include "device_corner.h"

namespace rmcv {

// LDS written by some lanes of a wavefront is read by others behind this (device_hull.h's idiom)
__device__ __forceinline__ void corner_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int SRC>
__global__ __launch_bounds__(256) void k_corner_subpix(CornerJob j)
{
    __shared__ float s_mask[CORNER_MASK_MAX];
    __shared__ float s_patch[CORNER_WAVES][CORNER_PATCH_MAX];
    __shared__ uint32_t s_gray[CORNER_WAVES][CORNER_GRAY_MAX / 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int win_w = 2 * j.win_x + 1, win_h = 2 * j.win_y + 1, nel = win_w * win_h;
    const int gw = win_w + 3, gh = win_h + 3, pw = win_w + 2, ph = win_h + 2;
    for (int i = tid; i < nel; i += 256) s_mask[i] = j.mask[i];
    __syncthreads(); // (the only workgroup barrier: wavefronts leave behind it)
    const int64_t item = (int64_t)blockIdx.x * CORNER_WAVES + wv;
    if (item >= (int64_t)j.n * j.per_frame) return;
    const int k = (int)(item / j.per_frame), q = (int)(item - (int64_t)k * j.per_frame);
    int cnt = j.per_frame;
    if (j.counts) {
        cnt = j.counts[k];
        cnt = cnt < 0 ? 0 : (cnt > j.per_frame ? j.per_frame : cnt);
    }
    if (q >= cnt) return;
    const FramePixels S = frame_pixels<SRC>(j.src, j.frames ? j.frames[k] : k);
    uint8_t* g8 = reinterpret_cast<uint8_t*>(s_gray[wv]);
    float* pt = s_patch[wv];
    auto sums = [&](float cx, float cy) {
        const CornerPatch P = corner_patch(cx, cy, win_w, win_h, j.src.w, j.src.h);
        corner_wave_sync(); // (the pass before has read its patch)
        for (int i = lane; i < gw * gh; i += 64) {
            const int r = i / gw, c = i - r * gw;
            g8[i] = (uint8_t)corner_gray_at<SRC>(S, P.ix + c, P.iy + r);
        }
        corner_wave_sync();
        for (int i = lane; i < pw * ph; i += 64) {
            const int r = i / pw, c = i - r * pw;
            const uint8_t* g = g8 + r * gw + c;
            pt[i] = corner_patch_px(g[0], g[1], g[gw], g[gw + 1], P);
        }
        corner_wave_sync();
        CornerSums acc = corner_zero_sums();
        for (int e = lane; e < nel; e += 64) {
            const int i = e / win_w;
            corner_element(pt, pw, i, e - i * win_w, s_mask[e], j.win_x, j.win_y, acc);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            CornerSums o;
            o.a = __shfl_xor(acc.a, s);
            o.b = __shfl_xor(acc.b, s);
            o.c = __shfl_xor(acc.c, s);
            o.bb1 = __shfl_xor(acc.bb1, s);
            o.bb2 = __shfl_xor(acc.bb2, s);
            acc = corner_add(acc, o);
        }
        return acc;
    };
    float* cp = j.corners + 2 * item;
    float x = cp[0], y = cp[1];
    int32_t st = 0;
    corner_refine(x, y, st, j.src.w, j.src.h, j.win_x, j.win_y, j.max_iters, j.eps, sums);
    if (lane == 0) {
        cp[0] = x;
        cp[1] = y;
        if (j.status) j.status[item] = st;
    }
}

hipError_t launch_corner(const CornerJob& j, hipStream_t s)
{
    const dim3 grid((unsigned)corner_workgroups(j.n, j.per_frame)), block(64 * CORNER_WAVES);
    return with_source_kind(j.src.kind, [&](auto K) { return launch(k_corner_subpix<decltype(K)::value>, grid, block, 0, s, j); });
}

} // namespace rmcv

// ---- the host-side entry points (no context) ----
extern "C" {

int rmcv_corner_mask(int win_x, int win_y, int zero_x, int zero_y, float* mask_out)
{
    if (!mask_out || rmcv::corner_params_refusal(win_x, win_y, zero_x, zero_y, 1, 0.0)) return RMCV_ERR_BAD_ARG;
    rmcv::corner_mask(win_x, win_y, zero_x, zero_y, mask_out);
    return RMCV_OK;
}

int rmcv_gray_host(const uint8_t* bgr, int w, int h, int stride, uint8_t* gray_out, int gray_stride)
{
    if (!bgr || !gray_out || w < 1 || h < 1 || stride < 3 * (int64_t)w || gray_stride < w) return RMCV_ERR_BAD_ARG;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint8_t* q = bgr + (int64_t)y * stride + 3 * (int64_t)x;
            gray_out[(int64_t)y * gray_stride + x] = (uint8_t)rmcv::corner_gray(q[0], q[1], q[2]);
        }
    return RMCV_OK;
}

int rmcv_corner_subpix_host(const uint8_t* bgr, int w, int h, int stride, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y,
                            int max_iters, double eps, int32_t* status_out)
{
    if (rmcv::corner_image_refusal(bgr, corners, w, h, stride, n) || rmcv::corner_params_refusal(win_x, win_y, zero_x, zero_y, max_iters, eps)) return RMCV_ERR_BAD_ARG;
    rmcv::corner_subpix_host(bgr, w, h, stride, corners, n, win_x, win_y, zero_x, zero_y, max_iters, eps, status_out);
    return RMCV_OK;
}

} // extern "C"
