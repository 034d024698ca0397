// k_enhance.hip -- rm::AutoEnhance / rm::CalcGamma (the reference's src/imgproc.cpp:37-48, 77-98) as three small kernels:
//
//   k_frame_sums     the exact sums of the B, G and R bytes of every frame bound: cv::mean's numerators.  A pure read of 3 B/px:
//                    HBM-bound, loads shaped like the pixel kernel's (a wave reads 768 contiguous bytes per instruction, lane i the
//                    four pixels 4i .. 4i+3, non-temporal), three v_dot4_u32_u8 per dword triple pick the channels apart.  Integer
//                    sums are order-independent: per-lane 32-bit partial sums, a wave reduction, one 64-bit vector atomic per wave,
//                    strip and channel.
//   k_enhance_table  per frame: sums -> gamma (enhance_math.h: enh_gamma) -> the 256-entry table -> the pixel kernel's threshold
//                    table M for the run's lower bound.  One thread per entry; pow is pinned_math.h's.
//   k_bytemap        dst = table[src] over a staged host image (rmcv_calc_gamma, rmcv_auto_enhance).
//
// No enhanced frame is ever written by a detection run: k_binary_enh and k_classify_enh read the frame through the tables.
#include <algorithm>

#include "enhance_math.h"
#include "rmcv_internal.h"

namespace rmcv {

typedef uint32_t u32x3e __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4e __attribute__((ext_vector_type(4)));
static constexpr int SUM_ROWS = 32;  // rows of one work unit (a strip of one frame)
static constexpr int SUM_UNROLL = 8; // loads a wave has in flight
static constexpr uint32_t SUM_OOB = 0xFFFFFF00u; // voffset of a lane that reads nothing (extents are checked below 4 GiB - 4096)

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t sel, uint32_t acc)
{
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, sel, acc, false);
#else
    return __builtin_amdgcn_sad_u8(a & (sel * 0xFFu), 0u, acc);
#endif
}

// FAST (w % 4 == 0, rows, frames and base 4-byte aligned, the extent below 4 GiB): raw-buffer dwordx3 loads; a lane's 12 bytes are four
// whole pixels, so byte j of them is channel j % 3 wherever the lane stands, and a lane with nothing to read loads from beyond the
// extent (zeros, no traffic).  Rows that are contiguous in memory (stride == 3 w) are read as ONE run per strip.
// FAST == 0: any width, stride and alignment, byte loads.
template <int FAST>
__global__ __launch_bounds__(256) void k_frame_sums(const uint8_t* __restrict__ frames, int64_t frame_pitch, int stride, int n_frames, int w, int h,
                                                    int strips, int n_units, unsigned long long* __restrict__ sums /* [frame][3], zeroed */)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int f = unit / strips, y0 = (unit - f * strips) * SUM_ROWS;
        const int rows = min(SUM_ROWS, h - y0);
        uint32_t sb = 0, sg = 0, sr = 0;
        if (FAST) {
            const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint8_t*>(frames), 0, (int)((int64_t)(n_frames - 1) * frame_pitch + (int64_t)(h - 1) * stride + 3 * w), 0x00020000);
            const bool linear = stride == 3 * w;
            const int n_runs = linear ? 1 : rows;
            const uint32_t run_px = (uint32_t)(linear ? rows * w : w);
            const int nb = (int)((run_px + 255u) >> 8), n_items = n_runs * nb; // n_items <= 32 * 256 for w <= 65536: below 2^16
            const uint32_t r_nb = nb > 1 ? (uint32_t)((0x100000000ull + nb - 1) / nb) : 0u; // it / nb as a multiply (exact below 2^16)
            const uint32_t base = (uint32_t)((int64_t)f * frame_pitch) + (uint32_t)y0 * (uint32_t)stride;
            for (int it0 = wv; it0 < n_items; it0 += 4 * SUM_UNROLL) {
                u32x3e v[SUM_UNROLL];
#pragma unroll
                for (int u = 0; u < SUM_UNROLL; u++) {
                    const int it = it0 + 4 * u; // wave-uniform
                    const int run = linear ? 0 : (r_nb ? (int)__umulhi((uint32_t)it, r_nb) : it), blk = it - run * nb;
                    const uint32_t px = (uint32_t)blk * 256u + (uint32_t)lane * 4u; // w % 4 == 0: a lane's four pixels are all inside the run or all outside
                    const uint32_t vo = (it < n_items && px < run_px) ? base + (uint32_t)run * (uint32_t)stride + px * 3u : SUM_OOB;
                    v[u] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo, 0, 2 /* nt: read once */);
                }
#pragma unroll
                for (int u = 0; u < SUM_UNROLL; u++) {
                    // bytes: x = B0 G0 R0 B1, y = G1 R1 B2 G2, z = R2 B3 G3 R3
                    sb = dot4(v[u].x, 0x01000001u, dot4(v[u].y, 0x00010000u, dot4(v[u].z, 0x00000100u, sb)));
                    sg = dot4(v[u].x, 0x00000100u, dot4(v[u].y, 0x01000001u, dot4(v[u].z, 0x00010000u, sg)));
                    sr = dot4(v[u].x, 0x00010000u, dot4(v[u].y, 0x00000100u, dot4(v[u].z, 0x01000001u, sr)));
                }
            }
        } else {
            const uint8_t* frame = frames + (int64_t)f * frame_pitch + (int64_t)y0 * stride;
            const int n_px = rows * w;
            int y = tid / w, x = tid - y * w;
            const int dy = 256 / w, dx = 256 - dy * w;
            for (int i = tid; i < n_px; i += 256) {
                const uint8_t* p = frame + (int64_t)y * stride + 3 * x;
                sb += p[0];
                sg += p[1];
                sr += p[2];
                y += dy;
                x += dx;
                if (x >= w) { x -= w; y++; }
            }
        }
        // a strip holds at most 32 x w pixels: the 32-bit partial sums cannot wrap (255 x 32 x w < 2^32 up to w = 526 000)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            sb += __shfl_xor(sb, o);
            sg += __shfl_xor(sg, o);
            sr += __shfl_xor(sr, o);
        }
        if (lane < 3) atomicAdd(&sums[(int64_t)f * 3 + lane], (unsigned long long)(lane == 0 ? sb : (lane == 1 ? sg : sr)));
    }
}

// one workgroup per frame, one thread per table entry
__global__ __launch_bounds__(256) void k_enhance_table(const unsigned long long* __restrict__ sums, int64_t n_pixels, float max_gain, float min_gain,
                                                       int lb /* 1 .. 256 */, float* __restrict__ gamma_out, uint8_t* __restrict__ lut_out,
                                                       uint16_t* __restrict__ m_out)
{
    __shared__ uint8_t s_lut[256];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint64_t s3[3] = {sums[(int64_t)f * 3], sums[(int64_t)f * 3 + 1], sums[(int64_t)f * 3 + 2]};
    const float g = enh_gamma(s3, n_pixels, max_gain, min_gain);
    const uint8_t e = enh_lut_entry(t, g);
    s_lut[t] = e;
    __syncthreads();
    lut_out[(int64_t)f * 256 + t] = e;
    m_out[(int64_t)f * 256 + t] = enh_m_entry(s_lut, t, lb);
    if (t == 0) gamma_out[f] = g;
}

__global__ __launch_bounds__(256) void k_gamma_lut(float gamma, uint8_t* __restrict__ lut_out) { lut_out[threadIdx.x] = enh_lut_entry(threadIdx.x, gamma); }

// dst[i] = lut[src[i]] over n16 16-byte vectors (the staged image is padded to whole vectors); dst == src allowed: a thread reads its
// vector before it writes it.  A 256-byte table is 64 dwords, one per LDS bank: the byte gathers never conflict.
__global__ __launch_bounds__(256) void k_bytemap(const u32x4e* src, u32x4e* dst, int64_t n16, const uint8_t* __restrict__ lut)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const u32x4e v = src[i];
        u32x4e o;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t d = v[k];
            o[k] = (uint32_t)s_lut[d & 0xFFu] | ((uint32_t)s_lut[(d >> 8) & 0xFFu] << 8) | ((uint32_t)s_lut[(d >> 16) & 0xFFu] << 16) |
                   ((uint32_t)s_lut[d >> 24] << 24);
        }
        dst[i] = o;
    }
}

hipError_t launch_enhance_tables(const Geom& g, const Bufs& b, int lower_bound, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(b.enh_sums, 0, (size_t)g.n_frames * 3 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const int strips = (g.h + SUM_ROWS - 1) / SUM_ROWS;
    const int n_cu = g.n_cu > 0 ? g.n_cu : 256;
    const bool aligned = (g.w % 4 == 0) && (g.stride % 4 == 0) && (g.frame_pitch % 4 == 0) && ((uintptr_t)b.frames % 4 == 0);
    // 32-bit offsets: one launch covers as many frames as keep the extent below 4 GiB - 4096 (as k_binary's FAST path does)
    const int64_t lim = 0xFFFFF000ll;
    const int chunk = aligned ? (int)std::min<int64_t>(g.n_frames, std::max<int64_t>(1, (lim - 1) / g.frame_pitch)) : g.n_frames;
    const bool fast = aligned && (int64_t)(chunk - 1) * g.frame_pitch + (int64_t)(g.h - 1) * g.stride + 3 * (int64_t)g.w < lim;
    for (int f0 = 0; f0 < g.n_frames; f0 += chunk) {
        const int nf = std::min(chunk, g.n_frames - f0);
        const int n_units = nf * strips;
        // persistent grid, a multiple of the CU count: 8 workgroups of 4 wavefronts fill a CU's wave slots
        const int grid = std::min(n_cu * 8, ((n_units + n_cu - 1) / n_cu) * n_cu);
        const uint8_t* frames = b.frames + (int64_t)f0 * g.frame_pitch;
        unsigned long long* sums = reinterpret_cast<unsigned long long*>(b.enh_sums) + (int64_t)f0 * 3;
        e = fast ? launch(k_frame_sums<1>, dim3(grid), dim3(256), 0, s, frames, g.frame_pitch, g.stride, nf, g.w, g.h, strips, n_units, sums)
                 : launch(k_frame_sums<0>, dim3(grid), dim3(256), 0, s, frames, g.frame_pitch, g.stride, nf, g.w, g.h, strips, n_units, sums);
        if (e != hipSuccess) return e;
    }
    int lb = lower_bound;
    if (lb < 1) lb = 1; // (lb <= 0: everything passes and the pixel kernel reads no table)
    if (lb > 256) lb = 256;
    return launch(k_enhance_table, dim3(g.n_frames), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(b.enh_sums), (int64_t)g.w * g.h,
                  g.enh_max_gain, g.enh_min_gain, lb, b.enh_gamma, b.enh_lut, b.enh_m);
}

hipError_t launch_gamma_lut(float gamma, uint8_t* d_lut, hipStream_t s) { return launch(k_gamma_lut, dim3(1), dim3(256), 0, s, gamma, d_lut); }

hipError_t launch_bytemap(const uint8_t* d_src, uint8_t* d_dst, int64_t n16, const uint8_t* d_lut, int n_cu, hipStream_t s)
{
    if (n16 <= 0) return hipSuccess;
    const int64_t want = (n16 + 255) / 256;
    const int grid = (int)std::min<int64_t>(want, (int64_t)(n_cu > 0 ? n_cu : 256) * 8);
    return launch(k_bytemap, dim3(grid), dim3(256), 0, s, reinterpret_cast<const u32x4e*>(d_src), reinterpret_cast<u32x4e*>(d_dst), n16, d_lut);
}

} // namespace rmcv
