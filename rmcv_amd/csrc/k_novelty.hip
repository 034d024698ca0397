// k_novelty.hip -- the dataset harvest's novelty filter (the rule: device_novelty.h).  One launch in front of k_harvest_plan
// when the dataset's ring_rows > 0, and the copy that stands in for k_harvest_rows when the rows come from memory.
//
//   k_harvest_novel<SRC>  one workgroup of eight wavefronts per stream (= frame of the append); the grid is n_frames, known on the host from the
//                         bound batch.  Wavefront 0 reads the stream's ring (at most 8 rows of 1200 bytes) into LDS once and owns the chain.
//                         Then, in rounds of eight candidates in armour order: each wavefront computes one candidate's row with icon_row
//                         (device_classify.h, the function k_harvest_rows computes it with) or reads it from memory into 1200 bytes of
//                         LDS -- the rows do not depend on the decisions, only the decisions on each other -- a workgroup barrier, and
//                         wavefront 0 decides the round's candidates one after the other: the distance to every held ring row summed as
//                         packed bytes (v_sad_u8: four bytes per instruction, 300 words over 64 lanes) and reduced over the wave, a
//                         wave-uniform decision, a kept row pushed to the ring in LDS and written through to the ring in memory.
//                         Writes one keep byte per candidate armour, the stream's pushed, and adds the stream's near count with one
//                         atomic (an integer sum: the order does not matter).  Barriers are the workgroup's own: no workgroup waits for
//                         another; no lane-private array.  (One wavefront per stream, the first form, spent a stream's whole chain of
//                         icon_row latencies in sequence: DESIGN.md 4n has both forms' times.)
//                         SRC: the four pixel accessors of k_harvest_rows* (BGR, BGR through the window origin, mosaics, frames through
//                         their gamma tables) and rows from memory (rmcv_dataset_append_rows).
//   k_harvest_plan_novel  k_harvest_plan's body (k_harvest_plan.inc) compiled a second time: the keep bytes are a further input of harvest_keeps.
//   k_harvest_copy_rows   rows from memory: walks k_harvest_plan's work list as k_harvest_rows does, 75 uint4 per row, and fills meta[slot].
#include "device_classify.h"
#include "device_harvest.h"
#include "device_novelty.h"

namespace rmcv {

enum { NOVEL_BGR = 0, NOVEL_WIN = 1, NOVEL_BAYER = 2, NOVEL_ENH = 3, NOVEL_MEM = 4 };
static constexpr int NOVEL_WORDS = NOVEL_ROW / 4, NOVEL_WAVES = 8, NOVEL_THREADS = 64 * NOVEL_WAVES;
static_assert(NOVEL_ROW % 16 == 0 && NOVEL_ROW == NFEAT, "a row is 300 words, 75 uint4");

struct NovelArgs {
    // the batch (SRC != NOVEL_MEM) ...
    const uint8_t* frames;
    int64_t frame_pitch;
    int stride, w, h;
    const rmcv_armour* armours;
    const int32_t* status;
    const int32_t* identity;   // read only with RMCV_HARVEST_MISSES
    const rmcv_point* win_eff; // NOVEL_WIN
    // ... or the rows in memory (NOVEL_MEM)
    const uint8_t* src_rows;
    const int32_t* row_off;
    // both
    const int32_t* n_armours; // NOVEL_MEM: n_rows
    const int32_t* labels;
    int n_frames, max_armours, flags;
    // the dataset's state
    int ring_rows;
    int32_t max_sad;
    uint8_t* rings;
    int64_t* pushed;
    unsigned long long* near;
    uint8_t* keep;
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

template <int SRC>
__device__ __forceinline__ void harvest_novel(const NovelArgs& N, int pattern, int lay, const uint8_t* __restrict__ luts)
{
    __shared__ uint32_t s_cand[NOVEL_WAVES][NOVEL_WORDS];
    __shared__ uint32_t s_ring[RMCV_HARVEST_RING_MAX * NOVEL_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x;
    if (f >= N.n_frames) return; // (the same for the whole workgroup, like every return and loop bound in front of a barrier below)
    const int R = N.ring_rows < RMCV_HARVEST_RING_MAX ? N.ring_rows : RMCV_HARVEST_RING_MAX, ma = N.max_armours;
    const int32_t label = N.labels[f];
    const int m = harvest_candidates(N.n_armours[f], ma, SRC == NOVEL_MEM ? 0 : N.status[f], label);
    if (m == 0 || R < 1) return; // the ring and pushed stay untouched
    uint32_t* cand = s_cand[wave];
    uint32_t* gring = reinterpret_cast<uint32_t*>(N.rings + (int64_t)f * R * NOVEL_ROW);
    // the chain's state lives in wavefront 0: the ring in LDS is read and written by it alone
    int64_t pushed = 0;
    int held = 0;
    uint32_t near = 0;
    if (wave == 0) {
        pushed = N.pushed[f];
        held = novelty_held(pushed, R);
        for (int i = lane; i < held * NOVEL_WORDS; i += 64) s_ring[i] = gring[i];
    }
    for (int base = 0; base < m; base += NOVEL_WAVES) {
        // the rows of candidates base .. base + 7, one wavefront each
        const int a = base + wave;
        if (a < m && harvest_keeps(N.flags, (N.flags & RMCV_HARVEST_MISSES) ? N.identity[(int64_t)f * ma + a] : 0, label)) { // (wave-uniform)
            if constexpr (SRC == NOVEL_MEM) {
                const uint32_t* src = reinterpret_cast<const uint32_t*>(N.src_rows + ((int64_t)N.row_off[f] + a) * NOVEL_ROW);
                for (int i = lane; i < NOVEL_WORDS; i += 64) cand[i] = src[i];
            } else {
                const uint8_t* frame = N.frames + (int64_t)f * N.frame_pitch + (SRC == NOVEL_WIN ? frame_origin_offset(N.win_eff, f, N.stride) : 0);
                uint8_t* bytes = reinterpret_cast<uint8_t*>(cand);
                float ic[4][2];
                icon_row<SRC == NOVEL_BAYER ? 1 : (SRC == NOVEL_ENH ? 2 : 0)>(frame, f, lane, N.armours + (int64_t)f * ma + a, N.w, N.h, N.stride, pattern, lay, luts, ic,
                                                                            [&](int o, const int (&res)[3]) __attribute__((always_inline)) {
#pragma unroll
                                                                                for (int c = 0; c < 3; c++) bytes[o * 3 + c] = (uint8_t)res[c];
                                                                            });
            }
        }
        __syncthreads();
        // the decisions, in armour order
        if (wave == 0) {
            const int top = m - base < NOVEL_WAVES ? m - base : NOVEL_WAVES;
            for (int j = 0; j < top; j++) {
                uint8_t* keep = N.keep + (int64_t)f * ma + base + j;
                if (!harvest_keeps(N.flags, (N.flags & RMCV_HARVEST_MISSES) ? N.identity[(int64_t)f * ma + base + j] : 0, label)) {
                    if (lane == 0) *keep = 0;
                    continue;
                }
                const uint32_t* row = s_cand[j];
                // d: the minimum over the held rows of the wave's sum of packed-byte distances
                int32_t d = NOVEL_NO_SAD;
                for (int k = 0; k < held; k++) {
                    uint32_t acc = 0;
                    for (int i = lane; i < NOVEL_WORDS; i += 64) acc = __builtin_amdgcn_sad_u8(row[i], s_ring[k * NOVEL_WORDS + i], acc);
                    const int32_t sum = (int32_t)wave_sum_u32(acc);
                    d = sum < d ? sum : d;
                }
                d = __builtin_amdgcn_readfirstlane(d);
                if (novelty_near(d, N.max_sad)) {
                    near++;
                    if (lane == 0) *keep = 0;
                    continue;
                }
                const int pos = novelty_position(pushed, R);
                for (int i = lane; i < NOVEL_WORDS; i += 64) {
                    const uint32_t v = row[i];
                    s_ring[pos * NOVEL_WORDS + i] = v;
                    gring[pos * NOVEL_WORDS + i] = v;
                }
                __builtin_amdgcn_wave_barrier(); // (the next candidate reads the ring behind these writes)
                pushed++;
                held = novelty_held(pushed, R);
                if (lane == 0) *keep = 1;
            }
        }
        __syncthreads(); // (the next round's rows overwrite s_cand)
    }
    if (wave == 0 && lane == 0) {
        N.pushed[f] = pushed;
        if (near) atomicAdd(N.near, (unsigned long long)near);
    }
}

__global__ __launch_bounds__(NOVEL_THREADS) void k_harvest_novel(NovelArgs N) { harvest_novel<NOVEL_BGR>(N, 0, 0, nullptr); }
__global__ __launch_bounds__(NOVEL_THREADS) void k_harvest_novel_win(NovelArgs N) { harvest_novel<NOVEL_WIN>(N, 0, 0, nullptr); }
__global__ __launch_bounds__(NOVEL_THREADS) void k_harvest_novel_bayer(NovelArgs N, int pattern, int lay) { harvest_novel<NOVEL_BAYER>(N, pattern, lay, nullptr); }
__global__ __launch_bounds__(NOVEL_THREADS) void k_harvest_novel_enh(NovelArgs N, const uint8_t* __restrict__ luts) { harvest_novel<NOVEL_ENH>(N, 0, 0, luts); }
__global__ __launch_bounds__(NOVEL_THREADS) void k_harvest_novel_mem(NovelArgs N) { harvest_novel<NOVEL_MEM>(N, 0, 0, nullptr); }

// the keep bytes as a further input of harvest_keeps: harvest_frame_kept / harvest_frame_emit of device_harvest.h with `keep`, the frame's row
// of the keep table
__device__ inline int novel_frame_kept(int32_t n, int max_armours, int32_t status, int32_t label, int flags, const int32_t* ident, const uint8_t* keep)
{
    const int m = harvest_candidates(n, max_armours, status, label);
    int k = 0;
    for (int a = 0; a < m; a++) k += harvest_keeps(flags, (flags & RMCV_HARVEST_MISSES) ? ident[a] : 0, label) && keep[a];
    return k;
}
__device__ inline int novel_frame_emit(int f, int32_t n, int max_armours, int32_t status, int32_t label, int flags, const int32_t* ident, int64_t k0,
                                       int32_t count, int32_t capacity, HarvestItem* list, const uint8_t* keep)
{
    const int m = harvest_candidates(n, max_armours, status, label);
    int k = 0;
    for (int a = 0; a < m; a++) {
        if (!(harvest_keeps(flags, (flags & RMCV_HARVEST_MISSES) ? ident[a] : 0, label) && keep[a])) continue;
        const int64_t slot = (int64_t)count + k0 + k;
        if (slot < capacity) list[k0 + k] = HarvestItem{f, a, (int32_t)slot};
        k++;
    }
    return k;
}
// k_harvest_plan's body once more (k_harvest_plan.inc), with the keep bytes: the same work list and counters
#define HP_KERNEL k_harvest_plan_novel
#define HP_NOVEL
#include "k_harvest_plan.inc"
#undef HP_NOVEL
#undef HP_KERNEL

struct CopyRowsArgs {
    const uint8_t* src_rows;
    const int32_t* row_off;
    const int32_t* labels;
    const HarvestCounters* ctr;
    const HarvestItem* list;
    uint8_t* rows;
    rmcv_harvest_meta* meta;
    int32_t capacity;
    int n_streams, max_armours;
    uint64_t tag;
};

__global__ __launch_bounds__(256) void k_harvest_copy_rows(CopyRowsArgs H)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
    const int n_list = H.ctr->n_list;
    for (int e = wave; e < n_list; e += nwaves) {
        const HarvestItem it = H.list[e];
        if (it.slot < 0 || it.slot >= H.capacity || it.frame < 0 || it.frame >= H.n_streams || it.armour < 0 || it.armour >= H.max_armours) continue; // (the plan never writes such an entry)
        const uint4* src = reinterpret_cast<const uint4*>(H.src_rows + ((int64_t)H.row_off[it.frame] + it.armour) * NOVEL_ROW);
        uint4* dst = reinterpret_cast<uint4*>(H.rows + (int64_t)it.slot * NOVEL_ROW);
        for (int i = lane; i < NOVEL_ROW / 16; i += 64) dst[i] = src[i];
        if (lane == 0) {
            rmcv_harvest_meta m;
            m.tag = H.tag;
            m.frame = it.frame, m.armour = it.armour, m.label = H.labels[it.frame];
            m.identity = INT32_MIN;
            m.win_x = 0, m.win_y = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) { m.icon[i][0] = 0.0f; m.icon[i][1] = 0.0f; }
            H.meta[it.slot] = m;
        }
    }
}

hipError_t launch_harvest_novel(const Geom& g, const Bufs& b, const Limits& lim, const DatasetRowsSource* src, const DatasetView& d, const int32_t* d_labels,
                                int flags, const int32_t* ident, hipStream_t s)
{
    NovelArgs N{};
    N.labels = d_labels, N.flags = flags;
    N.ring_rows = d.ring_rows, N.max_sad = d.max_sad, N.rings = d.rings, N.pushed = d.pushed, N.near = d.near, N.keep = d.keep;
    if (src) {
        N.src_rows = src->rows, N.row_off = src->row_off, N.n_armours = src->n_rows, N.n_frames = src->n_streams, N.max_armours = src->max_armours;
        return launch(k_harvest_novel_mem, dim3((unsigned)N.n_frames), dim3(NOVEL_THREADS), 0, s, N);
    }
    N.frames = b.frames, N.frame_pitch = g.frame_pitch, N.stride = g.stride, N.w = g.w, N.h = g.h;
    N.armours = b.armours, N.status = b.status, N.identity = ident, N.win_eff = g.win ? b.win_eff : nullptr;
    N.n_armours = b.n_armours, N.n_frames = g.n_frames, N.max_armours = lim.max_armours;
    const dim3 grid((unsigned)g.n_frames), block(NOVEL_THREADS); // from the bound batch, never from data
    if (g.input_format != RMCV_INPUT_BGR)
        return launch(k_harvest_novel_bayer, grid, block, 0, s, N, g.input_format, raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient));
    if (g.enhance) return launch(k_harvest_novel_enh, grid, block, 0, s, N, b.enh_lut);
    if (g.win) return launch(k_harvest_novel_win, grid, block, 0, s, N);
    return launch(k_harvest_novel, grid, block, 0, s, N);
}

hipError_t launch_harvest_plan_novel(const int32_t* n_armours, const int32_t* status, const int32_t* d_labels, const int32_t* ident, int n_frames, int max_armours,
                                     int flags, const DatasetView& d, hipStream_t s)
{
    return launch(k_harvest_plan_novel, dim3(1), dim3(256), 0, s, n_armours, status, d_labels, ident, d.keep, n_frames, max_armours, flags, d.capacity, d.ctr, d.list);
}

hipError_t launch_harvest_rows_source(const DatasetRowsSource& src, const DatasetView& d, int n_cu, uint64_t tag, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (d.ring_rows > 0) e = launch_harvest_novel(Geom{}, Bufs{}, Limits{}, &src, d, src.labels, 0, nullptr, s);
    if (e == hipSuccess) e = launch_harvest_plan(src.n_rows, src.zeros, src.labels, nullptr, src.n_streams, src.max_armours, 0, d, s);
    if (e != hipSuccess) return e;
    CopyRowsArgs H;
    H.src_rows = src.rows, H.row_off = src.row_off, H.labels = src.labels, H.ctr = d.ctr, H.list = d.list, H.rows = d.rows, H.meta = d.meta;
    H.capacity = d.capacity, H.n_streams = src.n_streams, H.max_armours = src.max_armours, H.tag = tag;
    // as k_harvest_rows: one wavefront per row the call can have, up to four workgroups of four per CU
    const int64_t most = (int64_t)src.n_streams * src.max_armours;
    const int64_t groups = (most + 3) / 4, cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 4;
    return launch(k_harvest_copy_rows, dim3((unsigned)(groups < 1 ? 1 : (groups < cap ? groups : cap))), dim3(256), 0, s, H);
}

} // namespace rmcv
