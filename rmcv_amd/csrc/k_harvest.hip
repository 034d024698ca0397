// k_harvest.hip -- the dataset harvest: the labeler's job (the reference's executable/svm/labeler.cpp: detect,
// rm::affine_correction per armour, file the icon under its label) on the device, two launches behind a batch's last run.
//
//   k_harvest_plan   one workgroup.  The rule of device_harvest.h over the batch's n_armours / status / identity tables and the label
//                    table: thread t takes frames [t * per, (t + 1) * per), per = ceil(n_frames / 256), counts their kept rows, the
//                    exclusive scan over the 256 totals is a wave64 scan (__shfl_up) with the four waves' carries through LDS; every
//                    thread then writes the (frame, armour, slot) of its frames' kept rows that have a slot into the work list, and
//                    thread 0 updates the dataset's count / dropped and leaves the list's length.
//   k_harvest_rows   a grid fixed by the context's limits and the CU count, never by data (no host read between the two launches): each
//                    wavefront walks the work list with a stride, computes the armour's 20x20xBGR row (device_classify.h: icon_row, the
//                    function classify_frame computes it with) into rows[slot] and fills meta[slot].  The loop is bounded by the list's
//                    length: no inter-workgroup wait, no spin.  The armour table is only read.
//   k_harvest_gather rows[idx[k]] -> out[k], meta[idx[k]].label -> responses[k]: a training or validation subset, contiguous.
// A dataset with novelty on (k_novelty.hip) gets k_harvest_novel in front and k_harvest_plan_novel in k_harvest_plan's place;
// k_harvest_rows then runs over the shorter list as ever.
#include "device_classify.h"
#include "device_harvest.h"

namespace rmcv {

static_assert(sizeof(rmcv_harvest_meta) == 64, "rmcv_harvest_meta is 64 bytes");
static_assert(sizeof(HarvestItem) == sizeof(rmcv_harvest_item), "the work list's entry is the ABI's item");
static_assert(NFEAT == RMCV_SVM_FEATURES && NFEAT % 16 == 0, "a row is 75 uint4");

// k_harvest_plan: the body lives in k_harvest_plan.inc and is compiled twice -- here as it always was, and in k_novelty.hip with the keep bytes
// of k_harvest_novel as a further input
#define HP_KERNEL k_harvest_plan
#include "k_harvest_plan.inc"
#undef HP_KERNEL

// what k_harvest_rows needs of the batch and the dataset
struct HarvestRowsArgs {
    const uint8_t* frames;
    int64_t frame_pitch;
    int stride, w, h, max_armours;
    const rmcv_armour* armours;
    const int32_t* labels;
    const int32_t* identity;   // null: the run had no identity stage
    const rmcv_point* win_eff; // null: whole frames
    const HarvestCounters* ctr;
    const HarvestItem* list;
    uint8_t* rows;
    rmcv_harvest_meta* meta;
    int32_t capacity;
    uint64_t tag;
};

// BAYER as device_classify.h: 0 BGR (WIN: through the frame's window origin), 1 mosaics (pattern, lay), 2 through the gamma tables (luts)
template <int BAYER, bool WIN>
__device__ __forceinline__ void harvest_rows(const HarvestRowsArgs& H, int pattern, int lay, const uint8_t* __restrict__ luts)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
    const int n_list = H.ctr->n_list;
    for (int e = wave; e < n_list; e += nwaves) {
        const HarvestItem it = H.list[e];
        if (it.slot < 0 || it.slot >= H.capacity) continue; // (the plan never writes such an entry)
        const int f = it.frame;
        const rmcv_armour* A = H.armours + (int64_t)f * H.max_armours + it.armour;
        const uint8_t* frame = H.frames + (int64_t)f * H.frame_pitch + (WIN ? frame_origin_offset(H.win_eff, f, H.stride) : 0);
        uint8_t* __restrict__ row = H.rows + (int64_t)it.slot * NFEAT;
        float ic[4][2];
        icon_row<BAYER>(frame, f, lane, A, H.w, H.h, H.stride, pattern, lay, luts, ic, [&](int o, const int (&res)[3]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < 3; c++) row[o * 3 + c] = (uint8_t)res[c];
        });
        if (lane == 0) {
            rmcv_harvest_meta m;
            m.tag = H.tag;
            m.frame = f, m.armour = it.armour, m.label = H.labels[f];
            m.identity = H.identity ? H.identity[(int64_t)f * H.max_armours + it.armour] : INT32_MIN;
            m.win_x = WIN ? H.win_eff[f].x : 0, m.win_y = WIN ? H.win_eff[f].y : 0;
#pragma unroll
            for (int i = 0; i < 4; i++) { m.icon[i][0] = ic[i][0]; m.icon[i][1] = ic[i][1]; }
            H.meta[it.slot] = m;
        }
    }
}

__global__ __launch_bounds__(256) void k_harvest_rows(HarvestRowsArgs H) { harvest_rows<0, false>(H, 0, 0, nullptr); }
__global__ __launch_bounds__(256) void k_harvest_rows_win(HarvestRowsArgs H) { harvest_rows<0, true>(H, 0, 0, nullptr); }
__global__ __launch_bounds__(256) void k_harvest_rows_bayer(HarvestRowsArgs H, int pattern, int lay) { harvest_rows<1, false>(H, pattern, lay, nullptr); }
__global__ __launch_bounds__(256) void k_harvest_rows_enh(HarvestRowsArgs H, const uint8_t* __restrict__ luts) { harvest_rows<2, false>(H, 0, 0, luts); }

// one workgroup of 128 threads per output row; idx null: row k is slot k.  A slot outside 0 .. count - 1 (the host has refused those) reads nothing.
__global__ __launch_bounds__(128) void k_harvest_gather(const uint8_t* __restrict__ rows, const rmcv_harvest_meta* __restrict__ meta,
                                                       const HarvestCounters* __restrict__ ctr, const int32_t* __restrict__ idx, int n,
                                                       uint8_t* __restrict__ out, int32_t* __restrict__ responses)
{
    const int k = blockIdx.x;
    if (k >= n) return;
    const int32_t slot = idx ? idx[k] : k;
    const bool ok = slot >= 0 && slot < ctr->count;
    if (out && threadIdx.x < NFEAT / 16) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = reinterpret_cast<const uint4*>(rows + (int64_t)slot * NFEAT)[threadIdx.x];
        reinterpret_cast<uint4*>(out + (int64_t)k * NFEAT)[threadIdx.x] = v;
    }
    if (responses && threadIdx.x == 0) responses[k] = ok ? meta[slot].label : 0;
}

hipError_t launch_harvest_plan(const int32_t* n_armours, const int32_t* status, const int32_t* d_labels, const int32_t* ident, int n_frames, int max_armours,
                               int flags, const DatasetView& d, hipStream_t s)
{
    if (d.ring_rows > 0) return launch_harvest_plan_novel(n_armours, status, d_labels, ident, n_frames, max_armours, flags, d, s);
    return launch(k_harvest_plan, dim3(1), dim3(256), 0, s, n_armours, status, d_labels, ident, n_frames, max_armours, flags, d.capacity, d.ctr, d.list);
}

hipError_t launch_harvest(const Geom& g, const Bufs& b, const Limits& lim, const DatasetView& d, const int32_t* d_labels, int flags, bool identity,
                          uint64_t tag, hipStream_t s)
{
    const int32_t* ident = identity ? b.identity : nullptr;
    hipError_t e = hipSuccess;
    // novelty on: the keep bytes first; the plan then takes them in, and the rows kernels run over its list as ever (a kept row is computed twice)
    if (d.ring_rows > 0) e = launch_harvest_novel(g, b, lim, nullptr, d, d_labels, flags, ident, s);
    if (e == hipSuccess) e = launch_harvest_plan(b.n_armours, b.status, d_labels, ident, g.n_frames, lim.max_armours, flags, d, s);
    if (e != hipSuccess) return e;
    HarvestRowsArgs H;
    H.frames = b.frames, H.frame_pitch = g.frame_pitch, H.stride = g.stride, H.w = g.w, H.h = g.h, H.max_armours = lim.max_armours;
    H.armours = b.armours, H.labels = d_labels, H.identity = ident, H.win_eff = g.win ? b.win_eff : nullptr;
    H.ctr = d.ctr, H.list = d.list, H.rows = d.rows, H.meta = d.meta, H.capacity = d.capacity, H.tag = tag;
    // one wavefront per row the batch can have, up to four workgroups of four per CU: fixed by limits and the device, never by data
    const int64_t most = (int64_t)lim.max_frames * lim.max_armours;
    const int64_t groups = (most + 3) / 4, cap = (int64_t)(g.n_cu > 0 ? g.n_cu : 256) * 4;
    const dim3 grid((unsigned)(groups < 1 ? 1 : (groups < cap ? groups : cap)));
    if (g.input_format != RMCV_INPUT_BGR)
        return launch(k_harvest_rows_bayer, grid, dim3(256), 0, s, H, g.input_format, raw_layout(8 * g.sample_bytes, g.valid_bit, g.orient));
    if (g.enhance) return launch(k_harvest_rows_enh, grid, dim3(256), 0, s, H, b.enh_lut);
    if (g.win) return launch(k_harvest_rows_win, grid, dim3(256), 0, s, H);
    return launch(k_harvest_rows, grid, dim3(256), 0, s, H);
}

hipError_t launch_harvest_gather(const DatasetView& d, const int32_t* d_idx, int n, uint8_t* d_out, int32_t* d_responses, hipStream_t s)
{
    if (n < 1) return hipSuccess;
    return launch(k_harvest_gather, dim3(n), dim3(128), 0, s, d.rows, d.meta, d.ctr, d_idx, n, d_out, d_responses);
}

} // namespace rmcv
