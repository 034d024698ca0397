// device_harvest.h -- the dataset harvest's rule: which armours of a batch become rows of a device-resident dataset, and
// where.  Pure functions of plain values, compiled for the device (k_harvest.hip: k_harvest_plan) and for the host
// (rmcv_harvest_plan_host, tests/test_harvest_plan.py, tests/harvest_san_main.cpp): one source for both.
//
// One append call: per-frame armour counts n[f], status words, labels label[f]; per-armour identities (optional); flags; the dataset's
// count and capacity before the call.
//   * frame f contributes nothing when label[f] == RMCV_HARVEST_SKIP, or when its status word carries an RMCV_FRAME_OVF_* bit (its tables
//     are then not its lists: the rule of rmcv_batch_get_debug_view);
//   * otherwise its candidates are armours 0 .. min(n[f], max_armours) - 1 in table order (the order of rmcv_batch_get_armours);
//   * RMCV_HARVEST_MISSES keeps a candidate only when identity != label[f]; without the flag every candidate is kept;
//   * kept rows are numbered frame-major, then armour-major; kept row k of the call goes to slot count + k;
//   * a row whose slot is >= capacity is dropped: count' = min(count + kept, capacity), dropped' = dropped + max(0, count + kept - capacity).
//     A full dataset is a prefix of what an unbounded one would hold.
#pragma once
#include <stdint.h>

#include "../../include/rmcv_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RMCV_HARVEST_HD __host__ __device__
#else
#define RMCV_HARVEST_HD
#endif

namespace rmcv {

static constexpr int HARVEST_OVF = RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS | RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_OVF_ARMOURS;

// one entry of the work list k_harvest_plan leaves for k_harvest_rows: a kept row that has a slot
struct HarvestItem { int32_t frame, armour, slot; };

// the counters of a dataset as they live on the device
struct HarvestCounters {
    int32_t count;   // rows held, <= capacity
    int32_t n_list;  // entries of the work list of the append enqueued last
    int64_t dropped; // rows that found the dataset full, over its life (rmcv_dataset_clear zeroes it)
};

// the candidates of frame f: armours 0 .. this - 1
RMCV_HARVEST_HD inline int harvest_candidates(int32_t n, int max_armours, int32_t status, int32_t label)
{
    if (label == RMCV_HARVEST_SKIP || (status & HARVEST_OVF)) return 0;
    const int m = n < max_armours ? n : max_armours;
    return m > 0 ? m : 0;
}
// whether a candidate is kept (identity: read only with RMCV_HARVEST_MISSES)
RMCV_HARVEST_HD inline bool harvest_keeps(int flags, int32_t identity, int32_t label) { return !(flags & RMCV_HARVEST_MISSES) || identity != label; }
// kept rows of frame f; ident: the frame's row of the identity table (read only with RMCV_HARVEST_MISSES)
RMCV_HARVEST_HD inline int harvest_frame_kept(int32_t n, int max_armours, int32_t status, int32_t label, int flags, const int32_t* ident)
{
    const int m = harvest_candidates(n, max_armours, status, label);
    if (!(flags & RMCV_HARVEST_MISSES)) return m;
    int k = 0;
    for (int a = 0; a < m; a++) k += harvest_keeps(flags, ident[a], label);
    return k;
}
// the work-list entries of frame f, whose first kept row is kept row `k0` of the call: entry k (for slot count + k < capacity) -> list[k].
// Returns the frame's kept rows.
RMCV_HARVEST_HD inline int harvest_frame_emit(int f, int32_t n, int max_armours, int32_t status, int32_t label, int flags, const int32_t* ident,
                                              int64_t k0, int32_t count, int32_t capacity, HarvestItem* list)
{
    const int m = harvest_candidates(n, max_armours, status, label);
    int k = 0;
    for (int a = 0; a < m; a++) {
        if (!harvest_keeps(flags, (flags & RMCV_HARVEST_MISSES) ? ident[a] : 0, label)) continue;
        const int64_t slot = (int64_t)count + k0 + k;
        if (slot < capacity) list[k0 + k] = HarvestItem{f, a, (int32_t)slot};
        k++;
    }
    return k;
}
// the counters behind a call that kept `kept` rows; returns the work list's length (rows that got a slot)
RMCV_HARVEST_HD inline int32_t harvest_finish(int32_t count, int32_t capacity, int64_t kept, int32_t* count_out, int64_t* dropped_add)
{
    const int64_t end = (int64_t)count + kept;
    const int64_t now = end < capacity ? end : capacity;
    *count_out = (int32_t)now;
    *dropped_add = end > capacity ? end - capacity : 0;
    return (int32_t)(now - count);
}

// The whole call, sequentially (rmcv_harvest_plan_host).  list: at least min(kept, capacity - count) entries -- capacity - count always
// suffices.  identity: [n_frames][max_armours], may be null without RMCV_HARVEST_MISSES.
inline int32_t harvest_plan_seq(const int32_t* n_armours, const int32_t* status, const int32_t* labels, const int32_t* identity, int n_frames,
                                int max_armours, int flags, int32_t count, int32_t capacity, HarvestItem* list, int32_t* count_out, int64_t* dropped_add)
{
    int64_t k0 = 0;
    for (int f = 0; f < n_frames; f++)
        k0 += harvest_frame_emit(f, n_armours[f], max_armours, status[f], labels[f], flags, identity ? identity + (int64_t)f * max_armours : nullptr, k0, count,
                                 capacity, list);
    return harvest_finish(count, capacity, k0, count_out, dropped_add);
}

// why an append is refused (null: it is not); nothing is enqueued before this has answered
inline const char* harvest_refusal(bool frames_bound, int last_stages, int flags, int ctx_device, int ds_device)
{
    if (flags & ~RMCV_HARVEST_MISSES) return "harvest: unknown flags";
    if (ctx_device != ds_device) return "harvest: the dataset belongs to another device";
    if (!frames_bound) return "harvest: no frames bound";
    if (!(last_stages & RMCV_STAGE_ARMOURS)) return "harvest: the batch's last run lacked RMCV_STAGE_ARMOURS";
    if ((flags & RMCV_HARVEST_MISSES) && !(last_stages & RMCV_STAGE_IDENTITY)) return "harvest: RMCV_HARVEST_MISSES needs a run with RMCV_STAGE_IDENTITY";
    return nullptr;
}

} // namespace rmcv
