// device_novelty.h -- the dataset harvest's novelty rule: which candidates of an append are near-duplicates of icons the
// dataset kept from the same stream a moment ago, and are therefore not kept.  Pure functions of plain values, compiled for the device
// (k_novelty.hip: k_harvest_novel) and for the host (rmcv_icon_sad, rmcv_harvest_novel_host, tests/novelty_san_main.cpp): one source
// for both.  Integers only: host and device agree bit for bit.
//
// Distance.  icon_sad(a, b) = sum over i < 1200 of |a[i] - b[i]| of two icon rows: an int32 in 0 .. RMCV_ICON_SAD_MAX (1200 * 255 = 306000).
//
// State of a dataset.  ring_rows R in 0 .. RMCV_HARVEST_RING_MAX (0: novelty is off), max_sad T in 0 .. RMCV_ICON_SAD_MAX, a counter
// `near` (int64), and per stream s in 0 .. label_cap - 1 (stream s is frame s of every append, as the label table has it): pushed[s]
// (int64), the rows ever pushed since the last reset, and a ring ring[s][R][1200] in which the row pushed as number k lies at position
// k % R.  The ring holds rows number max(0, pushed - R) .. pushed - 1; positions not yet written since the last reset are zero.
//
// One append with R > 0.
//   * the candidates of frame f are those device_harvest.h keeps: none when the label is RMCV_HARVEST_SKIP or the status word carries an
//     RMCV_FRAME_OVF_* bit, otherwise armours 0 .. min(n, max_armours) - 1, and under RMCV_HARVEST_MISSES only those with identity != label;
//   * candidates are taken in armour order.  For each, d is the minimum of icon_sad(row, r) over the rows r the ring of stream f holds at
//     that moment -- rows pushed by earlier candidates of the same frame in the same append included.  An empty ring gives no d: the
//     candidate is kept;
//   * d <= T: the candidate is near.  It is not kept and near += 1;
//   * otherwise the candidate is kept and its row is pushed to the ring of stream f;
//   * kept rows are numbered and placed as device_harvest.h says (frame-major, then armour-major; kept row k to slot count + k; a slot
//     >= capacity is dropped and counted).  A kept row is pushed to its ring whether or not it found a slot: a full dataset's rings, pushed
//     and near are those of an unbounded one, and its rows a prefix of that one's;
//   * streams never read each other's rings; a frame without candidates leaves its ring and pushed untouched.
// With R == 0 every candidate is kept and no state is read or written.
#pragma once
#include <stdint.h>

#include "../../include/rmcv_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RMCV_NOVELTY_HD __host__ __device__
#else
#define RMCV_NOVELTY_HD
#endif

namespace rmcv {

static constexpr int NOVEL_ROW = RMCV_SVM_FEATURES; // bytes of an icon row
static constexpr int32_t NOVEL_NO_SAD = INT32_MAX;  // "the ring was empty"
static_assert(NOVEL_ROW * 255 == RMCV_ICON_SAD_MAX, "the largest distance of two rows");

RMCV_NOVELTY_HD inline int32_t icon_sad(const uint8_t* a, const uint8_t* b)
{
    int32_t s = 0;
    for (int i = 0; i < NOVEL_ROW; i++) s += a[i] > b[i] ? a[i] - b[i] : b[i] - a[i];
    return s;
}
// rows a ring of depth R holds after `pushed` pushes; they lie at positions 0 .. this - 1
RMCV_NOVELTY_HD inline int novelty_held(int64_t pushed, int R) { return pushed < R ? (int)pushed : R; }
// the position the next pushed row goes to
RMCV_NOVELTY_HD inline int novelty_position(int64_t pushed, int R) { return (int)(pushed % R); }
// whether a candidate at distance d (NOVEL_NO_SAD: the ring was empty) is near
RMCV_NOVELTY_HD inline bool novelty_near(int32_t d, int32_t T) { return d != NOVEL_NO_SAD && d <= T; }
// the candidates of a stream of rmcv_dataset_append_rows / rmcv_harvest_novel_host
RMCV_NOVELTY_HD inline int novelty_row_candidates(int32_t n_rows, int32_t label) { return label == RMCV_HARVEST_SKIP || n_rows < 0 ? 0 : n_rows; }

// d of one candidate against one stream's ring [R][1200]
inline int32_t novelty_min_sad(const uint8_t* row, const uint8_t* ring, int R, int64_t pushed)
{
    int32_t d = NOVEL_NO_SAD;
    const int held = novelty_held(pushed, R);
    for (int k = 0; k < held; k++) {
        const int32_t s = icon_sad(row, ring + (int64_t)k * NOVEL_ROW);
        if (s < d) d = s;
    }
    return d;
}
// One candidate of one stream: decides, pushes a kept row.  Returns whether it is kept; *d_out (nullable) its distance.
inline bool novelty_step(const uint8_t* row, uint8_t* ring, int R, int32_t T, int64_t* pushed, int32_t* d_out)
{
    const int32_t d = novelty_min_sad(row, ring, R, *pushed);
    if (d_out) *d_out = d;
    if (novelty_near(d, T)) return false;
    uint8_t* at = ring + (int64_t)novelty_position(*pushed, R) * NOVEL_ROW;
    for (int i = 0; i < NOVEL_ROW; i++) at[i] = row[i];
    *pushed += 1;
    return true;
}
// The whole call over rows the caller has, sequentially (rmcv_harvest_novel_host).  rows: [sum n_rows][1200], stream-major (a skipped
// stream's rows are stepped over); rings [n_streams][R][1200] and pushed [n_streams]: in and out; keep [sum n_rows]: 1 kept, 0 near or
// skipped; min_sad (nullable) [sum n_rows].  Returns the near candidates of the call.  R == 0: every candidate is kept, no state is touched.
inline int64_t novelty_seq(const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, int R, int32_t T, uint8_t* rings,
                           int64_t* pushed, uint8_t* keep, int32_t* min_sad)
{
    int64_t at = 0, near = 0;
    for (int s = 0; s < n_streams; s++) {
        const int m = novelty_row_candidates(n_rows[s], labels[s]);
        for (int a = 0; a < n_rows[s]; a++, at++) {
            int32_t d = NOVEL_NO_SAD;
            bool k = a < m;
            if (k && R > 0) k = novelty_step(rows + at * NOVEL_ROW, rings + (int64_t)s * R * NOVEL_ROW, R, T, pushed + s, &d);
            if (a < m && !k) near++;
            keep[at] = k ? 1 : 0;
            if (min_sad) min_sad[at] = d;
        }
    }
    return near;
}

// why rmcv_dataset_set_novelty refuses its arguments (null: it does not)
inline const char* novelty_refusal(int ring_rows, int32_t max_sad)
{
    if (ring_rows < 0 || ring_rows > RMCV_HARVEST_RING_MAX) return "novelty: ring_rows outside 0 .. RMCV_HARVEST_RING_MAX";
    if (max_sad < 0 || max_sad > RMCV_ICON_SAD_MAX) return "novelty: max_sad outside 0 .. RMCV_ICON_SAD_MAX";
    return nullptr;
}
// why rmcv_dataset_append_rows refuses its arguments (null: it does not)
inline const char* novelty_rows_refusal(const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, int label_cap, int max_armours)
{
    if (n_streams < 1 || n_streams > label_cap) return "append_rows: n_streams outside 1 .. the creating context's max_frames";
    if (!rows || !n_rows || !labels) return "append_rows: a null pointer";
    for (int s = 0; s < n_streams; s++)
        if (n_rows[s] < 0 || n_rows[s] > max_armours) return "append_rows: a stream's n_rows outside 0 .. the creating context's max_armours";
    return nullptr;
}

} // namespace rmcv
