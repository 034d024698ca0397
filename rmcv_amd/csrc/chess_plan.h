// chess_plan.h -- what the chessboard detector (k_chess.hip, device_chess.h) decides outside its kernels: the limits, every
// refusal of its entry points, the LDS its workgroups need and the launch shapes.  Pure functions of plain values, without HIP types, so that
// a host compiler alone can check them (tests/test_chess_plan.py); the entry points and launch_chess read the same functions.
#pragma once

#include <stdint.h>

#include "../../include/rmcv_abi.h"
#include "corner_plan.h"
#include "source_view_plan.h"

namespace rmcv {

static constexpr int CHESS_SIDE_MIN = 2, CHESS_SIDE_MAX = 32, CHESS_NMS_MAX = 7, CHESS_DIST_MAX = 1023, CHESS_EXTENT_MAX = 32767;

static_assert(CHESS_SIDE_MAX * CHESS_SIDE_MAX <= RMCV_CORNER_PER_FRAME_MAX && RMCV_CORNER_PER_FRAME_MAX <= RMCV_CHESS_CAND_MAX, "a board fits a corner row and a candidate list");

inline rmcv_chess_params chess_default_params() { return {1000, 10, 3, 6, 255}; }

// ---- the refusals: the message an entry point fails with (RMCV_ERR_BAD_ARG), or null ----
// the pattern and the rule's parameters, the same for every entry point
inline const char* chess_params_refusal(int cols, int rows, const rmcv_chess_params& p)
{
    if (cols < CHESS_SIDE_MIN || rows < CHESS_SIDE_MIN || cols > CHESS_SIDE_MAX || rows > CHESS_SIDE_MAX) return "chessboard: cols and rows must be 2 .. 32";
    if (p.threshold < 0) return "chessboard: threshold must be >= 0";
    if (p.contrast < 0 || p.contrast > 255) return "chessboard: contrast must be 0 .. 255";
    if (p.nms < 1 || p.nms > CHESS_NMS_MAX) return "chessboard: nms must be 1 .. 7";
    if (p.dist_min < 1 || p.dist_min > p.dist_max || p.dist_max > CHESS_DIST_MAX) return "chessboard: 1 <= dist_min <= dist_max <= 1023";
    return nullptr;
}
// the image of the host and the stage-wise form
inline const char* chess_image_refusal(const void* bgr, const void* corners, int w, int h, int stride)
{
    if (!bgr || !corners) return "null buffer";
    if (w < 1 || h < 1) return "the image needs w >= 1 and h >= 1";
    if (w > CHESS_EXTENT_MAX || h > CHESS_EXTENT_MAX) return "chessboard: the image may be at most 32767 x 32767";
    if (stride < 3 * (int64_t)w) return "stride < 3 w";
    return nullptr;
}
static constexpr const char* CHESS_PER_FRAME = "chessboard: per_frame must be cols * rows .. 1024";
static constexpr const char* CHESS_BEYOND_LIMITS = "rmcv_find_chessboard: image beyond the context's max_width / max_height";
static constexpr const char* CHESS_NULL_TABLE = "chessboard: null corner or count table";
static constexpr const char* CHESS_NOTHING_BOUND = "chessboard: no frames are bound";
static constexpr const char* CHESS_NEEDS_RUN = "chessboard: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)";
// the batch entry points (rmcv_batch_find_chessboards, rmcv_batch_get_chessboard): the frame-list rule in the source views' words, then the
// tables and the parameters.  kind: source_kind of the batch; stages: those of its last run
inline const char* chessboards_refusal(const int32_t* frames, int n, int n_frames, int kind, int stages, const void* d_corners, const void* d_counts, int per_frame,
                                       int cols, int rows, const rmcv_chess_params& p)
{
    if (const FrameListFault bad = frame_list_fault(frames, n, n_frames)) return SOURCE_VIEW_FRAME_LIST[bad];
    if (!d_corners || !d_counts) return CHESS_NULL_TABLE;
    if (const char* why = chess_params_refusal(cols, rows, p)) return why;
    if (per_frame < cols * rows || per_frame > RMCV_CORNER_PER_FRAME_MAX) return CHESS_PER_FRAME;
    if ((kind == SOURCE_BGR_WIN || kind == SOURCE_BGR_LUT) && !(stages & RMCV_STAGE_BINARY)) return CHESS_NEEDS_RUN;
    return nullptr;
}

// ---- k_chess_response: a 256-thread workgroup owns a 64 x 32 tile of one chosen frame ----
static constexpr int CHESS_TILE_X = 64, CHESS_TILE_Y = 32, CHESS_RING_R = 5;
RMCV_PLAN_FN int chess_tiles_x(int w) { return (w + CHESS_TILE_X - 1) / CHESS_TILE_X; }
RMCV_PLAN_FN int chess_tiles_y(int h) { return (h + CHESS_TILE_Y - 1) / CHESS_TILE_Y; }
// LDS: the tile's gray bytes with a halo of 5 + nms and its responses with a halo of nms, int16 (R lies in -30600 .. 10200).  Both images
// have the pitch of the widest halo whatever nms is, so that every tap's offset is a constant of the compile; a call fills the columns and
// rows its nms needs.  Static: 88 x 56 bytes + 78 x 46 x 2 = 12 104 bytes a workgroup.
static constexpr int CHESS_GRAY_PITCH = CHESS_TILE_X + 2 * (CHESS_RING_R + CHESS_NMS_MAX), CHESS_RESP_PITCH = CHESS_TILE_X + 2 * CHESS_NMS_MAX;
RMCV_PLAN_FN int chess_gray_cols(int nms) { return CHESS_TILE_X + 2 * (CHESS_RING_R + nms); }
RMCV_PLAN_FN int chess_gray_rows(int nms) { return CHESS_TILE_Y + 2 * (CHESS_RING_R + nms); }
RMCV_PLAN_FN int chess_resp_cols(int nms) { return CHESS_TILE_X + 2 * nms; }
RMCV_PLAN_FN int chess_resp_rows(int nms) { return CHESS_TILE_Y + 2 * nms; }
static constexpr int CHESS_GRAY_MAX = CHESS_GRAY_PITCH * (CHESS_TILE_Y + 2 * (CHESS_RING_R + CHESS_NMS_MAX));
static constexpr int CHESS_RESP_MAX = CHESS_RESP_PITCH * (CHESS_TILE_Y + 2 * CHESS_NMS_MAX);
static constexpr int CHESS_RESPONSE_LDS_BYTES = CHESS_GRAY_MAX + 2 * CHESS_RESP_MAX;
static_assert(CHESS_GRAY_MAX % 4 == 0 && CHESS_TILE_Y % 4 == 0, "gray bytes are held as dwords; four wavefronts share a tile's rows");

// ---- k_chess_grid: one 512-thread workgroup per chosen frame.  LDS per candidate slot: the appended and the sorted key and response (16
// bytes), accepted and mutual neighbours (2 x 4 int16), label and direction (2 x 2 int16), queue, grid and order (3 int16), seen (1 byte): 47
// bytes, 48 128 a workgroup, plus one word.
static constexpr int CHESS_GRID_THREADS = 512;
static constexpr int CHESS_GRID_SLOT_BYTES = 16 + 16 + 8 + 6 + 1;
static constexpr int CHESS_GRID_LDS_BYTES = RMCV_CHESS_CAND_MAX * CHESS_GRID_SLOT_BYTES + 4;
// the candidate lists between the two kernels, per chosen frame: a count word, RMCV_CHESS_CAND_MAX keys and as many responses
static constexpr int CHESS_LIST_WORDS = 2 * RMCV_CHESS_CAND_MAX;

} // namespace rmcv
