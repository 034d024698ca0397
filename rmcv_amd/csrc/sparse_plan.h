// sparse_plan.h -- which launches a run's sparse stage makes (k_contours.hip: launch_contours_x).  A pure function of plain values,
// without HIP types, so that a host compiler alone can check it (tests/test_sparse_plan.py).
#pragma once

#include <stddef.h>

namespace rmcv {

// RunPlan::form: how a run treats the frames beyond findContours' LDS tables.  LEAN: a pipeline's dense mode, every frame through the lean
// build (k_contours_lean.hip).  SPLIT_*: such frames are marked by the 4-wavefront launch and left to one with 8 wavefronts -- a pipeline's
// split batch runs the first and the second launch apart; SPLIT_BOTH (RMCV_OPT_DENSE_DEFER) runs both.
enum SparseForm { SPARSE_STANDARD = 0, SPARSE_LEAN, SPARSE_SPLIT_FIRST, SPARSE_SPLIT_SECOND, SPARSE_SPLIT_BOTH };
// What a run's launches depend on beyond geometry, buffers and params.  The public entry points take it from the context's options
// (ctx_plan); a pipeline overrides parts of it per batch (batch_plan.h) instead of writing options before a run and undoing them after.
struct RunPlan {
    int pixel_ws;     // RMCV_OPT_PIXEL_SHAPE: whole batches with contiguous rows go to k_binary_ws (one 1024-thread workgroup per CU)
    int pixel_groups; // RMCV_OPT_PIXEL_GROUPS: k_binary's workgroups per CU
    int sparse_waves; // RMCV_OPT_SPARSE_WAVES: wavefronts per frame of the fused sparse kernel
    SparseForm form;  // RMCV_OPT_DENSE_DEFER: SPARSE_SPLIT_BOTH
};
enum SparseKernel { SPARSE_W8, SPARSE_W4, SPARSE_W_LEAN };
// LDS_ONE_PER_CU: at least 84 KB, one workgroup per CU beside k_binary_ws (k_contours_w4.hip)
enum SparseLds { LDS_FRAME, LDS_ONE_PER_CU };
static constexpr size_t LDS_ONE_PER_CU_BYTES = 84 * 1024;
// frame_bytes: lds_bytes(h) of the launcher's OWN translation unit (the lean build's tables are smaller)
constexpr size_t sparse_lds(SparseLds rule, size_t frame_bytes)
{
    return rule == LDS_ONE_PER_CU && frame_bytes < LDS_ONE_PER_CU_BYTES ? LDS_ONE_PER_CU_BYTES : frame_bytes;
}

struct SparseInputs {
    SparseForm form;
    int waves;      // RMCV_OPT_SPARSE_WAVES of a fused run (findContours alone always takes 8)
    bool fused;     // the fit / pairing tail rides in the kernel
    bool classify;  // ... and the icon classifier (no room for its feature rows in the lean build)
    int tier;       // RMCV_OPT_CONTOUR_TIER: 0 per frame, 1 literal scanner, 2 mid tier
    bool mid;       // the mid tier's scratch is there
    bool lean_rows; // h <= CT_MAXH and ww <= 32: the lean build's tables cover the frame
    bool pixel_ws;  // the plan's pixel shape, whether or not k_binary_ws launched
};
// flags: the forced tier (1, 2) | 4 = mark the frames beyond the LDS tables and leave them | 8 = take only the marked frames
struct SparseLaunch { SparseKernel kernel; int flags; SparseLds lds; };
struct SparseLaunches { int n; SparseLaunch l[2]; };

inline SparseLaunches resolve_sparse(const SparseInputs& in)
{
    SparseLaunches r{};
    if (!in.fused || in.waves != 4) {
        r.l[r.n++] = {SPARSE_W8, in.tier, LDS_FRAME};
    } else if (in.form == SPARSE_LEAN && !in.classify && in.tier == 0 && in.mid && in.lean_rows) {
        r.l[r.n++] = {SPARSE_W_LEAN, 2, LDS_FRAME};
    } else {
        const bool split = in.form >= SPARSE_SPLIT_FIRST, defer = split && in.tier == 0 && in.mid;
        if (in.form != SPARSE_SPLIT_SECOND) r.l[r.n++] = {SPARSE_W4, in.tier | (defer ? 4 : 0), in.pixel_ws ? LDS_ONE_PER_CU : LDS_FRAME};
        if (defer && in.form != SPARSE_SPLIT_FIRST) r.l[r.n++] = {SPARSE_W8, 2 | 8, LDS_FRAME}; // (split-second, nothing deferred: no launch)
    }
    return r;
}

} // namespace rmcv
