// rmcv_internal.h -- shared declarations of the HIP translation units (not part of the ABI): the device buffers, the kernel launchers of
// the k_*.hip units, and what the units behind the ABI (rmcv_host, rmcv_stagewise, rmcv_frame, rmcv_pipeline, rmcv_track, rmcv_tracker,
// rmcv_record, rmcv_gather, rmcv_harvest) need of each other.  Limits and Geom come from bind_plan.h; FrameSource, what the jobs of the
// source view, the corner refinement and the chessboard detector say of SRC(f), and its fillers from frame_source.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <utility>
#include <vector>

#include "../../include/rmcv_abi.h"
#include "bind_plan.h"
#include "calib_plan.h"
#include "chess_plan.h"
#include "corner_plan.h"
#include "device_harvest.h"
#include "device_novelty.h"
#include "frame_source.h"
#include "icon_strip_plan.h"
#include "image_plan.h"
#include "model_plan.h"
#include "pixel_plan.h"
#include "source_view_plan.h"
#include "sparse_plan.h"
#include "svm_plan.h"
#include "tracker_plan.h"

namespace rmcv {

// (Limits and Geom, the geometry of the frames currently bound to a context and of the bit planes derived from them: bind_plan.h)
// (RunPlan, what a run's launches depend on beyond geometry, buffers and params: sparse_plan.h)
static constexpr int CTR_STRIDE = 32;   // ints between the heads of k_binary's strip queues (Bufs::strip_ctr): a 128-byte line each, 9 of them
static constexpr int VISIT_CAP = 4096; // border visits of one frame the contour stage holds in LDS (contours_device.h); more -> mid tier
static constexpr int NN_MID = 1 << 17;   // border visits of one frame the mid tier holds (tables in global memory); more -> literal scanner
static constexpr int CAND_MID = 1 << 15; // outer borders (before RETR_EXTERNAL drops the nested ones) the mid tier holds
// bytes of one frame slot's mid-tier scratch block (layout: contours_device.h, mid_tables)
inline size_t mid_bytes(int slot_cap)
{
    return (size_t)slot_cap * (6 * 8 + 2 * 4) + (size_t)NN_MID * (2 * 8 + 2 * 4) + (size_t)CAND_MID * 4 * 4;
}

// Device buffers of one context (all sized by Limits at creation, reused by every call).
struct Bufs {
    const uint8_t* frames; // BGR input (owned upload buffer or borrowed)
    uint8_t* binary;       // [frame][h][w]          0/255           (imgproc.cpp:74 returns it)
    uint64_t* bits;        // [frame] padded plane F (closed binary as bits)
    int* strip_ctr;        // [8] per-XCD strip queue heads of k_binary + [8] = workgroups of the launch that have drawn their
                           // last strip; the last one to leave zeroes all nine, so every launch starts from 0 with no host mirror
    uint32_t* rowmask;     // [frame][h]  bit k: word k of row y of F is non-zero (rows are h apart; k_binary writes them)
    uint32_t* imgmask;     // [frame][h]  bit k: the 64 bytes of word k of row y in `binary` may be non-zero -- the image's CONTENTS, not the
                           // last run's result; in force while the context's ImageState says so (image_plan.h; k_binary_ws keeps it)
    uint64_t* lab;         // [frame] padded plane: pixel was visited by a border trace
    uint64_t* neg;         // [frame] padded plane: ... and got the negative ("right exit") label
    // contours in DISCOVERY order; cv::findContours returns them reversed (oracle/rmcv_oracle.c)
    rmcv_point* points;    // [frame][max_points]
    int32_t* cont_start;   // [frame][max_contours]
    int32_t* cont_len;     // [frame][max_contours]
    int32_t* n_contours;   // [frame]
    int32_t* n_points;     // [frame]
    uint32_t* visit_xy;    // [frame][VISIT_CAP] scratch of the contour stage: packed (x, y, directions) of every border visit
    uint8_t* mid;          // [frame][mid_stride] scratch of the contour stage's mid tier (contours_device.h: MidTables)
    int64_t mid_stride;
    int mid_slot_cap;      // words per frame the mid tier's per-word tables hold (= every word of the largest frame)
    // light blobs (positive list, in findContours order) and the negative list (contour indices)
    rmcv_lightblob* blobs; // [frame][max_blobs]
    int32_t* blob_src;     // [frame][max_blobs]   contour index (findContours order)
    rmcv_rrect* ellipses;  // [frame][max_blobs]   the fitted ellipse of each positive
    int32_t* elig;         // [frame][max_contours] discovery indices of the contours with >= 6 points (fit work list)
    int32_t* n_elig;       // [frame]
    int32_t* slot_kind;    // [frame][max_contours] per contour: 0 skipped, 1 positive, 2 negative
    rmcv_rrect* slot_ell;  // [frame][max_contours] per contour: fitted ellipse
    int32_t* neg_idx;      // [frame][max_contours]
    int32_t* n_blobs;      // [frame]
    int32_t* n_neg;        // [frame]
    rmcv_armour* armours;  // [frame][max_armours]
    int32_t* n_armours;    // [frame]
    int32_t* status;       // [frame] RMCV_FRAME_* bits
    int32_t* frame_order;  // [frame] the frames in k_binary's completion order, interleaved over the XCDs (SparseSched::order)
    // icon classifier (BASELINE config 5); allocated by rmcv_svm_load
    float* svm_w;          // [n_df][1200]
    double* svm_rho;       // [n_df]
    int32_t* svm_labels;   // [n_class]
    int svm_classes;
    int32_t* identity;     // [frame][max_armours]
    uint8_t* icons;        // [frame][max_armours][1200]  rectified 20x20 BGR icons
    // the model table: what k_classify_models reads.  Entry 0 is the model of svm_w / svm_rho / svm_labels above once more;
    // frame f takes entry frame_model_eff(model_idx[f], svm_models), and while model_idx is null every frame is classified from svm_*
    SvmModelEntry* svm_table;     // [RMCV_SVM_MAX_MODELS]  allocated with svm_w
    int svm_models;               // entries loaded: 1 behind rmcv_svm_load
    const int32_t* model_idx;     // [frame] the raw indices, any value (the context's own copy of host values, or the caller's device memory); null: off
    int32_t* model_eff;           // [frame] the effective indices the last k_classify_models used
    // armour pose; allocated by rmcv_pnp_load
    rmcv_pnp_config* pnp_cfg; //  [1]            rmcv_pnp_load's one camera
    // the camera table: what k_pnp reads.  pnp_cfg with n_cameras = 1 behind rmcv_pnp_load, cam_table behind
    // rmcv_pnp_load_cameras; frame f takes entry frame_camera_eff(cam_req[f], n_cameras), entry 0 while cam_req is null
    rmcv_pnp_config* cam_table;   // [max_frames]  allocated by the first rmcv_pnp_load_cameras
    const rmcv_pnp_config* pnp_cams;
    int n_cameras;
    const int32_t* cam_req;       // [frame] the raw indices, any value (the context's own copy of host values, or the caller's device memory); null: off
    int32_t* cam_eff;             // [frame] the effective indices the last k_pnp with cam_req used
    double* base2gripper;  // [frame][16]  the host's table (rmcv_batch_set_base2gripper)
    double* att_base2gripper; // [frame][16]  the attitude step's table (k_attitude.hip): the matrices of the batch it ran in front of
    const double* pose_base2gripper; // what k_pnp reads: att_base2gripper behind an attitude step, base2gripper from the next binding on
    double* poses;        // [frame][max_armours][9]  rvec | tvec | world position
    // exposure-adaptive detection (RMCV_OPT_ENHANCE; k_enhance.hip): rewritten by every run with the option on, in front of the pixel pass
    uint64_t* enh_sums;    // [frame][3]   exact sums of the B, G, R bytes
    float* enh_gamma;      // [frame]      rm::AutoEnhance's gamma of the frame
    uint8_t* enh_lut;      // [frame][256] rm::CalcGamma's table of that gamma
    uint16_t* enh_m;       // [frame][256] the pixel kernel's threshold table (enhance_math.h: enh_m_entry) for the run's lower bound
    // windowed detection (Geom::win): rewritten by every run that includes the pixel pass, in front of it
    const rmcv_point* win_req; // [frame] the requested origins, any value (the context's own copy of host origins, or the caller's device memory)
    rmcv_point* win_eff;   // [frame]      the effective origins (window_origin_eff): what every consumer of the frames reads
    // per-frame detection keys (Geom::keys): rewritten by every run that includes the pixel pass, in front of it
    const int32_t* key_camps; // [frame] the raw camps, any value (the context's own copy of host values, or the caller's device memory)
    const int32_t* key_lbs;   // [frame] the raw lower bounds, any value; null: the run's rmcv_params::lower_bound for every frame
    FrameKey* key_eff;     // [frame]      the effective keys (frame_key_eff): what the pixel kernel reads
    int32_t* key_enemy;    // [frame]      the raw camp once more: blobs[].target and what pairing compares against (the sparse stage reads it)
};
// the per-frame enemy label of a launch's frames: null without keys (the launch then uses rmcv_params::camp)
inline const int32_t* enemy_table(const Geom& g, const Bufs& b) { return g.keys ? b.key_enemy : nullptr; }

// The effective origin of a window, the one place it is computed: clamped into the frame, x snapped down to a multiple
// of 16 pixels (48 bytes: window rows keep the 16-byte alignment the raw-buffer loader wants).  Part of the semantics, always applied.
__host__ __device__ inline rmcv_point window_origin_eff(rmcv_point req, int frame_w, int frame_h, int win_w, int win_h)
{
    const int xm = frame_w - win_w, ym = frame_h - win_h;
    rmcv_point e;
    e.x = (req.x < 0 ? 0 : (req.x > xm ? xm : req.x)) & ~15;
    e.y = req.y < 0 ? 0 : (req.y > ym ? ym : req.y);
    return e;
}
// (frame_origin_offset, the byte offset of that origin inside frame f: frame_source.h)
// SRC(f) of the batch bound to (g, b), read as the run read it
inline FrameSource frame_source_of(const Geom& g, const Bufs& b) { return frame_source_of(g, b.frames, b.enh_lut, b.win_eff); }

// What pixel_shape (pixel_plan.h) takes of a batch bound to (g, b), as variant `v`, under the run's bound and plan
inline PixelBatch pixel_batch(const Geom& g, const Bufs& b, PixelVariant v, int lower_bound, const RunPlan& plan)
{
    return {v, g.n_frames, g.w, g.h, g.ww, g.stride, g.frame_pitch, g.plane_pitch, g.n_cu, g.pixel_rowquad, (uintptr_t)b.frames % 16 == 0,
            lower_bound, plan.pixel_ws, plan.pixel_groups};
}

// internal value of a frame's status word BETWEEN the two launches of the sparse stage (never seen by a caller: the second launch
// rewrites the word of every frame that carries it)
#define RMCV_FRAME_DEFERRED_ (1 << 30)

// The order in which the sparse kernel's workgroups take frames (Bufs::frame_order): the frames in the order k_binary completes
// them, interleaved over the XCDs the way workgroups are dealt to them -- a frame's planes are then read on the XCD whose L2 they
// were written through.
struct SparseSched {
    const int32_t* order; // [frame] workgroup b -> frame; null: identity
};

static constexpr int MAX_DEVICES = 64; // per-device launch state (hipFuncSetAttribute is per device) is kept in arrays of this size

// Launch a kernel and return the status of THIS launch.  hipLaunchKernelGGL reports errors only through the calling thread's
// sticky last-error slot, which may still hold the error of an unrelated earlier HIP call of the host application (one it
// handled by return code): reading that slot after a launch would turn a launch that ran into a reported failure.
template <typename... P, size_t... I>
inline hipError_t launch_tuple(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, std::tuple<P...>& vals,
                               std::index_sequence<I...>)
{
    void* ptrs[] = {static_cast<void*>(const_cast<typename std::remove_const<P>::type*>(&std::get<I>(vals)))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, s);
}
template <typename... P, typename... A>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... a)
{
    static_assert(sizeof...(P) == sizeof...(A), "argument count differs from the kernel's parameter list");
    std::tuple<P...> vals{static_cast<P>(a)...};
    return launch_tuple(kernel, grid, block, lds, s, vals, std::index_sequence_for<P...>{});
}

int64_t pixel_ws_launches(); // launches of k_binary_ws by this process (rmcv_pixel_ws_launches)
int64_t pixel_image_delta_launches(); // ... of them, those that stored the byte image in delta mode (rmcv_pixel_image_delta_launches)
int64_t pixel_plane_delta_launches(); // ... and of those, the ones that stored the bit plane in delta mode too (rmcv_pixel_plane_delta_launches)
// kernel launchers (each enqueues on `s` and returns the launch error)
hipError_t launch_match(const Geom& g, const Bufs& b, const Limits& lim, const rmcv_params& p, const rmcv_legacy_params& lp,
                        int mode, bool with_frames, bool pairs, hipStream_t s);
// identity: the frame's armours are classified by the same kernel (RMCV_STAGE_IDENTITY; needs pairs)
// lean (nullable): set to whether the lean build ran
hipError_t launch_sparse(const Geom& g, const Bufs& b, const Limits& lim, const rmcv_params& p, bool pairs, bool identity, const RunPlan& plan,
                         hipStream_t s, bool* lean = nullptr);
hipError_t launch_pnp(const Geom& g, const Bufs& b, const Limits& lim, hipStream_t s);
// img: the context's knowledge of its byte image, read for the store mode and rewritten for what this launch leaves (image_plan.h);
// plane: the frames whose bit plane is in step with it (plane_step), likewise
hipError_t launch_binary(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s,
                         ImageState* img, int* plane);
// the pixel stage of a Bayer batch (Geom::input_format != 0; k_binary_bayer.hip); launch_binary hands such batches to it
hipError_t launch_binary_bayer(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, hipStream_t s);
// exposure-adaptive detection (k_enhance.hip, k_binary_enh.hip).  launch_enhance_tables: the channel sums of the frames bound, then every
// frame's gamma, table and threshold table for `lower_bound` (Bufs::enh_*), in front of the pixel pass on the same stream.
hipError_t launch_enhance_tables(const Geom& g, const Bufs& b, int lower_bound, hipStream_t s);
// the pixel stage reading through Bufs::enh_m (Geom::enhance; launch_binary hands such batches to it): k_binary's shape, never k_binary_ws
hipError_t launch_binary_enh(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s);
// windowed detection (k_binary_win.hip).  launch_window_origins: Bufs::win_req -> Bufs::win_eff for the frames bound, in front of the pixel pass
hipError_t launch_window_origins(const Geom& g, const Bufs& b, hipStream_t s);
// the pixel stage of a windowed batch (Geom::win; launch_binary hands such batches to it): k_binary's shape, row-quad or byte-wise loader
hipError_t launch_binary_win(const Geom& g, const Bufs& b, int camp, int lower_bound, int morph, bool image, const RunPlan& plan, hipStream_t s);
// per-frame detection keys (k_binary_camp.hip).  launch_frame_keys: Bufs::key_camps, ::key_lbs (or run_lower_bound) -> Bufs::key_eff, ::key_enemy for
// the frames bound, in front of the pixel pass
hipError_t launch_frame_keys(const Geom& g, const Bufs& b, int run_lower_bound, hipStream_t s);
// the pixel stage of a batch with keys (Geom::keys; launch_binary hands such batches to it): k_binary's shape with the key read per strip, all
// three loaders; with windows too (k_binary_camp_win.hip: row-quad or byte-wise loader); never k_binary_ws
hipError_t launch_binary_camp(const Geom& g, const Bufs& b, int morph, bool image, const RunPlan& plan, hipStream_t s);
hipError_t launch_binary_camp_win(const Geom& g, const Bufs& b, int morph, bool image, const RunPlan& plan, hipStream_t s);
// dst[i] = lut[src[i]] over n16 16-byte vectors of a staged image (rm::CalcGamma); dst == src allowed
hipError_t launch_bytemap(const uint8_t* d_src, uint8_t* d_dst, int64_t n16, const uint8_t* d_lut, int n_cu, hipStream_t s);
// lut[0..255] of `gamma` on the device (the table builder of enhance_math.h)
hipError_t launch_gamma_lut(float gamma, uint8_t* d_lut, hipStream_t s);
// D(m) of one device mosaic into a device BGR frame (rmcv_demosaic)
// lay: the buffer's layout word (device_bayer.h: raw_layout; 0 = a plain 8-bit mosaic) -> D(T(r)) (rmcv_demosaic_raw)
hipError_t launch_demosaic(const uint8_t* d_raw, int stride, int w, int h, int pattern, int lay, uint8_t* d_out, int out_stride, hipStream_t s);
hipError_t launch_contours(const Geom& g, const Bufs& b, const Limits& lim, hipStream_t s);
hipError_t launch_blobs(const Geom& g, const Bufs& b, const Limits& lim, const rmcv_params& p, hipStream_t s);
hipError_t launch_armours(const Geom& g, const Bufs& b, const Limits& lim, const rmcv_params& p, hipStream_t s);
hipError_t launch_blobs_armours(const Geom& g, const Bufs& b, const Limits& lim, const rmcv_params& p, hipStream_t s);
// d_status_or (nullable): TWO words = the OR of the batch's per-frame status words, the number of frames with RMCV_FRAME_MID_PATH; hd_record (nullable, needs d_status_or): the
// record [frame_offs | ... status ... | armours at host_head] once more, in mapped pinned host memory (device address)
hipError_t launch_compact_armours(const Geom& g, const Bufs& b, const Limits& lim, rmcv_armour* d_out, int cap,
                                  int32_t* d_frame_offs, hipStream_t s, int32_t* d_status_or = nullptr, uint8_t* hd_record = nullptr, int host_head = 0);
hipError_t launch_status_clear(const Geom& g, const Bufs& b, int mask, hipStream_t s); // status[f] &= ~mask
hipError_t launch_classify(const Geom& g, const Bufs& b, const Limits& lim, hipStream_t s);
// the classifier of a batch with per-frame models (Geom::models; k_classify_models.hip); launch_classify hands such batches to it
hipError_t launch_classify_models(const Geom& g, const Bufs& b, const Limits& lim, hipStream_t s);
// stage-wise helpers: binary (host-supplied 0/255 image) -> bit plane
hipError_t launch_pack_bits(const Geom& g, const Bufs& b, hipStream_t s);
// contours in findContours order as CSR (for download); d_offs has max_contours+1 entries per frame
// The per-frame chain's results on their way to the host in ONE kernel: up to 8 lists (src on the device, dst in pinned host
// memory mapped into the device's address space) of `count[0] + count_add` elements, clamped to `max_elems`, and up to 12 header
// words.  Nine small device-to-host copies in a row, each a hand-over to the copy engine, cost the chain 40-60 us; the kernel's
// own stores cross PCIe as posted writes.
struct ExportSec {
    const void* src;
    void* dst;
    const int32_t* count; // null: max_elems elements
    int count_add, elem_bytes, max_elems;
};
struct ExportArgs {
    ExportSec sec[8];
    int n_sec;
    const int32_t* hdr_src[12]; // header word i = *hdr_src[i] (null: left alone)
    int32_t* hdr_dst;
};
hipError_t launch_export(const ExportArgs& a, hipStream_t s);
hipError_t launch_pack_contours(const Geom& g, const Bufs& b, const Limits& lim, rmcv_point* d_pts_out, int32_t* d_offs_out,
                                int32_t* d_hdr /* nullable: frame 0's {n_contours, n_points, status} */, hipStream_t s, const ExportArgs* ex = nullptr); // ex: frame 0's workgroup also exports (one-frame chains)
hipError_t launch_gather3(const int32_t* a, const int32_t* b, const int32_t* c, int32_t* d_out, hipStream_t s); // d_out[0..2] = *a, *b, *c

// ---- the operator's debug view (k_view.hip) ----
// Where the lists of the frames to draw are: the batch tables (frame f's rows of Bufs), or -- csr -- ONE frame's lists as the stage-wise
// helper uploads them (the negatives as CSR: neg_offs has n_neg + 1 entries, points holds the contours back to back)
struct ViewLists {
    const rmcv_lightblob* blobs; // [frame][max_blobs]
    const int32_t* n_blobs;      // [frame]
    const rmcv_armour* armours;  // [frame][max_armours]
    const int32_t* n_armours;    // [frame]
    const rmcv_point* points;    // [frame][max_points]
    const int32_t* cont_start;   // [frame][max_contours]  (discovery order; unused with csr)
    const int32_t* cont_len;
    const int32_t* n_contours;   // [frame]
    const int32_t* neg_idx;      // [frame][max_contours]  findContours indices (unused with csr)
    const int32_t* n_neg;        // [frame]
    const int32_t* neg_offs;     // csr only
    int max_blobs, max_armours, max_points, max_contours, csr;
};
// n views of vw x vh: view k is of frame frames[k] (device memory; null: frame k), drawn through overlay planes [n][2][plane_pitch]
struct ViewJob {
    int w, h, prow;              // the frames' extent (a windowed batch: the window's) and their planes' padded row
    int64_t plane_pitch;
    const uint64_t* bits;        // [frame] Bufs::bits
    uint64_t* overlay;
    const int32_t* frames;
    int n, vw, vh, flags;
    uint8_t* out;
    int out_stride;
    int64_t out_pitch;
    ViewLists lists;
};
// k_view_overlay + k_view_resize on `s`; every argument has been checked by the caller
hipError_t launch_view(const ViewJob& j, hipStream_t s);
// the stages a view with `flags` reads the results of
inline int view_stages_needed(int flags)
{
    return RMCV_STAGE_BINARY | ((flags & (RMCV_VIEW_BLOBS | RMCV_VIEW_NEGATIVES)) ? RMCV_STAGE_CONTOURS | RMCV_STAGE_BLOBS : 0) |
           ((flags & RMCV_VIEW_ARMOURS) ? RMCV_STAGE_CONTOURS | RMCV_STAGE_BLOBS | RMCV_STAGE_ARMOURS : 0);
}
// (the view entry points of a context and the stage-wise rmcv_debug_view: rmcv_views.hip)
// what a pipeline needs of them: everything n views need allocated now (blocking); the check of a request against the context's limits;
// and the enqueue itself on frames the caller has bound and run, the frame list already on the device, nothing blocking
int ctx_view_prepare(rmcv_ctx* c, int n);
// (frames: host values; n_frames / stages: the batch the views are of and the stages it has been, or will be, through)
int ctx_view_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int flags, int out_stride, int64_t out_pitch);
int ctx_view_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s);

// ---- the source view (k_view_source.hip): the same views over SRC(f), the BGR image the frame's results are defined on ----
// view: the job k_view_overlay is launched with as it is (w, h: the extent of SRC, a windowed batch's the window's; bits is never read)
struct SourceViewJob {
    ViewJob view;
    FrameSource src;             // (src.w, src.h == view.w, view.h)
};
// k_view_overlay + k_view_source<src.kind> on `s`; every argument has been checked by the caller
hipError_t launch_source_view(const SourceViewJob& j, hipStream_t s);
// (the entry points of a context: rmcv_views.hip; the stage-wise rmcv_source_view: rmcv_stagewise.hip).  What a pipeline needs of them, as
// of the operator's view: the planes come from ctx_view_prepare, the check takes the frames as host values, the enqueue blocks nothing
int ctx_source_view_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int flags, int out_stride, int64_t out_pitch);
int ctx_source_view_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s);

// ---- view labels (k_view_text.hip): text lines and tracker targets over finished views ----
// n views of vw x vh in `out`; view k is of frame frames[k] (device memory; null: frame k) of tables in the geometry (w, h).  Either half
// may be off (armours / tracks null); the tracks are drawn first.
struct LabelJob {
    int n, vw, vh, w, h, scale, n_frames;
    uint8_t* out;
    int out_stride;
    int64_t out_pitch;
    const int32_t* frames;
    // the armours' lines
    const rmcv_armour* armours;  // [frame][max_armours]
    const int32_t* n_armours;    // [frame]
    int max_armours;
    const int32_t* identity;     // [frame][max_armours]; null: -1
    const double* positions;     // armour i of frame f: positions[(f max_armours + i) pos_stride + 0 .. 2]; null: (0, 0, 0)
    int pos_stride;
    // the tracks' quadrilaterals and lines: TrackerBufs' tables (sel null: list 0 is current)
    const rmcv_track* tracks;
    const float* side;
    const int32_t *sel, *n_tracking;
    int n_streams, track_cap;
    const rmcv_point* win_eff;   // [frame] the effective window origins the side records are moved by; null: (x_eff, y_eff) for every frame
    int x_eff, y_eff;
};
// k_view_text on `s`; every argument has been checked by the caller
hipError_t launch_view_text(const LabelJob& j, hipStream_t s);
int64_t view_text_launches(); // launches of k_view_text by this process (rmcv_view_text_launches)
// what the label entry points of a context refuse before anything is enqueued (rmcv_views.hip): the views' list and layout as
// ctx_view_check, the scale, the stages (RMCV_STAGE_ARMOURS), and for tracks (trk non-null) what a tracker step refuses of the batch
// (n_frames / stages: the batch the views are of).  who: the entry point, for the message
int ctx_label_check(rmcv_ctx* c, const char* who, rmcv_tracker* trk, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int scale,
                    int out_stride, int64_t out_pitch);
// the enqueue on frames the caller has bound and run, the frame list already on the device, nothing blocking.  what: RMCV_LABEL_*; with
// RMCV_LABEL_TRACKS the launch is ordered as a step of the tracker's (behind its last one; the next one waits for it)
int ctx_label_enqueue(rmcv_ctx* c, rmcv_tracker* trk, int what, int stages, const int32_t* d_frames, int n, int vw, int vh, int scale, void* d_views,
                      int out_stride, int64_t out_pitch, hipStream_t s);

// ---- the icon strip and the labeler's sheet (k_icon_strip.hip) ----
// n strips of `side` rows of strip_w >= cap * side pixels: strip k holds the icons of frame view_frames[k] (device memory; null: frame k) at
// side x side, slot j at columns [j side, (j + 1) side); slots from the frame's count on and the remainder behind slot cap - 1 are zeros
struct IconStripJob {
    const uint8_t* frames;
    int64_t frame_pitch;
    int stride, w, h, max_armours;
    const rmcv_armour* armours;   // [frame][max_armours], only read
    const int32_t* n_armours;     // [frame]
    const rmcv_point* win_eff;    // null: whole frames
    const int32_t* view_frames;
    int n, side, cap, strip_w;
    uint8_t* out;
    int out_stride;
    int64_t out_pitch;
    int32_t* counts;              // [n] the icons rendered (nullable)
};
// k_icon_strip (BGR frames) on `s`; every argument has been checked by the caller
hipError_t launch_icon_strip(const IconStripJob& j, hipStream_t s);
// the strips of the batch bound to (g, b), by the kernel of the batch's kind
hipError_t launch_icon_strip(const Geom& g, const Bufs& b, const Limits& lim, const int32_t* d_frames, int n, int side, int cap, int strip_w, uint8_t* d_out,
                             int out_stride, int64_t out_pitch, int32_t* d_counts, hipStream_t s);
// the sheet's entry points of a context (rmcv_views.hip) as a pipeline needs them, as of the views: the planes come from ctx_view_prepare, the
// check takes the frames as host values, the enqueue (left pane, right pane, strip) blocks nothing
int ctx_sheet_check(rmcv_ctx* c, const int32_t* frames, int n, int n_frames, int stages, int vw, int vh, int side, int flags, int out_stride, int64_t out_pitch);
int ctx_sheet_enqueue(rmcv_ctx* c, const int32_t* d_frames, int n, int vw, int vh, int side, int flags, void* d_out, int out_stride, int64_t out_pitch, hipStream_t s);

// ---- sub-pixel corner refinement (k_corner.hip, device_corner.h) ----
// per_frame corners of each of n chosen frames, refined in place; SRC(f) is read as the source view reads it
struct CornerJob {
    FrameSource src;
    const int32_t* frames;       // [n] device memory; null: row k is of frame k
    int n, per_frame;
    float* corners;              // [n][per_frame][2]
    const int32_t* counts;       // [n] nullable: corners in row k, clamped to 0 .. per_frame
    int32_t* status;             // [n][per_frame] nullable
    const float* mask;           // [win_h][win_w] device memory (device_corner.h: corner_mask)
    int win_x, win_y, max_iters;
    double eps;
};
// k_corner_subpix<src.kind> on `s`; every argument has been checked by the caller (corner_plan.h)
hipError_t launch_corner(const CornerJob& j, hipStream_t s);

// ---- the chessboard detector (k_chess.hip, device_chess.h) ----
// the board of each of n chosen frames
struct ChessJob {
    FrameSource src;
    const int32_t* frames;       // [n] device memory; null: row k is of frame k
    int n;
    int cols, rows;
    rmcv_chess_params prm;
    uint32_t* lists;             // [n][1 + CHESS_LIST_WORDS] the candidates between the two kernels: count, keys, responses
    float* corners;              // [n][per_frame][2]
    int per_frame;
    int32_t* counts;             // [n]
    int32_t* status;             // [n] nullable
    int32_t* cand;               // [n][RMCV_CHESS_CAND_MAX][3] nullable: the sorted candidates (x, y, R)
    int32_t* cand_n;             // [n] nullable
};
// the count words zeroed, k_chess_response<src.kind>, k_chess_grid<src.kind> on `s`; every argument has been checked by the caller (chess_plan.h)
hipError_t launch_chess(const ChessJob& j, hipStream_t s);

// ---- the calibration solve (k_calib.hip, device_calib.h) ----
struct CalibJob;
// k_calib_homography, k_calib_solve on `s`; every argument has been checked by the caller (calib_plan.h)
hipError_t launch_calib(const CalibJob& j, hipStream_t s);

// ---- the hand-eye solve (k_handeye.hip, device_handeye.h) ----
struct HandEyeJob;
// k_handeye on `s`, one workgroup per camera; every argument has been checked by the caller (handeye_plan.h)
hipError_t launch_handeye(const HandEyeJob& j, hipStream_t s);

// ---- what rmcv_pipeline.hip needs of a context beyond the public ABI (rmcv_host.hip) ----
// external order: the pipeline chains a context's launches with its own events (it knows which stream ran what), so the context
// does not record / wait for its own ordering event around every launch (two HIP calls per launch); rmcv_batch_sync and the getters
// then wait for `done` (recorded by the pipeline behind the slot's last launch) instead
void ctx_external_order(rmcv_ctx* c, hipEvent_t done);
// rmcv_batch_compact_armours + the batch's OR-ed status word
int ctx_compact(rmcv_ctx* c, void* d_armours_out, int cap, void* d_frame_offs, void* d_status_or, hipStream_t s, void* hd_record = nullptr, int host_head = 0);
const Limits& ctx_limits(const rmcv_ctx* c);
// the plan of a run from the context's own options
RunPlan ctx_plan(const rmcv_ctx* c);
// rmcv_batch_run / rmcv_batch_run_legacy (lp non-null) with a plan of the caller's, on frames the caller has bound (ctx_bind_frames);
// lean (nullable): set to whether the sparse stage ran the lean build
int ctx_run(rmcv_ctx* c, const rmcv_params* p, const rmcv_legacy_params* lp, int stages, hipStream_t s, const RunPlan& plan, bool* lean = nullptr);
// rmcv_batch_set_device_frames without a blocking call: a change of geometry (planes zeroed, frame order recomputed) is ENQUEUED on `s`,
// which the caller has made wait for the context's last batch
// d_origins non-null: a windowed batch (rmcv_batch_set_device_windows in the same step: ONE change of geometry, the window's)
// d_camps non-null: per-frame detection keys (rmcv_batch_set_device_frame_camps in the same step; d_lower_bounds nullable)
int ctx_bind_frames(rmcv_ctx* c, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch, hipStream_t s,
                    const void* d_origins = nullptr, int win_w = 0, int win_h = 0, const void* d_camps = nullptr, const void* d_lower_bounds = nullptr);
// what a batch with per-frame keys / for the legacy matcher refuses of a context's options as they are set (pixel_refusal of a Bayer input
// format, RMCV_OPT_ENHANCE), checked without enqueuing anything
int ctx_check_modes(rmcv_ctx* c, bool keys, bool legacy);
// everything binding a full batch would allocate (the mid tier's scratch), now
int ctx_prepare_ring(rmcv_ctx* c);
// the second set of the pixel kernel's outputs (plane, row masks, image, image mask), allocated and zeroed now (blocking; once); then
// ctx_pixel_sets is 2 and ctx_use_pixel_set(c, s) makes set s the one Bufs name -- between batches, by the one thread that owns the context
int ctx_prepare_pixel_sets(rmcv_ctx* c);
int ctx_pixel_sets(const rmcv_ctx* c);
int ctx_pixel_set(const rmcv_ctx* c); // the current one
void ctx_use_pixel_set(rmcv_ctx* c, int s);
// whether binding this extent would enqueue anything (planes zeroed, frame order recomputed: extent_change)
bool ctx_bind_enqueues(const rmcv_ctx* c, int n_frames, int w, int h);
// allocations, host-side synchronisations and blocking copies this context has made while binding geometries
uint64_t ctx_blocking_calls(const rmcv_ctx* c);
int ctx_wait_timeout_ms(const rmcv_ctx* c);
// PixelShape::ws_full of what is bound to the context: the batch will run as one launch of k_binary_ws with a workgroup on every CU
bool pixel_ws_full(const rmcv_ctx* c, int lower_bound, const RunPlan& plan);
// waits that poll with a deadline instead of parking the thread in the runtime: 0 done, 1 deadline passed, -1 HIP error (*err)
int wait_stream_deadline(hipStream_t s, int timeout_ms, hipError_t* err);
int wait_event_deadline(hipEvent_t ev, int timeout_ms, hipError_t* err);
hipError_t launch_delay(unsigned long long ns, hipStream_t s); // holds `s` back for `ns` nanoseconds
// what rmcv_batch_run would refuse for (p, stages) apart from frames not bound, checked without enqueuing anything
int ctx_check_stages(rmcv_ctx* c, const rmcv_params* p, int stages);
// RMCV_OPT_ENHANCE as set on the context
int ctx_enhance(const rmcv_ctx* c);
// entries of the context's camera table (0: nothing loaded)
int ctx_n_cameras(const rmcv_ctx* c);
// rmcv_batch_set_device_frame_cameras on what ctx_bind_frames has just bound: nothing is enqueued, nothing blocks
void ctx_set_frame_cameras(rmcv_ctx* c, const void* d_idx);
// entries of the context's model table (0: nothing loaded)
int ctx_n_models(const rmcv_ctx* c);
// rmcv_batch_set_device_frame_models on what ctx_bind_frames has just bound: nothing is enqueued, nothing blocks
void ctx_set_frame_models(rmcv_ctx* c, const void* d_idx);
// the pixel kernel variant of the frames bound last (what the runs on them launch)
PixelVariant ctx_pixel_variant(const rmcv_ctx* c);


// ---- device-resident tracker (k_track.hip, rmcv_tracker.hip) ----
// (TrackerBufs, the device state of a tracker, and TrackerView, what is read of one outside rmcv_tracker.hip: tracker_plan.h)
// one step for the n_streams frames of the batch in `b`; identity / pose: the run included those stages; win_eff: null without windows
hipError_t launch_track(const rmcv_tracker_config& cfg, const TrackerBufs& tb, const Bufs& b, const Limits& lim, bool identity, bool pose,
                        const rmcv_point* win_eff, int64_t timestamp, hipStream_t s);
// rmcv_batch_track with the stages given (a pipeline runs a batch's halves separately: the context's record of its last run is not the batch's)
// loop (nullable): the recorder's loop records of this batch (k_loop.hip) go behind the aim step, in front of the tracker's event
struct LoopTicket;
int ctx_track(rmcv_ctx* c, rmcv_tracker* trk, int64_t timestamp, int stages, hipStream_t s, const LoopTicket* loop = nullptr);
// what a caller outside rmcv_tracker.hip has of the object: the view of its state as it stands (tracker_plan.h: tracker_view_of; kept in the
// tracker and refreshed by its setters: valid until the next rmcv_tracker_* call on it) ...
const TrackerView& tracker_view(const rmcv_tracker* t);
// ... and the order of a step on `s`: wait (on the GPU) for the tracker's last step if that ran on another stream -- a consumer of its
// origins on another stream does the same --; afterwards record it
hipError_t tracker_order_begin(rmcv_tracker* t, hipStream_t s);
hipError_t tracker_order_end(rmcv_tracker* t, hipStream_t s);

// ---- device-resident aiming (k_aim.hip) ----
// aiming on (TrackerView::aim_on): the aim step of every stream right behind a tracker step (ctx_track), `now` = the step's timestamp
hipError_t launch_aim(const TrackerView& v, int64_t now, hipStream_t s);

// ---- per-stream gimbal attitude (k_attitude.hip) ----
// attitude on (TrackerView::att_on): the attitude step of every stream in front of a tracked batch, on its pixel stream
// d_packets (nullable): n_streams x 24 bytes; d_base2gripper (nullable): the batch context's [n_streams][16]
hipError_t launch_attitude(const TrackerView& v, const void* d_packets, double* d_base2gripper, hipStream_t s);
// rmcv_batch_attitude on `s` (every check before the first enqueue; never synchronises): behind the tracker's previous step, recorded as its newest
int ctx_attitude(rmcv_ctx* c, rmcv_tracker* trk, const void* d_packets, hipStream_t s);

// ---- the session recorder's frame packer (k_pack.hip) ----
static constexpr int PACK_MAX_FRAMES = 64; // frames of one pack job (their indices travel as a kernel argument)
struct PackIdx { int32_t f[PACK_MAX_FRAMES]; };
// n planes of h rows of w_bytes bytes -> n packed frames, out_pitch apart (device_pack.h: the format), their sizes in sizes[n].
// Plane k is frame idx.f[k] of `frames` when use_idx, frame k otherwise.  keys_out / origins_out (nullable): the batch's effective
// detection keys / window origins of those frames, copied alongside by the same launches.
struct PackJob {
    const uint8_t* frames;
    int64_t pitch;
    int stride, w_bytes, h, lag, n;
    uint8_t* out;
    int64_t out_pitch;
    int64_t* sizes;
    int use_idx;
    PackIdx idx;
    const FrameKey* key_eff;
    int32_t* keys_out;        // [n][4]
    const int32_t* key_enemy; // the raw camps, with key_eff
    int32_t* camps_out;       // [n]
    const rmcv_point* win_eff;
    rmcv_point* origins_out;  // [n]
};
// k_pack_widths + k_pack_scan + k_pack_emit on `s`; every argument has been checked by the caller (pack_job_refusal)
hipError_t launch_pack(const PackJob& j, hipStream_t s);
// n packed frames, in_pitch apart -> n planes; a frame whose header or row table points outside its in_pitch bytes is left unfinished, never read past
hipError_t launch_unpack(const uint8_t* packed, int64_t in_pitch, int n, int w_bytes, int h, int lag, uint8_t* frames, int stride, int64_t pitch, hipStream_t s);
// why the kernels cannot take this geometry and these buffers (null: they can)
const char* pack_job_refusal(const void* frames, int n, int w_bytes, int h, int stride, int64_t pitch, int lag, const void* packed, int64_t packed_pitch);

// ---- the session recorder (rmcv_record.hip) as the pipeline drives it ----
// what a pipeline knows of a batch at its submit; everything else is the recorder's
struct RecordBatch {
    const void* d_frames;
    int w, h, stride;          // the frames as bound (pixels; bytes between rows)
    int w_bytes, lag;          // bytes of a row, and the distance to the previous sample of the same kind (device_pack.h: pack_lag)
    int64_t pitch;
    int batch_frames;
    int input_format, sample_bits, valid_bit, orient;
    int stages, win_w, win_h;
    rmcv_params params;
    int64_t timestamp;
    uint64_t ticket;
    const FrameKey* key_eff;   // device; null: per-run keys
    const int32_t* key_enemy;  // device, with key_eff: the raw camps
    const rmcv_point* win_eff; // device; null: whole frames
    const rmcv_tracker* trk;   // a tracked submit's tracker: with the recorder's track_cap > 0 the batch gets loop records; null: none
};
// why the recorder cannot take `n` chosen frames of this geometry (null: it can); nothing is enqueued
const char* recorder_refusal(const rmcv_recorder* r, int device, int n, int w_bytes, int h);
// pack frames[0 .. n) of the batch into the recorder's next slot on `s`: launches and event calls only, nothing blocks.  Frozen: nothing happens.
// loop (nullable): set to where the batch's loop records go (LoopTicket::rec null: the batch gets none)
int recorder_enqueue(rmcv_recorder* r, const RecordBatch& b, const int32_t* frames, int n, hipStream_t s, LoopTicket* loop = nullptr);
// the frames bound to a context as the recorder describes them: format, row bytes, lag, the effective key / origin tables (rmcv_host.hip)
void ctx_record_batch(const rmcv_ctx* c, RecordBatch* b);
// bytes of one pixel of the frames the context's options describe (what the next binding will record)
int ctx_frame_pixel_bytes(const rmcv_ctx* c);

// ---- the recorder's loop records (k_loop.hip, rmcv_record.hip) ----
// the latch record as the device writes it, in device memory and in the mapped host copy; `set` last
struct LoopLatch {
    uint32_t fired;    // fired & mask of the record that took the latch
    int32_t k, stream;
    int32_t set;       // 1 once the fields above are written
    uint64_t sequence;
};
// what a pipeline keeps of a recorded tracked batch between its submit (the slot is chosen there) and the call that enqueues its step
struct LoopTicket {
    rmcv_recorder* rec = nullptr; // null: the batch gets no loop records
    int slot = 0;
    uint64_t sequence = 0;
    const void* d_packets = nullptr; // the batch's serial packets (device; nullable)
};
// one launch of k_loop_record: everything by value
struct LoopArgs {
    int n, rec_cap, n_streams, trk_cap; // chosen frames; the recorder's and the tracker's track_cap
    PackIdx idx;                        // [n] the chosen frames = streams
    uint8_t* out;                       // [n] areas, `pitch` apart
    const uint8_t* prev;                // the previous slot's areas, or null: nothing is compared
    int64_t pitch;
    TrackerBufs tb;
    const rmcv_aim* aims;               // null: aiming was never on
    const rmcv_aim_input* aim_inputs;   // null: the defaults
    const rmcv_aim_config* aim_cfgs;    // null: aim_cfg for every stream
    const rmcv_attitude* attitudes;
    const int32_t* packet_errors;
    const double* stream_g2c;           // null: att_cfg's for every stream
    const uint8_t* packets;             // null: none
    const int32_t *n_armours, *frame_status; // the batch context's
    const rmcv_point* win_eff;          // null: whole frames
    const FrameKey* key_eff;            // null: per-run keys
    const int32_t* cam_eff;             // null: no camera table in use
    int has_aim, has_att, has_camps;
    rmcv_tracker_config tcfg;
    rmcv_aim_config aim_cfg;
    rmcv_attitude_config att_cfg;
    int64_t timestamp;
    uint64_t sequence;
    rmcv_trigger_config trig;           // (mask 0: nothing takes the latch)
    uint32_t* latch_word;               // device; 0: free
    LoopLatch *d_latch, *hd_latch;      // device memory; the mapped host copy's device address
};
hipError_t launch_loop_record(const LoopArgs& a, hipStream_t s);
// fill in the recorder's part of `a` for the ticket's batch (areas, predecessor, trigger, latch), make `s` wait for what still uses the
// slot's areas: event calls only.  trk: the tracker whose step this is.  RMCV_OK, or the recorder's error
int recorder_loop_begin(const LoopTicket& t, const rmcv_tracker* trk, LoopArgs* a, hipStream_t s);
// behind the launch: the slot's second event
int recorder_loop_end(const LoopTicket& t, hipStream_t s);
// why a pipeline of `depth` slots cannot take this recorder's armed triggers (null: it can)
const char* recorder_trigger_refusal(const rmcv_recorder* r, int depth);

// ---- the icon classifier's trainer (k_svm.hip) ----
// int32 [n][n] of u8 [n][1200]
hipError_t launch_svm_gram(const uint8_t* d_samples, int n, int32_t* d_gram, hipStream_t s);
// k_svm_smo + k_svm_weights over d.problems[0 .. n_problems): alphas, rho, outs, weights [n_problems][1200]; between (nullable): recorded between the two
hipError_t launch_svm_solve(const SvmDevice& d, int n_problems, double eps, int max_iter, hipStream_t s, hipEvent_t between = nullptr);
// d_out[m * n + r], m < n_models: row r under model m * k_fold + d_fold_of[r] (d_fold_of null: model 0); d_labels null: class indices
hipError_t launch_svm_predict(const uint8_t* d_samples, int n, const float* d_weights, const double* d_rho, int n_class, const int32_t* d_fold_of, int k_fold,
                              int n_models, const int32_t* d_labels, int32_t* d_out, hipStream_t s);
// rmcv_svm_train / rmcv_svm_predict behind their pointer checks (rmcv_svm.hip).  d_samples non-null: the rows are on the device already
// (rmcv_svm_train_dataset: the upload is skipped, `samples` is not read); null: `samples` (host) is uploaded
int svm_train_rows(rmcv_ctx* c, const uint8_t* d_samples, const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm,
                   const rmcv_svm_train_params* params, float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out,
                   rmcv_svm_train_report* report);
// model: an entry of the context's model table (its caller has checked it); -1: the single model's buffers, which hold entry 0
int svm_predict_rows(rmcv_ctx* c, const uint8_t* d_samples, const uint8_t* samples, int n, int32_t* identity_out, int model = -1);

// ---- the dataset harvest (k_harvest.hip, rmcv_harvest.hip) ----
// what is read of a dataset outside rmcv_harvest.hip, the one unit that knows struct rmcv_dataset
struct DatasetView {
    int device;
    int32_t capacity;
    uint8_t* rows;           // [capacity][1200]
    rmcv_harvest_meta* meta; // [capacity]
    HarvestCounters* ctr;    // count, the last append's list length, dropped
    HarvestItem* list;       // [capacity] the work list of the append in flight (appends are ordered: one at a time)
    int32_t* labels;         // [label_cap] the host labels of the append in flight (rmcv_batch_harvest copies them here)
    int label_cap;
    // novelty (device_novelty.h); the pointers are null until rmcv_dataset_set_novelty has turned it on once
    int ring_rows;           // 0: off
    int32_t max_sad;
    uint8_t* rings;          // [label_cap][ring_rows][1200]
    int64_t* pushed;         // [label_cap]
    unsigned long long* near;
    uint8_t* keep;           // [label_cap][keep_armours] the keep bytes of the append in flight
    int keep_armours;        // the creating context's max_armours
};
// the rows rmcv_dataset_append_rows has staged on the device
struct DatasetRowsSource {
    const uint8_t* rows;     // [sum n_rows][1200]
    const int32_t* n_rows;   // [n_streams]
    const int32_t* row_off;  // [n_streams] exclusive sums of n_rows
    const int32_t* zeros;    // [n_streams] (the status words of k_harvest_plan)
    const int32_t* labels;   // [n_streams]
    int n_streams, max_armours;
};
const DatasetView& dataset_view(const rmcv_dataset* ds);
// the order of an append on `s`: wait (on the GPU) for the dataset's last append if that ran on another stream; afterwards record it
hipError_t dataset_order_begin(rmcv_dataset* ds, hipStream_t s);
hipError_t dataset_order_end(rmcv_dataset* ds, hipStream_t s);
// k_harvest_plan + k_harvest_rows on `s`; identity: the batch's run included RMCV_STAGE_IDENTITY.  Every argument has been checked by the caller.
hipError_t launch_harvest(const Geom& g, const Bufs& b, const Limits& lim, const DatasetView& d, const int32_t* d_labels, int flags, bool identity,
                          uint64_t tag, hipStream_t s);
// d_out [n][1200] (nullable), d_responses [n] (nullable) of slots d_idx[0 .. n) (null: 0 .. n - 1)
// k_harvest_plan alone over any per-frame tables (device); with d.ring_rows > 0 its second instantiation, which takes d.keep in
hipError_t launch_harvest_plan(const int32_t* n_armours, const int32_t* status, const int32_t* d_labels, const int32_t* ident, int n_frames, int max_armours,
                               int flags, const DatasetView& d, hipStream_t s);
hipError_t launch_harvest_plan_novel(const int32_t* n_armours, const int32_t* status, const int32_t* d_labels, const int32_t* ident, int n_frames, int max_armours,
                                     int flags, const DatasetView& d, hipStream_t s); // (k_novelty.hip)
// the same for rows from memory (rmcv_dataset_append_rows): the plan, then a copy of 75 uint4 per kept row
hipError_t launch_harvest_rows_source(const DatasetRowsSource& src, const DatasetView& d, int n_cu, uint64_t tag, hipStream_t s);
// k_harvest_novel (k_novelty.hip) in front of the plan, novelty on: the keep bytes, rings, pushed and near of one append.  src null: the bound batch
hipError_t launch_harvest_novel(const Geom& g, const Bufs& b, const Limits& lim, const DatasetRowsSource* src, const DatasetView& d, const int32_t* d_labels,
                                int flags, const int32_t* ident, hipStream_t s);
hipError_t launch_harvest_gather(const DatasetView& d, const int32_t* d_idx, int n, uint8_t* d_out, int32_t* d_responses, hipStream_t s);
// rmcv_batch_harvest_device with the stages given (a pipeline runs a batch's halves separately), on `s` (rmcv_host.hip): every check before the
// first enqueue.  d_labels: n_labels entries (a batch with more frames is refused), launches and event calls only; or h_labels (host, one per
// frame bound): copied into the dataset's own table on `s`, behind its previous append
int ctx_harvest(rmcv_ctx* c, rmcv_dataset* ds, const int32_t* h_labels, const void* d_labels, int n_labels, int flags, uint64_t tag, int stages, hipStream_t s);
// ... and what it would refuse, checked without enqueuing anything (a pipeline's submit asks before its first enqueue)
// max_armours: the appending context's limit (a dataset with novelty on has one ring per stream and keep bytes for its creator's limits)
const char* ctx_harvest_refusal(int device, int n_frames, bool frames_bound, const rmcv_dataset* ds, int n_labels, int flags, int stages, int max_armours);

} // namespace rmcv
