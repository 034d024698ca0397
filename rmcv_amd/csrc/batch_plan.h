// batch_plan.h -- what the pipelined schedule (rmcv_pipeline.hip) decides, as pure functions of plain values without HIP types, so that a host
// compiler alone can check them (tests/test_batch_plan.py).  The pipeline keeps the queries (hipEventQuery, the contexts' options) and the
// enqueues.  The measurements behind the constants: DESIGN.md 4, "the hot contexts", "a burst's second pixel launch", "dense frames".
#pragma once

#include <stdio.h>

#include <initializer_list>

#include "../../include/rmcv_abi.h"
#include "pixel_plan.h"
#include "sparse_plan.h"

namespace rmcv {

// ---- the configuration: rmcv_pipeline_config against the defaults (rmcv_default_pipeline_config) ----
inline rmcv_pipeline_config default_batch_config()
{
    rmcv_pipeline_config c{}; // armour_cap 0: 8 per frame (record_layout); hot_contexts 0: derived per geometry (hot_for)
    c.depth = 8, c.sparse_streams = 4; // measured by alternating regions of one process (round 3): 8 batches over 4 sparse streams run 4.3-4.5 % ahead of 4 over 2
    c.pixel_streams = 2, c.sparse_waves = 4, c.pixel_groups = 2, c.host_results = 1, c.dense_streams = 4;
    return c;
}
// rc: RMCV_OK, or RMCV_ERR_BAD_ARG for a count beyond what the pipeline holds; hot_cfg: hot_contexts as hot_for reads it
struct BatchConfig { int rc; rmcv_pipeline_config cfg; int hot_cfg; };
inline BatchConfig resolve_config(const rmcv_pipeline_config* cfg /* nullable: the defaults */)
{
    BatchConfig r{RMCV_OK, default_batch_config(), 0};
    rmcv_pipeline_config& d = r.cfg;
    if (cfg) {
        const auto given = [](int32_t v, int32_t& to) { if (v > 0) to = v; };
        given(cfg->depth, d.depth), given(cfg->pixel_streams, d.pixel_streams), given(cfg->sparse_streams, d.sparse_streams);
        given(cfg->armour_cap, d.armour_cap), given(cfg->host_results, d.host_results);
        // alone a batch has the CUs to itself: the latency settings (8 wavefronts per frame, 3 pixel workgroups per CU)
        d.sparse_waves = cfg->sparse_waves > 0 ? cfg->sparse_waves : (d.depth >= 3 ? 4 : 8);
        d.pixel_groups = cfg->pixel_groups > 0 ? cfg->pixel_groups : (d.depth >= 2 ? 2 : 3);
        if (cfg->dense_streams != 0) d.dense_streams = cfg->dense_streams;
        if (cfg->hot_contexts != 0) d.hot_contexts = cfg->hot_contexts;
    }
    if (d.dense_streams < 0 || d.sparse_waves != 4 || d.host_results != 1) d.dense_streams = 0; // (the deferral exists for the 4-wavefront kernel; the policy reads the host mirror)
    if (d.depth > 64 || d.pixel_streams > 16 || d.sparse_streams > 16 || d.dense_streams > 16 || d.host_results > 2) r.rc = RMCV_ERR_BAD_ARG;
    for (int32_t* n : {&d.pixel_streams, &d.sparse_streams, &d.dense_streams}) if (*n > d.depth) *n = d.depth;
    // hot_contexts: 0 = derived from the bound geometry, -1 = off, n = exactly n.  (What came back is read from the records' host mirror; fewer than
    // 3 in rotation stall even sparse batches; the 4-wavefront sparse kernel is the one that fits beside the wave-specialised pixel kernel)
    const int hot_given = cfg ? cfg->hot_contexts : 0;
    if (hot_given > 0 && (hot_given < 3 || hot_given >= d.depth)) d.hot_contexts = -1;
    if (d.depth < 4 || d.host_results != 1 || d.sparse_waves != 4) d.hot_contexts = -1;
    r.hot_cfg = d.hot_contexts < 0 ? -1 : (hot_given > 0 ? hot_given : 0);
    if (d.hot_contexts < 0) d.hot_contexts = 0;
    return r;
}

// ---- the record: [frame_offs: max_frames + 1 | status | report | pad to 16 bytes | armours: armour_cap] ----
// armour_cap: as configured, or 8 per frame; status_word, report_word: int32 indices of the batch's OR-ed status and of the report below
struct RecordLayout { int armour_cap; int64_t head_bytes, record_bytes; int status_word, report_word; };
inline RecordLayout record_layout(int max_frames, int armour_cap)
{
    RecordLayout r{armour_cap > 0 ? armour_cap : 8 * max_frames, (((int64_t)max_frames + 3) * 4 + 15) / 16 * 16, 0, max_frames + 1, max_frames + 2};
    r.record_bytes = r.head_bytes + (int64_t)r.armour_cap * (int64_t)sizeof(rmcv_armour);
    return r;
}
// the report word as k_compact_armours (k_detect.hip) encodes it: frames beyond findContours' LDS tables in bits 0-19, border points per
// frame / 16, capped at 4095, in bits 20-31
struct RecordReport { int dense, points; };
inline RecordReport record_report(uint32_t word) { return {(int)(word & 0xFFFFFu), (int)(word >> 20) * 16}; }

// ---- the hot contexts: how many take turns while the batches are calm -- as many as keep the bit planes of the batches in flight inside the
// 256 MB Infinity Cache (with the planes resident their writes never reach HBM; one context too many and every plane line is a miss).  Budget
// 200 MB of the 256 (frames and byte image stream past it with the nt hint; the sparse kernels' tables want the rest): 256 x 1280x1024 -> 46 MB
// per batch -> 4 (the measured optimum: 4 < 5 << 3, 6); 256 x 1920x1200 -> 79 MB -> 2, below the three a context's reuse needs as slack -> 3
inline int hot_for(int hot_cfg, int depth, int n_frames, int w, int h)
{
    if (hot_cfg != 0) return hot_cfg > 0 ? hot_cfg : 0;
    const int64_t plane = (int64_t)n_frames * (h + 2) * ((w + 63) / 64 + 2) * 8;
    int n = (int)((200ll << 20) / (plane > 0 ? plane : 1));
    if (n < 3) n = 3;
    if (n > depth - 1) n = depth - 1;
    return n;
}
// rmcv_pipeline_set_hot_contexts(n > 0): what it is refused with, or null (n <= 0 switches the rotation off)
inline const char* hot_contexts_refusal(int n, const rmcv_pipeline_config& cfg)
{
    if (n < 3 || n >= cfg.depth) return "hot_contexts: 3 .. depth - 1, or 0 / -1 for off";
    return cfg.host_results != 1 || cfg.sparse_waves != 4 ? "hot_contexts needs host_results = 1 and sparse_waves = 4" : nullptr;
}

// ---- the stream's mood, from the newest record that has come back (lean / frames: of the slot it lives in) ----
// DENSE MODE (round 5): while the records say the batches are heavy -- more than an eighth of the frames beyond findContours' LDS tables, or
// 1 500 border points per frame and more (a plain frame has 650) -- the stream is bound by its sparse stage, and the batches run the LEAN build
// of the sparse kernel (k_contours_lean.hip).  The way back: fewer than 1 200 points per frame -- a dense-mode record says "every frame on the
// mid tier" by construction, so only its points count.  Measured: profiles/r05_dense_mode_ab.txt.  calm: nothing dense at all (one 0.5 ms frame
// per batch in the hot contexts, its own launch or not: 0.424 ms per step against 0.27)
struct Mood { bool heavy, calm; };
inline Mood stream_mood(RecordReport r, bool lean, int frames)
{
    const bool heavy = lean ? r.points >= 1200 : (r.dense * 8 > frames || r.points >= 1500);
    return {heavy, r.dense == 0 && !heavy};
}
// A split batch leaves its dense frames to a second launch on a stream of its own: while the batch that last left the slot had SOME such frames
// but at most an eighth.  A batch without any pays nothing (the second launch costs the plain stream 1-3 %); a batch full of them is better off
// with every frame finished where it is (0.312 against 0.360 ms per step at 233 dense frames of 256)
inline bool split_rule(RecordReport r, int frames) { return r.dense > 0 && r.dense * 8 <= frames; }

// ---- a ticket's slot and streams: a slot always meets the same sparse stream ----
struct TicketPlace { size_t slot, pixel, sparse; };
inline TicketPlace ticket_place(uint64_t t, const rmcv_pipeline_config& cfg)
{
    const size_t k = (size_t)(t % (uint64_t)cfg.depth);
    return {k, (size_t)(t % (uint64_t)cfg.pixel_streams), k % (size_t)cfg.sparse_streams};
}
// which event of the slot a context's last batch lives in the context's next pixel launch waits for: ev_free (behind the sparse stage, the last
// reader of the pixel outputs) if that batch was finished on this batch's sparse stream B -- its compaction reads the armour slots only, and this
// batch's sparse stage, which rewrites them, follows it in stream order --, else ev_done (behind the compaction: 35-95 us later)
inline bool waits_for_free(const void* last_stream, const void* b) { return last_stream == b; }

// ---- the front half of a batch's plan.  fast: one of the hot contexts in turn + k_binary_ws; heavy: dense mode; j: the context of the ring;
// plan: the batch's, from the options of the context it runs in (ctx_plan of ring[j]) ----
struct FrontPlan {
    bool fast, heavy;
    size_t j;
    RunPlan plan(RunPlan of_ctx) const { return {fast ? 1 : 0, of_ctx.pixel_groups, of_ctx.sparse_waves, heavy ? SPARSE_LEAN : of_ctx.form}; }
};
// hot / calm / heavy: the pipeline's state; ws_variant: PIXEL_VARIANTS[pixel_variant(...)].ws of the batch; k: its slot
inline FrontPlan front_plan(int hot, bool calm, bool heavy, const rmcv_pipeline_config& cfg, int stages, bool legacy, bool ws_variant, bool tracked,
                            uint64_t hot_seq, size_t k)
{
    FrontPlan f{};
    // (dense mode needs the records on the host, the 4-wavefront kernel and two pixel streams to make up for the halved launches)
    f.heavy = heavy && cfg.host_results == 1 && cfg.sparse_waves == 4 && !legacy && !(stages & (RMCV_STAGE_IDENTITY | RMCV_STAGE_POSE)) &&
              (stages & RMCV_STAGE_CONTOURS) && (stages & RMCV_STAGE_BLOBS);
    // Out of the hot rotation stay: batches with a classifier stage (round 5, three contexts at 256 x 1920x1200: 0.514 against 0.426 ms per step
    // with them in it); batches whose variant takes the k_binary shape whatever the plan says (pixel_plan.h) -- RMCV_OPT_ENHANCE on the slot's
    // context: the sums pass in front has no use for another batch's planes in the cache; windowed: a geometry of their own, in the rotation they
    // would re-zero the hot contexts' planes; per-frame keys (mosaics take turns as they always have: the format is left out of the question);
    // tracked ones: the step reads the context's lists behind the compaction
    f.fast = hot && calm && !legacy && !(stages & RMCV_STAGE_POSE) && !(stages & RMCV_STAGE_IDENTITY) && ws_variant && !tracked;
    f.j = f.fast ? (size_t)(hot_seq % (uint64_t)hot) : k;
    return f;
}

// ---- the back half.  w8: 8 wavefronts per frame for a batch nothing is launched beside; split: two launches -- `first` on B (frames beyond the
// LDS tables are marked and left alone), `second` on T (those frames only, + the pose stage, which needs every frame's armours); otherwise `first`
// is the only launch's form.  dense_stream: T, the stream the list is finished on -- this dense stream for a split batch, -1 = B ----
struct BackPlan { bool w8, split; int sparse_waves; SparseForm first, second; int dense_stream; };
// latency: nothing will be launched beside the batch; plan: the batch's (FrontPlan::plan); sparse: its stages without the pixel stage's
inline BackPlan back_plan(bool latency, const rmcv_pipeline_config& cfg, bool legacy, const RunPlan& plan, bool split_now, int n_dense, int sparse, size_t k)
{
    const bool heavy = plan.form == SPARSE_LEAN, w8 = latency && cfg.sparse_waves == 4 && !legacy && !heavy;
    const bool split = !w8 && !heavy && split_now && n_dense > 0 && !legacy && (sparse & RMCV_STAGE_CONTOURS) && (sparse & RMCV_STAGE_BLOBS);
    return {w8, split, w8 ? 8 : plan.sparse_waves, split ? SPARSE_SPLIT_FIRST : plan.form, SPARSE_SPLIT_SECOND, split ? (int)(k % (size_t)n_dense) : -1};
}

// ---- the burst hold-back: a burst's SECOND pixel launch is held back (k_delay on its stream) until the first one's workgroups have taken every
// CU -- two launches of k_binary_ws that reach an empty machine together split the CUs and run in lock-step pairs (profiles/r04k_burst_start.txt).
// Only where that reason exists -- the launch WILL be k_binary_ws on every CU (PixelShape::ws_full) -- and for a quarter of the launch's expected
// time (its bytes at 5.5 TB/s), 60 us at most, nothing below 100 us of launch: two 16-frame batches are not held back at all ----
struct HoldBack { bool cold; int hold_us; }; // cold: this launch finds the pixel stream idle, a burst's first
// was_cold: the batch before this one was cold; prev_live / prev_done: ticket t - 1 is still in its slot (false at t == 0) / its list is
// finished (asked only where fast && prev_live); ws_full: asked only where prev_live && !prev_done && was_cold
inline HoldBack hold_back(bool fast, uint64_t t, bool was_cold, bool prev_live, bool prev_done, bool ws_full, int n_frames, int w, int h)
{
    HoldBack r{fast && (t == 0 || (prev_live && prev_done)), 0};
    if (fast && !r.cold && was_cold && prev_live && ws_full) {
        const double launch_us = (double)n_frames * 4.0 * w * h / 5.5e6;
        r.hold_us = launch_us < 100.0 ? 0 : (int)(launch_us / 4.0 < 60.0 ? launch_us / 4.0 : 60.0);
    }
    return r;
}

// ---- what a submit refuses before anything is enqueued, with RMCV_ERR_BAD_ARG: the message, or null ----
// a tracked submit: everything rmcv_batch_track would refuse (w, h: the frames'; packets: serial packets came with the batch)
inline const char* tracked_refusal(int tracker_device, int device, const rmcv_tracker_config& tc, int n_frames, int w, int h, int stages, bool packets,
                                   bool attitude_on)
{
    if (tracker_device != device) return "rmcv_pipeline_submit_tracked: the tracker lives on another device than the pipeline";
    if (n_frames != tc.n_streams) return "rmcv_pipeline_submit_tracked: n_frames differs from the tracker's n_streams (frame f is the next frame of stream f)";
    if (w != tc.frame_w || h != tc.frame_h) return "rmcv_pipeline_submit_tracked: the frame size differs from the tracker's config";
    if (!(stages & RMCV_STAGE_ARMOURS)) return "rmcv_pipeline_submit_tracked: the stages have no RMCV_STAGE_ARMOURS: nothing to track";
    if (packets && !attitude_on) return "rmcv_pipeline_submit_tracked_serial: packets given and the tracker's attitude is off (rmcv_tracker_set_attitude)";
    return nullptr;
}
// the sticky camera table (rmcv_pipeline_set_frame_cameras) of a batch with a pose stage: one index per frame, and every slot's context must
// hold a table of the same size -- the batch runs in whichever slot its ticket gives it.  buf: where the message with the counts is written
inline const char* cameras_refusal(int n_frames, int cam_frames, bool tables_agree, char (&buf)[200])
{
    if (n_frames == cam_frames) return tables_agree ? nullptr : "n_cameras differs between the pipeline's contexts: load the same cameras into EVERY slot (rmcv_pipeline_context, rmcv_pnp_load_cameras)";
    snprintf(buf, sizeof(buf), "the batch has %d frames, the pipeline's camera table %d (rmcv_pipeline_set_frame_cameras)", n_frames, cam_frames);
    return buf;
}

} // namespace rmcv
