// bind_plan.h -- what a batch context decides on the host: what a binding refuses and records (Geom), when its planes are re-zeroed and
// its frame order recomputed, the device layout of an upload, what a stage mask refuses, which launches a run makes, and the values
// rmcv_ctx_set_option takes.  Pure functions of plain values, without HIP types, so that a host compiler alone can check them
// (tests/test_bind_plan.py); rmcv_host.hip makes the HIP calls they decide on.
#pragma once

#include <limits.h>
#include <stdint.h>

#include <cmath>

#include "../../include/rmcv_abi.h"
#include "pixel_plan.h"

namespace rmcv {

struct Limits {
    int max_frames, max_width, max_height, max_contours, max_points, max_blobs, max_armours;
};

// Geometry of the frames currently bound to a context and of the bit planes derived from them.
// Bit planes (foreground F, "labelled" LAB, "right-exit" NEG) hold one bit per pixel in u64 words,
// bit b of word k = pixel x = 64*k + b.  Each plane is padded with one zero word left and right of
// every row and one zero row above and below the image, so a 3x3 neighbourhood never needs a
// bounds check:  word(y, k) lives at (y + 1) * prow + (k + 1).
struct Geom {
    int device;          // HIP device of the owning context: per-device launch state (function attributes) is indexed by it
    int n_cu;            // compute units of that device (sizes the persistent grid of k_binary)
    int pixel_halo_nt;   // RMCV_OPT_PIXEL_HALO_NT: the row quads a strip shares with its neighbours are loaded non-temporal too
    int pixel_rowquad;   // hidden option 1001 (bench.py's RMCV_BENCH_AB): k_binary's row-quad loader even where rows are contiguous
    int overloads;       // RMCV_OPT_OVERLOADS: SURVEY A.6, which functions the reference's unqualified abs / atan2 / sin / cos on floats are
    int contour_tier;    // RMCV_OPT_CONTOUR_TIER: 0 = per frame (LDS tables, else mid tier, else literal scanner), 1 = literal, 2 = mid tier
    int input_format;    // RMCV_OPT_INPUT_FORMAT of the frames bound: 0 BGR, 1..4 a Bayer pattern (recorded when the frames are bound)
    int sample_bytes;    // RMCV_OPT_INPUT_SAMPLE_BITS of the frames bound, as bytes: 1, or 2 (16-bit Bayer samples; BGR: always 1)
    int valid_bit;       // RMCV_OPT_INPUT_VALID_BIT: the pixel is bits valid_bit .. valid_bit + 7 of a 2-byte sample
    int orient;          // RMCV_OPT_INPUT_ORIENT: RMCV_ORIENT_MIRROR | RMCV_ORIENT_FLIP of the frames bound
    int n_frames;
    int w, h;
    int stride;          // bytes between rows of the input (BGR or mosaic)
    int64_t frame_pitch; // bytes between frames of the input
    int ww;              // words per row = ceil(w / 64)
    int prow;            // padded words per row = ww + 2
    int64_t plane_pitch; // words per frame = (h + 2) * prow
    int enhance;         // RMCV_OPT_ENHANCE of the frames bound: the pixel pass and the classifier read every byte through the frame's gamma table
    float enh_max_gain, enh_min_gain; // rmcv_ctx_set_enhance_gains, recorded with it
    // windowed detection (rmcv_batch_set_windows): w, h, ww, prow, plane_pitch above are the WINDOW's -- everything behind the pixel pass
    // sees a batch of win_w x win_h images -- while stride and frame_pitch stay the frames'; the frames' own extent is kept here
    int win;             // 1: every frame is read at its effective origin (Bufs::win_eff)
    int frame_w, frame_h; // the frames as bound (== w, h without windows)
    // per-frame detection keys (rmcv_batch_set_frame_camps): camp and lower bound of every frame come from Bufs::key_eff / key_enemy, which every
    // run with the pixel pass rewrites in front of it; rmcv_params::camp and ::lower_bound are then not read
    int keys;
    // per-frame icon models (rmcv_batch_set_frame_models): every frame is classified with its own entry of the context's model
    // table (Bufs::model_idx), by k_classify_models; 0: entry 0 for every frame, the single-model kernels
    int models;
};
// bytes of one pixel of the frames a geometry describes: 3 (BGR), or the Bayer sample's 1 or 2
inline int geom_pixel_bytes(const Geom& g) { return g.input_format ? g.sample_bytes : 3; }

// What a binding records of the context's options (frames bound before keep what they were bound with)
struct InputOptions {
    int format = 0;       // RMCV_OPT_INPUT_FORMAT: 0 BGR, 1..4 a Bayer pattern (Geom::input_format)
    int sample_bits = 8;  // RMCV_OPT_INPUT_SAMPLE_BITS: 8 or 16   } the Bayer frame as the sensor delivers it (Geom::sample_bytes,
    int valid_bit = 0;    // RMCV_OPT_INPUT_VALID_BIT: 0 .. 4      } valid_bit, orient)
    int orient = 0;       // RMCV_OPT_INPUT_ORIENT: RMCV_ORIENT_*  }
    int enhance = 0;      // RMCV_OPT_ENHANCE: frames are read through their rm::AutoEnhance table (Geom::enhance)
    float max_gain = 100.0f, min_gain = 50.0f; // rmcv_ctx_set_enhance_gains (include/imgproc.h:35)
    // bytes of one sample of what the options describe: 3 per BGR pixel, 1 or 2 per Bayer sample
    int pixel_bytes() const { return format ? sample_bits / 8 : 3; }
};

// the gains rm::AutoEnhance can divide by (rmcv_ctx_set_enhance_gains, rmcv_enhance_gamma, rmcv_auto_enhance)
inline bool gains_ok(float max_gain, float min_gain) { return std::isfinite(max_gain) && std::isfinite(min_gain) && max_gain != min_gain; }

// a refusal: the ABI's code and the message rmcv_last_error gives; code RMCV_OK: none
struct Refusal {
    int code;
    const char* why;
    explicit operator bool() const { return code != RMCV_OK; }
};
inline Refusal bad_arg(const char* why) { return {why ? RMCV_ERR_BAD_ARG : RMCV_OK, why}; }

// BGR frames have no sample size and no orientation of their own: a context left at 16 bits or mirrored / flipped would read them wrongly
inline const char* layout_refusal(const InputOptions& in)
{
    if (in.format != RMCV_INPUT_BGR) return nullptr;
    if (in.sample_bits != 8) return "a BGR frame with RMCV_OPT_INPUT_SAMPLE_BITS = 16: the option is for Bayer frames (RMCV_OPT_INPUT_FORMAT)";
    if (in.orient != 0) return "a BGR frame with RMCV_OPT_INPUT_ORIENT set: the option is for Bayer frames (RMCV_OPT_INPUT_FORMAT)";
    return nullptr;
}

// what windows of win_w x win_h refuse (fw x fh: the frames; fmt / enh: what they are read as)
inline const char* windows_refusal(const Limits& lim, int fw, int fh, int fmt, int enh, int win_w, int win_h)
{
    if (const char* why = pixel_refusal(fmt, enh, true, false, false)) return why;
    if (win_w < 1 || win_h < 1) return "window size out of range: win_w and win_h must be at least 1";
    if (win_w > fw || win_h > fh) return "window size out of range: larger than the frames";
    if (win_w > lim.max_width || win_h > lim.max_height) return "window size out of range: larger than the context's limits";
    return nullptr;
}

// what a binding of n_frames frames of w x h refuses, checked before anything of the context moves; win_w > 0: read through win_w x win_h windows
inline Refusal binding_refusal(const Limits& lim, const InputOptions& in, int n_frames, int w, int h, int stride, int64_t frame_pitch, int win_w, int win_h)
{
    if (n_frames < 1 || n_frames > lim.max_frames) return bad_arg("n_frames out of range");
    if (w < 1 || h < 1 || w > lim.max_width || h > lim.max_height) return bad_arg("frame size out of range");
    if (const char* why = layout_refusal(in)) return bad_arg(why);
    const int bpp = in.pixel_bytes();
    if (in.format && (w < 3 || h < 3)) return bad_arg("a Bayer frame needs w >= 3 and h >= 3");
    if (stride < bpp * w || frame_pitch < (int64_t)stride * (h - 1) + bpp * w) return bad_arg("bad stride/pitch");
    if (bpp == 2 && ((stride & 1) || (frame_pitch & 1))) return bad_arg("16-bit samples (RMCV_OPT_INPUT_SAMPLE_BITS): stride and frame_pitch are bytes and must be even");
    if (const char* why = pixel_refusal(in.format, in.enhance, false, false, false)) return bad_arg(why);
    if (win_w > 0) return bad_arg(windows_refusal(lim, w, h, in.format, in.enhance, win_w, win_h));
    return bad_arg(nullptr);
}

// Make w x h the extent everything behind the frame loads sees (the frames' own, or their windows')
inline void extent_fields(Geom& g, int w, int h)
{
    g.w = w;
    g.h = h;
    g.ww = (w + 63) / 64;
    g.prow = g.ww + 2;
    g.plane_pitch = (int64_t)(h + 2) * g.prow;
}

// The fields of a binding binding_refusal has passed.  A new binding returns to per-run keys (Geom::keys), as it returns to whole frames.
inline void bind_geom(Geom& g, const InputOptions& in, int n_frames, int w, int h, int stride, int64_t frame_pitch, int win_w, int win_h)
{
    g.enhance = in.enhance;
    g.enh_max_gain = in.max_gain;
    g.enh_min_gain = in.min_gain;
    g.input_format = in.format;
    g.sample_bytes = in.format ? in.sample_bits / 8 : 1;
    g.valid_bit = g.sample_bytes == 2 ? in.valid_bit : 0;
    g.orient = in.format ? in.orient : 0;
    g.n_frames = n_frames;
    g.stride = stride;
    g.frame_pitch = frame_pitch;
    g.frame_w = w;
    g.frame_h = h;
    g.win = win_w > 0;
    g.keys = 0;
    g.models = 0;
    extent_fields(g, g.win ? win_w : w, g.win ? win_h : h);
}

// What a change of extent costs: the padded planes are zeroed when (w, h) differs from what they were zeroed for (their pads must read
// 0), the frame order is recomputed when (n_frames, h) differs from what it was computed for.
struct ExtentChange { bool planes, order; };
inline ExtentChange extent_change(int geom_w, int geom_h, int order_n, int order_h, int w, int h, int n_frames)
{
    return {geom_w != w || geom_h != h, order_n != n_frames || order_h != h};
}

// The device layout of rmcv_batch_upload: tightly packed rows (3 w bytes -- w or 2 w for a mosaic -- rounded up to 16), frames back to back
struct UploadLayout {
    int bpp, row_bytes, h;
    int stride;    // device bytes between rows
    int64_t pitch; // device bytes between frames
    // what the upload refuses of the HOST's stride and pitch before the binding is checked (a BGR frame's are left to the copy)
    const char* refusal(int host_stride, int64_t host_pitch) const
    {
        if (bpp != 3 && (host_stride < row_bytes || host_pitch < (int64_t)host_stride * (h - 1) + row_bytes)) return "bad stride/pitch";
        if (bpp == 2 && ((host_stride & 1) || (host_pitch & 1))) return "16-bit samples (RMCV_OPT_INPUT_SAMPLE_BITS): stride and frame_pitch are bytes and must be even";
        return nullptr;
    }
    // the host's frames lie as the device's do: one copy for the batch
    bool same(int host_stride, int64_t host_pitch) const { return host_stride == stride && host_pitch == pitch; }
};
inline UploadLayout upload_layout(int bpp, int w, int h)
{
    const int rowb = bpp * w, dstride = (rowb + 15) & ~15;
    return {bpp, rowb, h, dstride, (int64_t)dstride * h};
}

// what a run refuses of its parameters and stage mask, whatever is bound
inline const char* stage_refusal(const rmcv_params* p, int stages, bool have_svm, bool have_pnp)
{
    if (!p) return "null params";
    if (p->morph < RMCV_MORPH_NONE || p->morph > RMCV_MORPH_CLOSE) return "bad morph";
    if (stages <= 0 || stages > (RMCV_STAGE_ALL | RMCV_STAGE_IDENTITY | RMCV_STAGE_POSE | RMCV_STAGE_NO_IMAGE)) return "bad stage mask";
    if ((stages & RMCV_STAGE_IDENTITY) && !have_svm) return "RMCV_STAGE_IDENTITY needs rmcv_svm_load first";
    if ((stages & RMCV_STAGE_POSE) && !have_pnp) return "RMCV_STAGE_POSE needs rmcv_pnp_load first";
    return nullptr;
}

// ---- what a run enqueues, in the order of the fields ----
struct RunSteps {
    const char* refusal;  // the legacy matcher against what is bound (pixel_refusal), before the first enqueue
    // Status bits belong to the stage that sets them: k_contours rewrites the whole word; a run that starts at a later stage
    // clears only the bits of the stages it runs, so OVF_CONTOURS / OVF_POINTS / SLOW_PATH of the contour run it builds on survive.
    int status_clear;     // the bits k_status_clear takes; 0: no launch
    // in front of the pixel pass, at RUN time (borrowed frames and tables may have changed since they were bound):
    //   RMCV_OPT_ENHANCE: every frame's sums, gamma and tables; windows: the effective origins (the requests may be a tracker's, rewritten
    //   on the device since they were set); per-frame keys: the effective keys (lower_bounds null: this run's bound)
    bool enhance_tables, window_origins, frame_keys;
    bool binary, image;   // the pixel pass; with the 0/255 byte image
    // findContours + filter_lightblobs (+ filter_armours) as ONE per-frame kernel when the stages are asked for together; the per-stage
    // events of rmcv_batch_run_timed need per-stage launches.  The icon classifier rides in it when the armours come from it (not for
    // mosaics: its classifier reads BGR; nor through a gamma table or windows: k_classify takes those; nor with per-frame models: the
    // fused classifier is never given a table, k_classify_models takes every such batch)
    bool sparse, sparse_pairs, sparse_identity, contours;
    bool match, match_pairs, blobs_armours, blobs; // the legacy matcher (+ pairing in the same launch); fit and pairing in one launch; the fit alone
    bool armours, classify, pnp;
};
inline RunSteps run_steps(int stages, bool timed, bool legacy, int input_format, int enhance, int win, int keys, int models = 0)
{
    const auto has = [stages](int s) { return (stages & s) != 0; };
    RunSteps r{};
    r.refusal = legacy ? pixel_refusal(input_format, enhance, false, keys != 0, true) : nullptr;
    if (!has(RMCV_STAGE_CONTOURS))
        r.status_clear = (has(RMCV_STAGE_BLOBS) ? (RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_HULL) : 0) | (has(RMCV_STAGE_ARMOURS) ? RMCV_FRAME_OVF_ARMOURS : 0);
    r.binary = has(RMCV_STAGE_BINARY);
    r.image = r.binary && !has(RMCV_STAGE_NO_IMAGE);
    r.enhance_tables = r.binary && enhance;
    r.window_origins = r.binary && win;
    r.frame_keys = r.binary && keys;
    r.sparse = !timed && !legacy && has(RMCV_STAGE_CONTOURS) && has(RMCV_STAGE_BLOBS);
    r.sparse_pairs = r.sparse && has(RMCV_STAGE_ARMOURS);
    r.sparse_identity = r.sparse_pairs && has(RMCV_STAGE_IDENTITY) && input_format == RMCV_INPUT_BGR && !enhance && !win && !models;
    r.contours = !r.sparse && has(RMCV_STAGE_CONTOURS);
    const bool both = has(RMCV_STAGE_BLOBS) && has(RMCV_STAGE_ARMOURS), rest = !r.sparse && has(RMCV_STAGE_BLOBS);
    r.match = rest && legacy;
    r.match_pairs = r.match && both;
    r.blobs_armours = rest && !legacy && both;
    r.blobs = rest && !legacy && !both;
    r.armours = !r.sparse && !both && has(RMCV_STAGE_ARMOURS);
    r.classify = has(RMCV_STAGE_IDENTITY) && !r.sparse_identity;
    r.pnp = has(RMCV_STAGE_POSE);
    return r;
}
// the stages the batch bound has been through since its last pixel pass, after a run of `stages`
inline int next_last_stages(int last, int stages) { return (stages & RMCV_STAGE_BINARY) ? stages : (last | stages); }

// ---- the values rmcv_ctx_set_option takes: lo .. hi, or (ends_only) lo and hi alone ----
struct OptionRule {
    int option, lo, hi;
    bool ends_only;
    bool accepts(int v) const { return ends_only ? (v == lo || v == hi) : (v >= lo && v <= hi); }
};
static constexpr int OPT_PIXEL_ROWQUAD = 1001; // dev (not in the header): Geom::pixel_rowquad, for bench.py's RMCV_BENCH_AB=1001:0:1
static constexpr OptionRule OPTION_RULES[] = {
    {RMCV_OPT_SPARSE_WAVES, 4, 8, true},
    {RMCV_OPT_RUN_AHEAD, 0, 1, false},
    {RMCV_OPT_FRAME_UPLOAD, 0, 3, false},
    {RMCV_OPT_TEST_SLOW_US, 0, INT_MAX, false},
    {RMCV_OPT_PIXEL_HALO_NT, 0, 1, false},
    {OPT_PIXEL_ROWQUAD, 0, 1, false},
    {RMCV_OPT_PIXEL_SHAPE, 0, 1, false},
    {RMCV_OPT_OVERLOADS, 0, 3, false},
    {RMCV_OPT_DENSE_DEFER, 0, 1, false},
    {RMCV_OPT_CONTOUR_TIER, 0, 2, false},
    {RMCV_OPT_IMAGE_EXPORT, 0, 2, false},
    {RMCV_OPT_WAIT_TIMEOUT_MS, 0, INT_MAX, false},
    {RMCV_OPT_TEST_DELAY_US, 0, 10000000, false},
    {RMCV_OPT_INPUT_FORMAT, RMCV_INPUT_BGR, RMCV_BAYER_BG, false},
    {RMCV_OPT_INPUT_SAMPLE_BITS, 8, 16, true},
    {RMCV_OPT_INPUT_VALID_BIT, 0, 4, false},
    {RMCV_OPT_INPUT_ORIENT, 0, RMCV_ORIENT_MIRROR | RMCV_ORIENT_FLIP, false},
    {RMCV_OPT_ENHANCE, 0, 1, false},
    {RMCV_OPT_PIXEL_GROUPS, 1, 8, false},
};
// the rule of an option, or null: not an option
inline const OptionRule* option_rule(int option)
{
    for (const OptionRule& r : OPTION_RULES)
        if (r.option == option) return &r;
    return nullptr;
}

} // namespace rmcv
