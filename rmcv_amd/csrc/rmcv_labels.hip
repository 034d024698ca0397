// rmcv_labels.hip -- view labels behind the ABI: the host-side functions, which need no context and no device -- the two
// number formats' public face, the lines, the glyphs, and the sequential restatement rmcv_view_labels_host -- and the stage-wise
// rmcv_view_labels, the kernel on host lists with buffers of its own.  The rule is device_text.h; the batch entry points, which live
// on a context's bound tables, are rmcv_views.hip's; the pipeline's setter is rmcv_pipeline.hip's.  No kernel lives here.
// With RMCV_LABELS_HOST_ONLY defined only the host-side functions are compiled, by any C++ compiler, with no HIP header in sight: the
// form tests/labels_san_main.cpp builds under the sanitizers.
#include <string.h>

#include "device_text.h"
#ifndef RMCV_LABELS_HOST_ONLY
#include "rmcv_ctx.h"

using namespace rmcv;
#endif

// a line into the caller's buffer: its length, or RMCV_ERR_CAPACITY when cap cannot hold it and its terminator (nothing of it is promised then)
static int line_out(const label_fields& L, int n_fields, char* out, int cap)
{
    if (!out || cap < 1) return RMCV_ERR_BAD_ARG;
    const int n = label_line_host(L.f, L.start, n_fields, out, cap);
    if (n < 0) {
        out[cap - 1] = 0;
        return RMCV_ERR_CAPACITY;
    }
    return n;
}

extern "C" {

int rmcv_format_f6(double v, char* out, int cap)
{
    label_fields L;
    L.start[0] = label_f6(v, L.f);
    return line_out(L, 1, out, cap);
}

int rmcv_label_text(int32_t identity, const double position[3], char* out, int cap)
{
    label_fields L;
    label_fields_armour(&L, identity, position);
    return line_out(L, 4, out, cap);
}

int rmcv_track_label_text(const rmcv_track* t, char* out, int cap)
{
    if (!t) return RMCV_ERR_BAD_ARG;
    label_fields L;
    label_fields_track(&L, t);
    return line_out(L, 5, out, cap);
}

int rmcv_view_glyph(int ch, uint8_t rows[7])
{
    if (!rows) return RMCV_ERR_BAD_ARG;
    const uint64_t g = label_glyph(ch);
    if (g == ~0ull) return RMCV_ERR_BAD_ARG;
    for (int r = 0; r < LABEL_GLYPH_H; r++) rows[r] = (uint8_t)label_glyph_row(g, r);
    return RMCV_OK;
}

int rmcv_view_labels_host(uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours, const int32_t* identities,
                          const double* positions, int n_armours, const rmcv_track* tracks, const float* last_vertices, int n_tracks, int x_eff, int y_eff)
{
    if (!tracks) n_tracks = 0; // (nullable: no tracks)
    if (label_check_host(view, vw, vh, stride, w, h, scale, armours, n_armours, tracks, last_vertices, n_tracks)) return RMCV_ERR_BAD_ARG;
    label_host(view, vw, vh, stride, w, h, scale, armours, identities, positions, n_armours, tracks, last_vertices, n_tracks, x_eff, y_eff);
    return RMCV_OK;
}

#ifndef RMCV_LABELS_HOST_ONLY
int64_t rmcv_view_text_launches(void) { return view_text_launches(); }

int rmcv_view_labels(rmcv_ctx* c, uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours, const int32_t* identities,
                     const double* positions, int n_armours, const rmcv_track* tracks, const float* last_vertices, int n_tracks, int x_eff, int y_eff)
{
    if (!c) return RMCV_ERR_BAD_ARG;
    if (!tracks) n_tracks = 0;
    if (const char* bad = label_check_host(view, vw, vh, stride, w, h, scale, armours, n_armours, tracks, last_vertices, n_tracks)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "rmcv_view_labels: %s", bad);
        return fail(c, RMCV_ERR_BAD_ARG, msg);
    }
    if (vw > c->lim.max_width || vh > c->lim.max_height) return fail(c, RMCV_ERR_BAD_ARG, "rmcv_view_labels: the view is beyond the context's max_width / max_height");
    if (const int rc = ctx_ready(c)) return rc;
    // (a stage-wise helper: buffers of its own, so that nothing bound to the context moves) -- one host block, one upload.  The view keeps
    // the caller's stride on the device: the kernel writes into the layout it was given
    const size_t view_bytes = (size_t)stride * (vh - 1) + (size_t)3 * vw;
    const size_t o_arm = up16(view_bytes), o_id = o_arm + up16((size_t)n_armours * sizeof(rmcv_armour)), o_pos = o_id + up16((size_t)n_armours * 4);
    const size_t o_trk = o_pos + up16((size_t)n_armours * 24), o_side = o_trk + up16((size_t)n_tracks * sizeof(rmcv_track));
    const size_t o_cnt = o_side + up16((size_t)n_tracks * 32), total = o_cnt + 16;
    std::vector<uint8_t> host(total, 0);
    memcpy(host.data(), view, view_bytes);
    if (n_armours) memcpy(&host[o_arm], armours, (size_t)n_armours * sizeof(rmcv_armour));
    if (n_armours && identities) memcpy(&host[o_id], identities, (size_t)n_armours * 4);
    if (n_armours && positions) memcpy(&host[o_pos], positions, (size_t)n_armours * 24);
    if (n_tracks) memcpy(&host[o_trk], tracks, (size_t)n_tracks * sizeof(rmcv_track));
    if (n_tracks) memcpy(&host[o_side], last_vertices, (size_t)n_tracks * 32);
    const int32_t counts[4] = {n_armours, n_tracks, 0, 0};
    memcpy(&host[o_cnt], counts, sizeof(counts));
    Scratch blk;
    hipError_t e = blk.alloc(total);
    uint8_t* const d = blk.d;
    if (e == hipSuccess) e = hipMemcpyAsync(d, host.data(), total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const int32_t* cnt = reinterpret_cast<const int32_t*>(d + o_cnt);
        LabelJob j{};
        j.n = 1, j.vw = vw, j.vh = vh, j.w = w, j.h = h, j.scale = scale, j.n_frames = 1;
        j.out = d, j.out_stride = stride, j.out_pitch = 0, j.frames = nullptr;
        if (n_armours) {
            j.armours = reinterpret_cast<const rmcv_armour*>(d + o_arm), j.n_armours = cnt, j.max_armours = n_armours;
            j.identity = identities ? reinterpret_cast<const int32_t*>(d + o_id) : nullptr;
            j.positions = positions ? reinterpret_cast<const double*>(d + o_pos) : nullptr;
            j.pos_stride = 3;
        }
        if (n_tracks) {
            j.tracks = reinterpret_cast<const rmcv_track*>(d + o_trk), j.side = reinterpret_cast<const float*>(d + o_side);
            j.sel = nullptr, j.n_tracking = cnt + 1, j.n_streams = 1, j.track_cap = n_tracks;
            j.win_eff = nullptr, j.x_eff = x_eff, j.y_eff = y_eff;
        }
        e = launch_view_text(j, c->stream);
    }
    c->last_what = "k_view_text";
    int rcw = 0;
    if (e == hipSuccess) rcw = blk.waited(wait_stream(c, c->stream, "k_view_text"));
    if (e == hipSuccess && rcw == 0) e = hipMemcpy2D(view, stride, d, stride, (size_t)3 * vw, vh, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? RMCV_ERR_NOMEM : RMCV_ERR_HIP, "rmcv_view_labels", e);
    return rcw;
}
#endif

} // extern "C"
