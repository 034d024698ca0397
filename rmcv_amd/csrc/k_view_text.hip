// k_view_text.hip -- the label pass over finished views: for n views of a batch, already rendered by either view kind into
// the caller's device memory, the text line rm::debug::draw_armours writes next to every armour (src/debug.cpp:53-57) and, for a tracked
// run, every target's quadrilateral and line.  Formats, glyphs, placement and the draws are device_text.h, the same source
// rmcv_view_labels_host runs on the CPU.
//
// Mapping (gfx950, wave64).  ONE LAUNCH, one workgroup of 4 wavefronts per view; a wavefront takes a label.  Lanes 0 .. 4 each format one
// number of the line into the wavefront's own LDS row (a digit is only ever stored to LDS: no private array is indexed dynamically, no
// scratch), lanes 0 .. 3 map the four vertices; behind a workgroup barrier lanes 0 .. 3 walk one edge of the quadrilateral each, then
// lane = character (two trips cover RMCV_LABEL_MAX_CHARS) and every lane blits its own glyph with byte stores into the caller's layout --
// no alignment of the view is assumed.  The trip count of a phase is the same for the four wavefronts, so the barriers are uniform.
// The two colours are two phases of the workgroup, tracks first, separated by a barrier (its release / acquire orders the byte stores of
// the phases where a yellow pixel lands on a magenta one); within a phase every store writes the same three bytes, so no order is needed.
// Counts read from device tables are clamped to the tables' capacities.  Static LDS: 816 B; no scratch.
#include <atomic>

#include "rmcv_internal.h"
#include "device_text.h"

namespace rmcv {

static constexpr int TEXT_WAVES = 4, TEXT_THREADS = 64 * TEXT_WAVES;

__global__ __launch_bounds__(TEXT_THREADS) void k_view_text(LabelJob j)
{
    __shared__ char s_f[TEXT_WAVES][LABEL_FIELDS * LABEL_FIELD];
    __shared__ int s_start[TEXT_WAVES][LABEL_FIELDS];
    __shared__ long long s_xy[TEXT_WAVES][8];
    const int v = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (v >= j.n) return;
    const int f = j.frames ? j.frames[v] : v;
    if (f < 0 || f >= j.n_frames) return; // (the host has checked the list; uniform over the workgroup)
    uint8_t* const view = j.out + (int64_t)v * j.out_pitch;
    const int stride = j.out_stride, vw = j.vw, vh = j.vh;
    char* const fields = s_f[wave];
    int* const starts = s_start[wave];
    long long* const xy = s_xy[wave];

    // ---- the tracks of the frame's stream: quadrilateral and line, (255, 0, 255)
    if (j.tracks) {
        auto put = [=](int x, int y) {
            uint8_t* p = view + (int64_t)y * stride + 3 * x;
            p[0] = 255, p[1] = 0, p[2] = 255;
        };
        const int raw = j.n_tracking[f];
        const int nt = raw < 0 ? 0 : (raw > j.track_cap ? j.track_cap : raw);
        const size_t at = ((size_t)(j.sel ? j.sel[f] & 1 : 0) * j.n_streams + f) * j.track_cap;
        rmcv_point org = {j.x_eff, j.y_eff};
        if (j.win_eff) org = j.win_eff[f];
        for (int t0 = 0; t0 < nt; t0 += TEXT_WAVES) {
            const int t = t0 + wave;
            const bool live = t < nt;
            unsigned ok = 0;
            if (live) {
                const rmcv_track* tr = j.tracks + at + t;
                int mine = 0;
                if (lane < 4) {
                    int64_t ax = 0, ay = 0;
                    mine = label_anchor(j.side + (at + t) * 8 + 2 * lane, org.x, org.y, j.w, j.h, vw, vh, &ax, &ay);
                    xy[2 * lane] = ax, xy[2 * lane + 1] = ay;
                }
                ok = (unsigned)__ballot(mine) & 15u;
                if (lane == 0) starts[0] = label_dec(tr->identity, fields);
                else if (lane < 4) starts[lane] = label_f6(label_track_coord(tr, lane - 1), fields + lane * LABEL_FIELD);
                else if (lane == 4) starts[4] = label_dec(tr->lost_count, fields + 4 * LABEL_FIELD);
            }
            __syncthreads();
            if (live) {
                if (ok == 15u && lane < 4) label_segment(vw, vh, xy[2 * lane], xy[2 * lane + 1], xy[2 * ((lane + 1) & 3)], xy[2 * ((lane + 1) & 3) + 1], put);
                if (ok & 1u)
                    for (int k = lane; k < RMCV_LABEL_MAX_CHARS; k += 64) {
                        const int ch = label_char_at(fields, starts, 5, k);
                        if (ch) label_blit(vw, vh, xy[0], xy[1], j.scale, k, ch, put);
                    }
            }
            __syncthreads();
        }
    }
    __syncthreads(); // every store of the first colour is behind this for every wavefront of the workgroup

    // ---- the frame's armours: the reference's line at vertices[0], (0, 255, 255)
    if (j.armours) {
        auto put = [=](int x, int y) {
            uint8_t* p = view + (int64_t)y * stride + 3 * x;
            p[0] = 0, p[1] = 255, p[2] = 255;
        };
        const int raw = j.n_armours[f];
        const int na = raw < 0 ? 0 : (raw > j.max_armours ? j.max_armours : raw);
        const size_t base = (size_t)f * j.max_armours;
        for (int i0 = 0; i0 < na; i0 += TEXT_WAVES) {
            const int i = i0 + wave;
            const bool live = i < na;
            unsigned ok = 0;
            if (live) {
                int mine = 0;
                if (lane == 0) {
                    int64_t ax = 0, ay = 0;
                    mine = label_anchor(j.armours[base + i].vertices[0], 0, 0, j.w, j.h, vw, vh, &ax, &ay);
                    xy[0] = ax, xy[1] = ay;
                    starts[0] = label_dec(j.identity ? j.identity[base + i] : -1, fields);
                } else if (lane < 4) {
                    starts[lane] = label_f6(j.positions ? j.positions[(base + i) * j.pos_stride + (lane - 1)] : 0.0, fields + lane * LABEL_FIELD);
                }
                ok = (unsigned)__ballot(mine) & 1u;
            }
            __syncthreads();
            if (live && ok)
                for (int k = lane; k < RMCV_LABEL_MAX_CHARS; k += 64) {
                    const int ch = label_char_at(fields, starts, 4, k);
                    if (ch) label_blit(vw, vh, xy[0], xy[1], j.scale, k, ch, put);
                }
            __syncthreads();
        }
    }
}

static std::atomic<int64_t> g_text_launches{0};
int64_t view_text_launches() { return g_text_launches.load(std::memory_order_relaxed); }

hipError_t launch_view_text(const LabelJob& j, hipStream_t s)
{
    if (j.n < 1 || (!j.tracks && !j.armours)) return hipSuccess;
    g_text_launches.fetch_add(1, std::memory_order_relaxed);
    return launch(k_view_text, dim3(j.n), dim3(TEXT_THREADS), 0, s, j);
}

} // namespace rmcv
