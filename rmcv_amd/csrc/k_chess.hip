// k_chess.hip -- the chessboard detector: the inner corners of a cols x rows pattern in n chosen frames of a batch, coarse, into
// the caller's device tables in the layout k_corner_subpix refines.  The rule is the text at the head of device_chess.h, the same source
// rmcv_find_chessboard_host runs on the CPU; what is decided outside the kernels is chess_plan.h.
//
// Mapping (gfx950, wave64), two launches behind a memset of the count words:
// k_chess_response<SRC>: a 256-thread workgroup owns a 64 x 32 tile of one chosen frame.  It stages the tile's gray bytes with a halo of
//   5 + nms in LDS -- each a clamped read of SRC(f) through device_corner.h's accessor: the frame's bytes, its table, or the demosaic of its
//   mosaic -- computes R for the tile with a halo of nms into LDS (int16; both images at constant pitches), and a wavefront takes a row of 64 pixels through the non-maximum test.
//   Candidates are appended to the frame's list with one ballot and one atomic per wavefront and row; appends past the cap are dropped but
//   counted.  No frame-sized gray or response image is written to memory.
// k_chess_grid<SRC>: one 512-thread workgroup per chosen frame.  A rank sort of the keys in LDS (the append order is not deterministic, the
//   sorted order is); then a wavefront per candidate: eight rounds of a wave-wide minimum over the others' keys pick its nearest eight, lane
//   8 s + k - 1 takes sample k of the edge test with partner s (its 18 taps read SRC(f) through the caches), two ballots tell which partners
//   pass; a thread per candidate keeps the mutual ones, ascending; one lane runs chess_label on the LDS tables (at most 1024 nodes of degree
//   at most 4); the workgroup stores corners, count, status and, where asked for, the sorted candidates.
// Ordinary vector loads and stores; no scratch; static LDS 12 104 B and 48 132 B (chess_plan.h).
#include "rmcv_internal.h"
#include "device_chess.h"

namespace rmcv {

template <int SRC>
__global__ __launch_bounds__(256) void k_chess_response(ChessJob j)
{
    __shared__ uint32_t s_gray[CHESS_GRAY_MAX / 4];
    __shared__ int16_t s_resp[CHESS_RESP_MAX];
    constexpr int GP = CHESS_GRAY_PITCH, RP = CHESS_RESP_PITCH;   // (constants: every tap's LDS offset is an immediate)
    const int tid = threadIdx.x, lane = tid & 63, k = blockIdx.z;
    const FramePixels S = frame_pixels<SRC>(j.src, j.frames ? j.frames[k] : k);
    const int nms = j.prm.nms, halo = CHESS_RING_R + nms, w = j.src.w, h = j.src.h;
    const int x0 = blockIdx.x * CHESS_TILE_X, y0 = blockIdx.y * CHESS_TILE_Y;
    const int gc = chess_gray_cols(nms), gr = chess_gray_rows(nms), rc = chess_resp_cols(nms), rr = chess_resp_rows(nms);
    uint8_t* g8 = reinterpret_cast<uint8_t*>(s_gray);
    for (int i = tid; i < gc * gr; i += 256) {
        const int r = i / gc, c = i - r * gc;
        g8[r * GP + c] = (uint8_t)corner_gray_at<SRC>(S, x0 - halo + c, y0 - halo + r);
    }
    __syncthreads();
    for (int i = tid; i < rc * rr; i += 256) {
        const int r = i / rc, c = i - r * rc;
        int v = 0;
        if (chess_inside_ring(x0 - nms + c, y0 - nms + r, w, h)) {
            const uint8_t* centre = g8 + (r + CHESS_RING_R) * GP + c + CHESS_RING_R;
            v = chess_response([&](int dx, int dy) { return (int)centre[dy * GP + dx]; });
        }
        s_resp[r * RP + c] = (int16_t)v;   // (R lies in -30600 .. 10200)
    }
    __syncthreads();
    uint32_t* count = j.lists + k;
    uint32_t* keys = j.lists + j.n + (int64_t)k * CHESS_LIST_WORDS;
    for (int it = 0; it < CHESS_TILE_Y / 4; it++) {
        const int r = it * 4 + (tid >> 6), c = lane;   // (a wavefront: one row of the tile)
        const int16_t* centre = s_resp + (r + nms) * RP + c + nms;
        const int mine = *centre;
        bool cand = mine > j.prm.threshold;   // (threshold >= 0: never a pixel of the border or beyond the image, whose R is 0)
        if (cand)
            for (int dy = -nms; dy <= nms && cand; dy++)
                for (int dx = -nms; dx <= nms; dx++)
                    if ((dx | dy) != 0 && chess_beaten(mine, centre[dy * RP + dx], dx, dy)) {
                        cand = false;
                        break;
                    }
        const unsigned long long m = __ballot(cand);
        if (m == 0) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
        base = __shfl(base, 0);
        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (cand && at < RMCV_CHESS_CAND_MAX) {
            keys[at] = chess_key(x0 + c, y0 + r);
            keys[RMCV_CHESS_CAND_MAX + at] = (uint32_t)mine;
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(CHESS_GRID_THREADS) void k_chess_grid(ChessJob j)
{
    __shared__ uint32_t s_key0[RMCV_CHESS_CAND_MAX], s_key[RMCV_CHESS_CAND_MAX];
    __shared__ int32_t s_val0[RMCV_CHESS_CAND_MAX], s_val[RMCV_CHESS_CAND_MAX];
    __shared__ int16_t s_acc[4 * RMCV_CHESS_CAND_MAX], s_adj[4 * RMCV_CHESS_CAND_MAX], s_lab[2 * RMCV_CHESS_CAND_MAX], s_u[2 * RMCV_CHESS_CAND_MAX];
    __shared__ int16_t s_queue[RMCV_CHESS_CAND_MAX], s_grid[RMCV_CHESS_CAND_MAX], s_order[RMCV_CHESS_CAND_MAX];
    __shared__ uint8_t s_seen[RMCV_CHESS_CAND_MAX];
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = blockIdx.x;
    const uint32_t total = j.lists[k];
    const uint32_t* keys = j.lists + j.n + (int64_t)k * CHESS_LIST_WORDS;
    if (total > RMCV_CHESS_CAND_MAX) {   // (the whole workgroup)
        if (tid == 0) {
            j.counts[k] = 0;
            if (j.status) j.status[k] = chess_status(total, RMCV_CHESS_OVERFLOW);
            if (j.cand_n) j.cand_n[k] = 0;
        }
        return;
    }
    const int n = (int)total;
    for (int i = tid; i < n; i += CHESS_GRID_THREADS) {
        s_key0[i] = keys[i];
        s_val0[i] = (int32_t)keys[RMCV_CHESS_CAND_MAX + i];
    }
    __syncthreads();
    for (int i = tid; i < n; i += CHESS_GRID_THREADS) {   // keys are distinct pixels: the rank is the place
        const uint32_t mine = s_key0[i];
        int rank = 0;
        for (int o = 0; o < n; o++) rank += s_key0[o] < mine;
        s_key[rank] = mine;
        s_val[rank] = s_val0[i];
    }
    __syncthreads();
    const FramePixels S = frame_pixels<SRC>(j.src, j.frames ? j.frames[k] : k);
    const int dmin2 = j.prm.dist_min * j.prm.dist_min, dmax2 = j.prm.dist_max * j.prm.dist_max, bar = 9 * j.prm.contrast;
    for (int a = wv; a < n; a += CHESS_GRID_THREADS / 64) {
        const uint32_t pa = s_key[a];
        int32_t last = -1;
        int partner = -1;   // of slot lane >> 3
        for (int round = 0; round < CHESS_NEAR; round++) {
            int32_t m = INT32_MAX;
            for (int o = lane; o < n; o += 64) {
                const int32_t key = chess_near_key(pa, s_key[o], a, o, dmin2, dmax2);
                if (key > last && key < m) m = key;
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const int32_t o = __shfl_xor(m, s);
                m = o < m ? o : m;
            }
            if (m == INT32_MAX) break;   // (the same in every lane)
            last = m;
            if ((lane >> 3) == round) partner = m & (RMCV_CHESS_CAND_MAX - 1);
        }
        const int sample = (lane & 7) + 1;
        const bool valid = partner >= 0 && sample <= 7;
        int diff = 0;
        if (valid) {
            const int p = a < partner ? a : partner, q = a < partner ? partner : a;
            diff = chess_edge_diff([&](int x, int y) { return corner_gray_at<SRC>(S, x, y); }, s_key[p], s_key[q], sample);
        }
        const unsigned long long pos = __ballot(valid && diff > bar), neg = __ballot(valid && diff < -bar);
        int got = 0;
#pragma unroll
        for (int slot = 0; slot < CHESS_NEAR; slot++) {
            const int b = __shfl(partner, 8 * slot);
            const bool pass = ((pos >> (8 * slot)) & 0x7F) == 0x7F || ((neg >> (8 * slot)) & 0x7F) == 0x7F;
            if (b >= 0 && pass && got < CHESS_DEGREE) {
                if (lane == 0) s_acc[4 * a + got] = (int16_t)b;
                got++;
            }
        }
        if (lane == 0)
            for (int t = got; t < CHESS_DEGREE; t++) s_acc[4 * a + t] = -1;
    }
    __syncthreads();
    for (int a = tid; a < n; a += CHESS_GRID_THREADS) {
        int deg = 0;
        for (int t = 0; t < CHESS_DEGREE; t++) {
            const int b = s_acc[4 * a + t];
            bool mutual = false;
            for (int s = 0; b >= 0 && s < CHESS_DEGREE; s++) mutual = mutual || s_acc[4 * b + s] == a;
            if (!mutual) continue;
            int at = deg++;
            for (; at > 0 && s_adj[4 * a + at - 1] > b; at--) s_adj[4 * a + at] = s_adj[4 * a + at - 1];
            s_adj[4 * a + at] = (int16_t)b;
        }
        for (int t = deg; t < CHESS_DEGREE; t++) s_adj[4 * a + t] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        ChessTables T;
        T.key = s_key; T.adj = s_adj; T.lab = s_lab; T.u = s_u; T.queue = s_queue; T.grid = s_grid; T.order = s_order; T.seen = s_seen;
        s_found = chess_label(T, n, j.cols, j.rows) ? 1 : 0;
    }
    __syncthreads();
    const bool found = s_found != 0;
    if (found) {
        float* row = j.corners + 2 * (int64_t)k * j.per_frame;
        for (int g = tid; g < j.cols * j.rows; g += CHESS_GRID_THREADS) {
            const uint32_t key = s_key[s_order[g]];
            row[2 * g] = (float)chess_x(key);
            row[2 * g + 1] = (float)chess_y(key);
        }
    }
    if (j.cand) {
        int32_t* out = j.cand + 3 * (int64_t)k * RMCV_CHESS_CAND_MAX;
        for (int i = tid; i < n; i += CHESS_GRID_THREADS) {
            out[3 * i] = chess_x(s_key[i]);
            out[3 * i + 1] = chess_y(s_key[i]);
            out[3 * i + 2] = s_val[i];
        }
    }
    if (tid == 0) {
        j.counts[k] = found ? j.cols * j.rows : 0;
        if (j.status) j.status[k] = chess_status(total, found ? RMCV_CHESS_FOUND : RMCV_CHESS_NO_GRID);
        if (j.cand_n) j.cand_n[k] = n;
    }
}

template <int SRC>
static hipError_t launch_chess_kind(const ChessJob& j, hipStream_t s)
{
    const dim3 tiles((unsigned)chess_tiles_x(j.src.w), (unsigned)chess_tiles_y(j.src.h), (unsigned)j.n);
    hipError_t e = hipMemsetAsync(j.lists, 0, (size_t)j.n * 4, s);
    if (e == hipSuccess) e = launch(k_chess_response<SRC>, tiles, dim3(256), 0, s, j);
    if (e == hipSuccess) e = launch(k_chess_grid<SRC>, dim3((unsigned)j.n), dim3(CHESS_GRID_THREADS), 0, s, j);
    return e;
}

hipError_t launch_chess(const ChessJob& j, hipStream_t s)
{
    return with_source_kind(j.src.kind, [&](auto K) { return launch_chess_kind<decltype(K)::value>(j, s); });
}

} // namespace rmcv

// ---- the host-side entry points (no context) ----
extern "C" {

void rmcv_chess_defaults(rmcv_chess_params* p)
{
    if (p) *p = rmcv::chess_default_params();
}

int rmcv_find_chessboard_host(const uint8_t* bgr, int w, int h, int stride, int cols, int rows, const rmcv_chess_params* params, float* corners_out,
                              int32_t* status_out, int32_t* cand_out, int32_t* cand_n_out)
{
    const rmcv_chess_params prm = params ? *params : rmcv::chess_default_params();
    if (rmcv::chess_image_refusal(bgr, corners_out, w, h, stride) || rmcv::chess_params_refusal(cols, rows, prm)) return RMCV_ERR_BAD_ARG;
    rmcv::chess_find_host(bgr, w, h, stride, cols, rows, prm, corners_out, status_out, cand_out, cand_n_out);
    return RMCV_OK;
}

} // extern "C"
