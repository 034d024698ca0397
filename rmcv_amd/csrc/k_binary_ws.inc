// k_binary_ws.inc -- K1 with the workgroup's wavefronts SPECIALISED (included by k_binary.hip, inside namespace rmcv).
//
// Why (profiles/r04f_k_binary_ws.txt): a bare 3:1 copy with k_binary's traffic (every workgroup walks its own strip: 120 KB in,
// 40 KB out) takes 0.2326 ms with 768 workgroups of 256 threads -- k_binary's own time -- but 0.2143 ms when ONE 1024-thread
// workgroup per CU lets 8 wavefronts load strip k+1 into LDS while 8 others write strip k out: the grid-stride copy's 0.2146.
// One address stream in and one out per CU, both running all the time, instead of three or four workgroups per CU that each
// load, compute and store in turn.
//
//   loader waves  (NL): phase 1 of k_binary.hip for strip k+1 -- coalesced dwordx3, thresh16, quad transpose, ds_write_b16 -- into
//                 the bit plane T[(k+1) & 1]
//   storer waves  (NS): strip k from T[k & 1]: every wave owns SR / NS output rows and computes them from T ALONE -- dilate and
//                 erode fused per output word (6 rows x 3 words of T in registers; the column ORs of the dilate are shared by the
//                 two output rows a lane produces) -- so no storer waits for another; then the bit plane words, the row masks
//                 and the 0/255 bytes of its own rows (wave-private staging in LDS for the coalesced 16-byte stores)
//   one s_barrier per strip for the whole workgroup: T[k & 1] is free, T[(k+1) & 1] is full.
//
// Same results bit for bit (same border rules: rows and columns outside the image read 0 for the dilate and 1 for the erode),
// same strip queue per XCD, same leaver protocol.  Used for whole batches whose rows are contiguous (the linear loader's
// condition); everything else -- strided rows, single frames handed out as pieces, lb <= 0 -- stays with k_binary.

struct K1Args {
    const uint8_t* frames;
    int64_t frame_pitch;
    int stride, n_frames, w, h, ww, lb, morph;
    uint8_t* binary;
    uint64_t* bits;
    int prow;
    int64_t plane_pitch;
    int strips, n_blocks;
    uint32_t* rowmask;
    int* strip_ctr;
    uint32_t* imgmask; // [frame][h] bit k: the 64 bytes of word k of the row in `binary` may be non-zero (image_plan.h); ww <= 32
    int delta;         // 1: `imgmask` is in force -- store only the words that are or were non-zero; 0: store every byte
    int plane_delta;   // 1 (with delta): plane and row masks come from the same launches as the image (image_plan.h: plane_step) -- the plane's
                       // words go by the image's mask as well, pad words are not stored, a row mask only where it changed
};

// Lane r of storer wave sw: the image's mask of row r of the wave's rows of strip L (0: no such row, or no delta launch).  The wave asks for
// it while it stores the strip BEFORE -- behind that strip's morphology, where the wave's registers are scarce: the answer comes from HBM,
// beside a kernel that keeps every channel busy, and takes microseconds.  The read ahead cannot race with a write of the mask: within a
// launch a row's mask is read and written by ONE wave (the strip's storer wave that owns the row), every strip is drawn once, and the
// launches of one context are ordered on its streams -- the word read here was last written by an earlier launch.
template <int NS>
__device__ __forceinline__ uint32_t ws_image_mask(const K1Args& a, const int L, const int sw, const int lane)
{
    constexpr int RPW = SR / NS;
    if (!(a.delta && a.binary && a.ww <= 32) || L < 0) return 0u;
    const int f = L / a.strips, y = (L - f * a.strips) * SR + sw * RPW + lane;
    return (lane < RPW && y < a.h) ? a.imgmask[(int64_t)f * a.h + y] : 0u;
}

template <int NS>
__device__ __forceinline__ uint32_t ws_store_strip(const K1Args& a, const int L, const uint64_t* __restrict__ T, uint64_t* __restrict__ Ew,
                                               const uint64_t* __restrict__ lut, const int sw, const int lane,
                                               const __amdgpu_buffer_rsrc_t r_bin, const __amdgpu_buffer_rsrc_t r_plane, const uint32_t m_old,
                                                   const int L_next)
{
    constexpr int RPW = SR / NS; // output rows per storer wave
    static_assert(RPW >= 2 && RPW % 2 == 0, "a lane produces a pair of rows");
    const int halo = a.morph, ww = a.ww, w = a.w, h = a.h;
    const int f = L / a.strips, strip = L - f * a.strips;
    const int y0 = strip * SR;
    const int s0 = sw * RPW; // this wave's first row of the strip
    if (y0 + s0 >= h) return ws_image_mask<NS>(a, L_next, sw, lane); // (wave-uniform) its rows lie below the image
    const uint32_t plane_base = (uint32_t)((int64_t)f * a.plane_pitch);
    const int n_task = (RPW / 2) * ww; // (row pair, word)
    const uint32_t r_ww = (uint32_t)((0x100000000ull + ww - 1) / ww);
    // m_new (lane r: the new mask of row r) is set on exactly one of the two row-mask paths below for every ww <= 32: in the pass itself
    // when the wave's tasks fit one pass (n_task <= 64), behind the passes otherwise.  (With RPW = 4 the second never runs: n_task = 2 ww.)
    // m_old: what the image holds in this wave's rows (lane r: row r; ws_image_mask, asked for a strip ahead).  Returns the next strip's.
    const bool masked = a.binary && ww <= 32, delta = masked && a.delta, pdelta = delta && a.plane_delta;
    const bool my_row = lane < RPW && y0 + s0 + lane < h;
    uint32_t* const im = a.imgmask + ((int64_t)f * h + y0 + s0 + lane);
    uint32_t m_new = 0;
    for (int t0 = 0; t0 < n_task; t0 += 64) {
        const int t = t0 + lane;
        const bool on = t < n_task;
        const int p = on ? div_r(t, r_ww) : 0, k = on ? t - p * ww : 0;
        const int s = s0 + 2 * p; // strip row of the first of the two outputs = index of the first row of T it depends on
        const uint64_t* base = T + __umul24(s, ww) + k;
        uint64_t e0, e1;
        if (halo == 0) {
            e0 = base[0];
            e1 = base[ww];
        } else {
            const int nr = 2 + 2 * halo; // rows of T behind the pair: 4 (dilate) or 6 (close)
            uint64_t ta[6], tb[6], tc[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                if (i < nr) {
                    tb[i] = base[i * ww];
                    ta[i] = k > 0 ? base[i * ww - 1] : 0ull;
                    tc[i] = k < ww - 1 ? base[i * ww + 1] : 0ull;
                } else {
                    ta[i] = tb[i] = tc[i] = 0ull;
                }
            }
            uint64_t Db[4];
            uint32_t DL[4], DR[4]; // bit 63 of the dilated word to the left, bit 0 of the one to the right
#pragma unroll
            for (int i = 1; i <= 4; i++) {
                if (i <= nr - 2) {
                    const uint64_t ca = ta[i - 1] | ta[i] | ta[i + 1], cb = tb[i - 1] | tb[i] | tb[i + 1], cc = tc[i - 1] | tc[i] | tc[i + 1];
                    uint64_t d = cb | (cb << 1) | (cb >> 1) | (ca >> 63) | ((cc & 1ull) << 63);
                    uint32_t dl = (uint32_t)((ca >> 62) != 0) | (uint32_t)(cb & 1ull);
                    uint32_t dr = (uint32_t)((cc & 3ull) != 0) | (uint32_t)(cb >> 63);
                    const int y = y0 - halo + s + i;
                    if (y < 0 || y >= h) { d = ~0ull; dl = 1; dr = 1; } // a row outside the image never wins the erode
                    if (k == 0) dl = 1;                                 // nor does a column outside it
                    if (k == ww - 1) dr = 1;
                    Db[i - 1] = d; DL[i - 1] = dl; DR[i - 1] = dr;
                } else {
                    Db[i - 1] = 0; DL[i - 1] = 0; DR[i - 1] = 0;
                }
            }
            if (halo == 1) {
                e0 = Db[0];
                e1 = Db[1];
            } else {
                uint64_t e[2];
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint64_t c = Db[j] & Db[j + 1] & Db[j + 2];
                    const uint64_t l = (uint64_t)(DL[j] & DL[j + 1] & DL[j + 2]), r = (uint64_t)(DR[j] & DR[j + 1] & DR[j + 2]);
                    e[j] = c & ((c << 1) | l) & ((c >> 1) | (r << 63));
                }
                e0 = e[0];
                e1 = e[1];
            }
        }
        const int y = y0 + s;
        // Delta stores of the plane: plane word k of a row is zero exactly when image word k is, so a word that is zero and was zero when the
        // context wrote it last (the image's mask says so) is not stored again; nor are the pads, which the last full launch left zero.
        bool k0 = true, k1 = true;
        if (pdelta) { // (wave-uniform)
            // the old masks of the wave's rows laid out as the tasks are -- bit t of mo0 / mo1: word k of the first / second row of task t's
            // pair was non-zero -- so that they meet the ballots of the new words bit for bit (ww <= 32: one pass of at most 64 tasks)
            static_assert(RPW / 2 * 32 <= 64, "a delta launch's tasks fit one pass");
            uint64_t mo0 = 0, mo1 = 0;
#pragma unroll
            for (int i = 0; i < RPW / 2; i++) {
                mo0 |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)m_old, 2 * i) << (i * ww);
                mo1 |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)m_old, 2 * i + 1) << (i * ww);
            }
            const uint64_t kb0 = mo0 | __builtin_amdgcn_ballot_w64(on && e0 != 0), kb1 = mo1 | __builtin_amdgcn_ballot_w64(on && e1 != 0);
            // (the unit is ONE word: whole rows with their pads, kept wherever the row is or was non-empty, measured no faster --
            // profiles/plane_delta_ab.txt)
            k0 = (kb0 >> lane) & 1ull;
            k1 = (kb1 >> lane) & 1ull;
        }
        if (on) {
            Ew[__umul24(2 * p, ww) + k] = e0;
            Ew[__umul24(2 * p + 1, ww) + k] = e1;
        }
        // the frame's bit plane (8 contiguous bytes per lane; plain stores: the sparse kernel of the same batch finds the words in L2)
#ifdef RMCV_K1_NOBITS
        const uint32_t po0 = OOB, po1 = OOB; // ablation build: the bit plane is not written
#else
        const uint32_t po0 = (on && y < h && k0) ? (plane_base + __umul24(y + 1, a.prow) + 1u + (uint32_t)k) * 8u : OOB;
        const uint32_t po1 = (on && y + 1 < h && k1) ? (plane_base + __umul24(y + 2, a.prow) + 1u + (uint32_t)k) * 8u : OOB;
#endif
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, e0), r_plane, po0, 0, RMCV_K1_PLAIN_PLAUX);
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, e1), r_plane, po1, 0, RMCV_K1_PLAIN_PLAUX);
        // ... and the two pad words between a row's last word and the next row's first (always zero): with them a row is 8 prow
        // CONTIGUOUS bytes and the plane's cache lines leave the L2 whole.  Without them every line goes out with a 16-byte hole, a
        // masked write that the memory side has to merge: free while the planes of all batches in flight sit in the Infinity Cache
        // (4 x 46 MB), 15 % of the kernel's time when they do not (8 x 46 MB) -- profiles/r04f_k_binary_ws.txt
        {
            const bool last = on && k == ww - 1 && !pdelta;
            const u32x4v z = {0u, 0u, 0u, 0u};
            __builtin_amdgcn_raw_buffer_store_b128(z, r_plane, last && po0 != OOB ? po0 + 8u : OOB, 0, RMCV_K1_PLAIN_PLAUX);
            __builtin_amdgcn_raw_buffer_store_b128(z, r_plane, last && po1 != OOB ? po1 + 8u : OOB, 0, RMCV_K1_PLAIN_PLAUX);
        }
        // row masks for the contour stage (bit k = word k of the row is non-zero): the pairs of one pass sit side by side in the wave
        if (ww <= 32 && n_task <= 64) {
            const uint64_t b0 = __builtin_amdgcn_ballot_w64(on && e0 != 0), b1 = __builtin_amdgcn_ballot_w64(on && e1 != 0);
            if (lane < RPW) {
                const int pr = lane >> 1;
                const uint64_t b = (lane & 1) ? b1 : b0;
                const uint32_t m = (uint32_t)(b >> __umul24(pr, ww)) & (ww == 32 ? 0xFFFFFFFFu : ((1u << ww) - 1u));
                m_new = m;
#ifndef RMCV_K1_NOROWMASK
                if (y0 + s0 + lane < h && (!pdelta || m != m_old)) a.rowmask[(int64_t)f * h + y0 + s0 + lane] = m;
#endif
            }
        }
    }
    // the wave's own words, written above by its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (ww <= 32 && n_task > 64) {
        if (lane < RPW && y0 + s0 + lane < h) {
            uint32_t m = 0;
            for (int k = 0; k < ww; k++) m |= (uint32_t)(Ew[__umul24(lane, ww) + k] != 0) << k;
            if (!pdelta || m != m_old) a.rowmask[(int64_t)f * h + y0 + s0 + lane] = m;
            m_new = m;
        }
    }
    const uint32_t m_ahead = ws_image_mask<NS>(a, L_next, sw, lane);
    if (a.binary) { // RMCV_STAGE_NO_IMAGE: the 0/255 byte image is not wanted
        // Delta stores: a 64-byte word of the image that is zero and was zero when this context wrote it last is not stored again (LED
        // bars on a dark field: 1.5 % of the words are not zero).  `keep` (lane r: row r) = the words to store; the mask then says what
        // the image holds now.  Nothing to keep in the wave's rows: no LUT work, no pass over the items.
        // (the unit is ONE aligned 64-byte word: aligned 128-byte pairs measured 4 % worse at C3, profiles/image_delta_schedule_ab.txt)
        const uint32_t keep = delta ? (m_old | m_new) : 0xFFFFFFFFu;
        if (masked && my_row && (!delta || m_new != m_old)) *im = m_new;
        if (delta && __builtin_amdgcn_ballot_w64(my_row && keep != 0) == 0) return m_ahead;
        // w % 64 == 0: the wave's rows are ONE run of 16-pixel items both in its LDS words and in the byte image
        const int n_valid = min(RPW, h - (y0 + s0)) * ww * 4;
        const uint16_t* R16 = reinterpret_cast<const uint16_t*>(Ew);
        const uint32_t out0 = (uint32_t)((int64_t)f * w * h) + (uint32_t)(y0 + s0) * (uint32_t)w;
        for (int b = 0; b < n_valid; b += 64) {
            const int it = b + lane;
            bool ok = it < n_valid;
            if (delta) { // (wave-uniform)
                const int wd = ok ? it >> 2 : 0, r = div_r(wd, r_ww), k = wd - r * ww; // the item's row of the wave and word of the row
                const uint32_t kr = (uint32_t)__shfl((int)keep, r);
                ok = ok && ((kr >> k) & 1u);
                if (__builtin_amdgcn_ballot_w64(ok) == 0) continue; // none of these 64 items is kept
            }
            const uint32_t m = R16[it < n_valid ? it : 0];
            const uint64_t lo = lut[m & 0xFF], hi = lut[m >> 8];
            const u32x4v o = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
#ifdef RMCV_K1_NOSTORE
            const uint32_t off = OOB; // ablation build: the byte image is not written
#else
            const uint32_t off = ok ? out0 + (uint32_t)it * 16u : OOB;
#endif
            __builtin_amdgcn_raw_buffer_store_b128(o, r_bin, off, 0, RMCV_K1_STAUX);
        }
    }
    return m_ahead;
}

// The loaders never drain: every loader wave keeps a RING of R items (4 dwordx3 loads each) in flight, across item, strip and
// barrier boundaries -- item b + R - 1 is issued before item b is thresholded, and the first R - 1 items of the NEXT strip are on
// their way while the workgroup meets at the barrier.  For the compiler to count the loads in flight (s_waitcnt vmcnt(4 (R - 1)), not
// vmcnt(0)) every load sits on ONE path: one cache policy for all of them, no branch around them (a position without an item loads
// from beyond the extent), and the strip indices are drawn by a STORER (waiting for an atomic's answer means waiting for every older
// load of the wave as well).
// Phases: in phase p the loaders fill T[p & 1] with the workgroup's p-th strip while the storers drain the (p-1)-th from T[(p-1) & 1].
template <int CA, int CB, int NL, int NS, int R, int AUX, int PRIO_L, int PRIO_S>
__global__ __launch_bounds__((NL + NS) * 64, 6) void k_binary_ws(const K1Args a)
{
    extern __shared__ uint64_t smem[];
    constexpr int RPW = SR / NS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ww = a.ww;
    const int PL = (SR + 4) * ww;
    uint64_t* const T0 = smem;
    uint64_t* const T1 = smem + PL;
    uint64_t* const Ew = smem + 2 * PL + (wave >= NL ? (wave - NL) * RPW * ww : 0);
    __shared__ uint64_t s_lut[256];
    __shared__ uint16_t s_spare[NL * 64];
    __shared__ int s_L[4];
    // ONE of these workgroups per CU, whatever the allocator finds: two (of consecutive batches, on the two pixel streams) would take
    // every wave slot of the CU and lock the sparse kernels of the batches in flight out until a whole launch has ended.  72 VGPRs
    // do that: 8 x 72 > 512, while 4 x 72 + the sparse kernel's 184 still fit.  (With the plane's delta stores the compiler takes 73,
    // allocated as 80: 8 x 80 > 512 and 4 x 80 + 184 = 504 <= 512 hold as well.)
    asm volatile("v_mov_b32 v71, 0" ::: "v71");
    if (tid < 256) s_lut[tid] = (uint64_t)expand4(tid) | ((uint64_t)expand4(tid >> 4) << 32);
    const int xcd = blockIdx.x & 7;
    const int per_xcd = (a.n_blocks + 7) >> 3;
    int* const head = a.strip_ctr + xcd * CTR_STRIDE;
    if (tid == 0) { // the workgroup's first two strips with ONE draw (one round trip to the memory side before anything can start)
        const int j0 = atomicAdd(head, 2);
        s_L[0] = j0;
        s_L[1] = j0 + 1;
    }
    const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(a.frames), 0, (int)((int64_t)(a.n_frames - 1) * a.frame_pitch + (int64_t)(a.h - 1) * a.stride + 3 * a.w), RSRC3);
    const __amdgpu_buffer_rsrc_t r_bin = __builtin_amdgcn_make_buffer_rsrc(a.binary, 0, a.binary ? (int)((int64_t)a.n_frames * a.w * a.h) : 0, RSRC3);
    const __amdgpu_buffer_rsrc_t r_plane = __builtin_amdgcn_make_buffer_rsrc(a.bits, 0, (int)((int64_t)a.n_frames * a.plane_pitch * 8), RSRC3);
    __syncthreads();
    auto strip_of = [&](int j) -> int {
        const int L = xcd * per_xcd + j;
        return ((uint32_t)j < (uint32_t)per_xcd && L < a.n_blocks) ? L : -1;
    };

    if (wave < NL) {
        // ------------------------------------------------------------------------------------------------ loader waves
        if (PRIO_L > 0) __builtin_amdgcn_s_setprio(PRIO_L);
        const int halo = a.morph, w = a.w, h = a.h;
        const int srh = SR + 2 * halo;
        const uint32_t lane_off = (uint32_t)lane * 12u;
        const uint32_t M1 = (lane & 1) ? 0xF0F0u : 0x0F0Fu, S1 = (lane & 1) ? 12u : 4u;
        const uint32_t P2 = (lane & 2) ? 0x0c0c0105u : 0x0c0c0400u;
        constexpr uint32_t OOB_S = 0xFFFFFC00u;
        const uint32_t px_total = (uint32_t)__umul24(srh, w);
        const int n_blk = (int)((px_total + 255u) >> 8);
        const int n_itl = (n_blk + 3) >> 2;              // items (1024 pixels) of a strip
        const int nbw = (n_itl + NL - 1) / NL;           // positions of a wave per strip: position b is item wave + NL b (if < n_itl)
        const int nbp = ((nbw + R - 1) / R) * R;         // ... padded to whole turns of the ring
        const bool ragged = (px_total & 1023u) != 0;
        const uint32_t lds_l = (uint32_t)(lane & 3) * 16u + (uint32_t)(lane >> 2);
        uint16_t* const spare = s_spare + tid;
        struct Geo { int L; uint32_t base, px_lo, px_span; bool whole; };
        auto geo_of = [&](int L) -> Geo {
            Geo g;
            g.L = L;
            if (L < 0) { g.base = 0; g.px_lo = 0; g.px_span = 0; g.whole = false; return g; }
            const int f = L / a.strips, strip = L - f * a.strips;
            const int y0 = strip * SR;
            const int rr_lo = max(0, halo - y0), rr_hi = min(srh, h - y0 + halo);
            g.base = (uint32_t)((int64_t)f * a.frame_pitch) + (uint32_t)(y0 - halo) * (uint32_t)a.stride;
            g.px_lo = (uint32_t)__umul24(rr_lo, w);
            g.px_span = (uint32_t)__umul24(rr_hi - rr_lo, w);
            g.whole = rr_lo == 0 && rr_hi == srh;
            return g;
        };
        auto item_of = [&](const Geo& g, int b) -> int { // the strip's item at position b of this wave, or -1
            const int j = wave + NL * b;
            if (g.L < 0 || j >= n_itl) return -1;
            return (g.L & 1) ? j : n_itl - 1 - j; // sweep direction: neighbouring strips meet at their shared rows
        };
        auto issue = [&](u32x3v (&v)[4], const Geo& g, int b) { // (no branch around the loads: a position without an item loads from beyond the extent)
            const int it = item_of(g, b);
            const uint32_t blk0 = (uint32_t)max(it, 0) * 4u;
            const uint32_t base = it >= 0 ? g.base + blk0 * 768u : OOB_S - 2304u;
            uint32_t vo[4];
#pragma unroll
            for (int k = 0; k < 4; k++) vo[k] = base + (uint32_t)k * 768u + lane_off;
            if (it >= 0 && (!g.whole || (ragged && it == n_itl - 1))) { // this lane's four pixels of block k: inside the strip's blocks and inside the image?
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t pix = (blk0 + (uint32_t)k) * 256u + (uint32_t)lane * 4u;
                    if ((int)(blk0 + k) >= n_blk || pix - g.px_lo >= g.px_span) vo[k] = OOB_S + lane_off;
                }
            }
            // ONE cache policy for every load, on one path: with a branch around the loads the compiler cannot count how many
            // younger loads are in flight and drains the ring before every item (s_waitcnt vmcnt(0))
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo[k], 0, AUX);
        };
        auto consume = [&](const u32x3v (&v)[4], const Geo& g, int b, uint64_t* T) {
            const int it = item_of(g, b);
            if (it < 0) return;
            const uint32_t d[12] = {v[0].x, v[0].y, v[0].z, v[1].x, v[1].y, v[1].z, v[2].x, v[2].y, v[2].z, v[3].x, v[3].y, v[3].z};
            const uint32_t m = thresh16<CA, CB>(d, a.lb);
            const uint32_t p1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xB1, 0xF, 0xF, true);
            const uint32_t t1 = (m & M1) | (((p1 << 8) >> S1) & ~M1);
            const uint32_t p2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)t1, 0x4E, 0xF, 0xF, true);
            const uint32_t t2 = __builtin_amdgcn_perm(p2, t1, P2);
            uint16_t* dst = reinterpret_cast<uint16_t*>(T) + (uint32_t)it * 64u + lds_l;
            // 16 pixels beyond the strip's last (the ragged end of its last item)
            if (ragged && (uint32_t)it * 1024u + (uint32_t)(lane & 3) * 256u + (uint32_t)(lane >> 2) * 16u >= px_total) dst = spare;
            *dst = (uint16_t)t2;
        };
        u32x3v ring[R][4];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int k = 0; k < 4; k++) ring[r][k] = u32x3v{0u, 0u, 0u};
        Geo gc = geo_of(strip_of(s_L[0]));
#pragma unroll
        for (int r = 0; r < R - 1; r++) issue(ring[r], gc, r); // (R - 1 <= nbp)
        for (int p = 0;; p++) {
            if (p > 0 && strip_of(s_L[(p - 1) & 3]) < 0) break;
            const Geo gn = geo_of(strip_of(s_L[(p + 1) & 3]));
            uint64_t* const T = (p & 1) ? T1 : T0;
            for (int b0 = 0; b0 < nbp; b0 += R) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int bi = b0 + r + R - 1;
                    issue(ring[(r + R - 1) % R], bi < nbp ? gc : gn, bi < nbp ? bi : bi - nbp);
                    consume(ring[r], gc, b0 + r, T);
                }
            }
            gc = gn;
            __syncthreads();
        }
    } else {
        // ------------------------------------------------------------------------------------------------ storer waves
        if (PRIO_S > 0) __builtin_amdgcn_s_setprio(PRIO_S);
        uint32_t m_ahead = ws_image_mask<NS>(a, strip_of(s_L[0]), wave - NL, lane); // the image's mask of the strip the loaders are filling
        for (int p = 0;; p++) {
            if (p > 0 && strip_of(s_L[(p - 1) & 3]) < 0) break;
            // the index for strip p+2 is drawn HERE, by a storer: waiting for an atomic's answer means waiting for every older load of
            // the wave as well, and a loader's ring would run empty once per strip
            if (tid == NL * 64) s_L[(p + 2) & 3] = atomicAdd(head, 1);
            if (p > 0) {
                const int Lp = strip_of(s_L[(p - 1) & 3]);
                m_ahead = ws_store_strip<NS>(a, Lp, ((p - 1) & 1) ? T1 : T0, Ew, s_lut, wave - NL, lane, r_bin, r_plane, m_ahead, strip_of(s_L[p & 3]));
            }
            __syncthreads();
        }
    }
    if (tid < 64) {
        int left = 0;
        if (tid == 0) left = atomicAdd(&a.strip_ctr[8 * CTR_STRIDE], 1);
        left = __builtin_amdgcn_readfirstlane(left);
        if (left == (int)gridDim.x - 1 && tid < 9) atomicExch(&a.strip_ctr[tid * CTR_STRIDE], 0);
    }
}
