// k_binary_kernel.inc -- the pixel kernel's body, compiled once per translation unit that includes it (k_binary.hip: K1_ENH 0, the kernel
// k_binary; k_binary_enh.hip: K1_ENH 1, k_binary_enh, the compare through the frame's threshold table).  The includer defines K1_KERNEL,
// K1_ENH, K1_THRESH(d) and K1_PASS(a, b) and has included k_binary_device.h.  k_binary_win.hip: K1_WIN 1, k_binary_win, every frame read at
// its window's effective origin (with K1_WIN 0 -- the default -- this file preprocesses to what it was before the switch existed).
#ifndef K1_WIN
#define K1_WIN 0
#endif
// k_binary_camp.hip / k_binary_camp_win.hip: K1_CAMP 1, k_binary_camp / k_binary_camp_win, per-frame detection keys -- every strip reads its
// frame's channel pair, bound and all-pass flag from a table (Bufs::key_eff) and runs phase 1 in the thresh16<CA, CB> / K1_PASS
// instantiation of that pair (with K1_CAMP 0 -- the default -- this file preprocesses to what it was before the switch existed).
#ifndef K1_CAMP
#define K1_CAMP 0
#endif

// Register budget: 6 waves per SIMD = at most 80 VGPRs.  Two launches of consecutive batches overlap (2 workgroups per CU each = 4
// waves per SIMD) next to one wave of the 4-wavefront sparse kernel (168 VGPRs): 4 x 80 + 168 <= 512.  At 88 the sparse kernel
// would no longer fit beside them and the batches in flight would take turns instead of sharing the CUs.
#if K1_CAMP
template <int FAST>
#else
template <int CA, int CB, int FAST /* 0: byte-wise loader, 1: row-quad items, 2: linear items (rows contiguous in memory) */>
#endif
#ifndef RMCV_K1_MINBLOCKS
#define RMCV_K1_MINBLOCKS 6
#endif
__global__ __launch_bounds__(256, RMCV_K1_MINBLOCKS) void K1_KERNEL(const uint8_t* __restrict__ frames, int64_t frame_pitch, int stride, int n_frames,
#if K1_CAMP
                                                 int w, int h, int ww, int, int /* the run's bound and flag: every strip takes its frame's */, int morph,
#else
                                                 int w, int h, int ww, int lb, int all_pass, int morph,
#endif
                                                 uint8_t* __restrict__ binary, uint64_t* __restrict__ bits, int prow,
                                                 int64_t plane_pitch, int strips, int n_blocks, uint32_t* __restrict__ rowmask,
                                                 int* __restrict__ strip_ctr, int taper_head, int taper_tail,
                                                 int halo_nt /* RMCV_OPT_PIXEL_HALO_NT */
#if K1_ENH
                                                 , const uint16_t* __restrict__ mtab /* [frame][256] Bufs::enh_m */
#endif
#if K1_WIN
                                                 , const rmcv_point* __restrict__ win_eff /* [frame] Bufs::win_eff; w, h are the window's */
                                                 , int in_extent /* bytes from `frames` to the end of the launch's last WHOLE frame */
#endif
#if K1_CAMP
                                                 , const FrameKey* __restrict__ keys /* [frame] Bufs::key_eff */
#endif
                                                 )
{
    extern __shared__ uint64_t smem[];
#ifdef RMCV_PROFILE_HANDOVER
    if (blockIdx.x == 0 && threadIdx.x == 0) printf("[kb start] %lld\n", (long long)wall_clock64());
#endif
#ifdef RMCV_K1_PRIO
    __builtin_amdgcn_s_setprio(RMCV_K1_PRIO); // dev knob (A/B of issue priorities against the sparse kernel's)
#endif
    const int halo = morph; // NONE 0, DILATE 1, CLOSE 2
    uint64_t* T = smem;
    uint64_t* D = smem + (size_t)(SR + 4) * ww;

    // Persistent workgroups: the grid is sized to a fixed number of workgroups per CU (leaving wave slots for the
    // sparse kernels of the previous batch that run on another stream) and every workgroup loops over strips.
    // XCD-aware order: workgroups b, b+8, b+16.. share an XCD; XCD x owns the contiguous strip range
    // [x*n/8, (x+1)*n/8) and its workgroups sweep it together, so neighbouring strips (which share halo rows)
    // are in flight on the same L2 at the same time.
    const int tid = threadIdx.x;
    const int wq = ww * 4; // 16-pixel groups per row
    const uint32_t r_wq = (uint32_t)((0x100000000ull + wq - 1) / wq), r_ww = (uint32_t)((0x100000000ull + ww - 1) / ww);
    const int xcd = blockIdx.x & 7; // gridDim.x is a multiple of 8
    const int per_xcd = (n_blocks + 7) >> 3;
    __shared__ int s_next;
    // A thread's items of a strip are tid, tid + 256, ...: their (row, group) pairs are stepped, not divided -- integer multiplies
    // (v_mul_lo/hi_u32) issue at a fraction of the rate of an add, and the FAST path is as much issue-bound as memory-bound
    const int q_first = tid - (int)div_r(tid, r_wq) * wq, r_first = div_r(tid, r_wq); // item tid = (r_first, q_first)
    const int q_step = 256 - (int)div_r(256, r_wq) * wq, r_step = div_r(256, r_wq);     // item + 256 = (r + r_step, q + q_step) or (r + r_step + 1, q + q_step - wq)
    const int k_first = tid - (int)div_r(tid, r_ww) * ww, s_first = div_r(tid, r_ww);   // the same for the strip's 64-pixel words
    const int k_step = 256 - (int)div_r(256, r_ww) * ww, s_step = div_r(256, r_ww);
    // 8 mask bits -> 8 bytes of 0/255: a 256-entry table in LDS instead of two multiplies per nibble (phase 4)
    __shared__ uint64_t s_lut[256];
    __shared__ uint16_t s_spare[256]; // where a lane without a place in the plane writes (no write sits behind a branch)
    if (FAST) s_lut[tid] = (uint64_t)expand4(tid) | ((uint64_t)expand4(tid >> 4) << 32);
#if K1_ENH
    __shared__ uint16_t s_m[256]; // the threshold table of the frame the strip belongs to
    int f_m = -1;
#endif
    int ticket = 0;
    if (tid == 0) ticket = atomicAdd(&strip_ctr[xcd * CTR_STRIDE], 1);
    for (;;) {
    // dynamic strip queue per XCD: a workgroup takes the next strip of its XCD's range when it is done with the previous
    // one, so CUs that also host kernels of another stream simply take fewer strips (a static split made them the tail)
    __syncthreads(); // also: the LDS planes of the previous strip are free
    // Every launch finds the heads at 0: the workgroup that leaves last zeroes them (below), so there is no memset per step
    // and no host-side mirror of device state that a failed or foreign launch could put out of step.
    // Pieces: the first taper_head and the last taper_tail strips of an XCD's range are handed out as four 8-row pieces each.
    // Used by launches with fewer strips than half the CUs (one camera frame: the per-frame drop-in chain), which hand out EVERY
    // strip that way; as a ramp / tail shortener of full batches it measured nothing (round 3) and is not offered any more.
    const int n_mid = per_xcd - taper_head - taper_tail;
    const int n_queue = 4 * taper_head + n_mid + 4 * taper_tail;
    // The ticket for THIS strip was drawn while the previous strip was being processed (`ticket`, thread 0); the next one is
    // drawn now and not looked at until the next iteration: a draw is a device-scope atomic -- a round trip of microseconds to the
    // memory side, which used to sit on every strip's critical path between two barriers.  (The queue heads are CTR_STRIDE ints
    // apart: eight heads in one cache line served every draw of every XCD one after the other.)
    if (tid == 0) {
        s_next = ticket;
        ticket = atomicAdd(&strip_ctr[xcd * CTR_STRIDE], 1);
    }
    __syncthreads();
    const int j = s_next;
    if ((uint32_t)j >= (uint32_t)n_queue) break;
    int s_local, piece = 0, sr = SR;
    if (j < 4 * taper_head) { s_local = j >> 2; piece = j & 3; sr = SR / 4; }
    else if (j < 4 * taper_head + n_mid) { s_local = taper_head + (j - 4 * taper_head); }
    else { const int jj = j - 4 * taper_head - n_mid; s_local = taper_head + n_mid + (jj >> 2); piece = jj & 3; sr = SR / 4; }
    const int L = xcd * per_xcd + s_local;
    if (L >= n_blocks) continue; // tail of the last XCD's range: draw on, so that every head advances alike
    const int f = L / strips, strip = L - f * strips;
    const int y0 = strip * SR + piece * (SR / 4);
    if (y0 >= h) continue; // a piece of the frame's last strip that lies below the image (h % SR <= 24): nothing to load or store
    const int srh = sr + 2 * halo;
#if K1_WIN
    // the window's first byte inside its frame (wave-uniform; x_eff is a multiple of 16 pixels, so 16-byte alignment survives)
    const uint32_t win_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)frame_origin_offset(win_eff, f, stride));
    const uint8_t* frame = frames + (int64_t)f * frame_pitch + win_off;
#else
    const uint8_t* frame = frames + (int64_t)f * frame_pitch;
#endif
#if K1_ENH
    // (every wave has left the previous strip's phase 1 -- two barriers ago -- so the table may change under nobody)
    if (f != f_m) { s_m[tid] = mtab[(int64_t)f * 256 + tid]; f_m = f; }
    __syncthreads();
#endif
#if K1_CAMP
    // the frame's key, once per strip (a workgroup's consecutive strips belong to different frames): wave-uniform, one scalar load; phase 1
    // below is then entered in the instantiation of the key's channel pair -- thresh16's selectors and register indices stay compile-time
    const FrameKey* const key = keys + __builtin_amdgcn_readfirstlane(f);
    const int key_ca = __builtin_amdgcn_readfirstlane(key->ca);
    const int lb = __builtin_amdgcn_readfirstlane(key->lb), all_pass = __builtin_amdgcn_readfirstlane(key->all_pass);
    // (the whole-frame row-quad loader takes w, ww and stride through a copy made opaque per strip: what its phase 1 derives from them is then
    // computed per strip on the scalar unit; hoisted out of the strip loop once per instantiation, three sets of loop invariants put that
    // loader alone one VGPR over the 80 -- 8 bytes of scratch.  The linear and the windowed loader fit as they are and are left alone.)
    int w_k = w, ww_k = ww, stride_k = stride;
    if (FAST == 1 && !K1_WIN) asm volatile("" : "+s"(w_k), "+s"(ww_k), "+s"(stride_k));
    auto phase1 = [&](auto ca_, auto cb_, const int w, const int ww, const int stride) __attribute__((always_inline)) {
    constexpr int CA = decltype(ca_)::value, CB = decltype(cb_)::value;
#endif

    // ---------------- phase 1: load + threshold -> T
    if (FAST) {
        // U items per wave per iteration: all 4*U loads are issued before the first threshold (memory-level
        // parallelism per wave); every 16-bit mask goes straight to its place in the LDS plane (ds_write_b16)
        constexpr int U = RMCV_K1_UNROLL;
        const int items = srh * wq;
#if K1_WIN
        // the extent covers whole frames: a ragged block's lanes beyond the window's row read the frame's pixels to its right (masked below)
        const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(frames), 0, in_extent, RSRC3);
        const uint32_t fbase = (uint32_t)((int64_t)f * frame_pitch) + win_off;
#else
        const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(frames), 0, (int)((int64_t)(n_frames - 1) * frame_pitch + (int64_t)(h - 1) * stride + 3 * w), RSRC3);
        const uint32_t fbase = (uint32_t)((int64_t)f * frame_pitch);
#endif
        // Wave-coalesced loads: an item is a 256-pixel block of FOUR rows; lane i loads pixels 4i..4i+3 of each row with one
        // dwordx3, so the wave reads 768 contiguous bytes = six whole cache lines per instruction and every line is touched by
        // exactly one instruction -- which is what lets the loads carry the non-temporal hint (round 2 measured it: per-lane
        // 48-byte loads touch a line with three instructions and lose 15-30 % with the hint; these gain 13 % with it,
        // profiles/r02d_k_binary_coalesced_x3.txt).  The 12 dwords of a lane are 16 whole pixels (thresh16): bit 4k+t = row k,
        // pixel 4i+t; the four lanes of a quad then transpose their 4x4 nibbles with two DPP exchanges, after which lane l of the
        // quad holds the 16 mask bits of row l and writes them with one ds_write_b16.  The item's (row quad, block) is
        // wave-uniform: its address arithmetic runs on the scalar unit.
        const int lane = tid & 63;
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int nb = (w + 255) >> 8, nq = (srh + 3) >> 2, n_it = nq * nb;
        const uint32_t r_nb = (uint32_t)((0x100000000ull + nb - 1) / nb);
        const uint32_t lane_off = (uint32_t)lane * 12u;
        const uint32_t lds_lane = (uint32_t)__umul24(lane & 3, ww) * 8u + (uint32_t)(lane >> 2) * 2u;
        const uint32_t M1 = (lane & 1) ? 0xF0F0u : 0x0F0Fu, S1 = (lane & 1) ? 12u : 4u;
        const uint32_t P2 = (lane & 2) ? 0x0c0c0105u : 0x0c0c0400u;
        constexpr uint32_t OOB_S = 0xFFFFFC00u; // scalar part of an offset that moves nothing (+ 63 * 12 stays out of extent)
        const int rr_lo = max(0, halo - y0), rr_hi = min(srh, h - y0 + halo); // the strip's rows that lie inside the image
        const uint32_t rr_span = (uint32_t)(rr_hi - rr_lo);
        const uint32_t strip_base = fbase + (uint32_t)(y0 - halo) * (uint32_t)stride; // wraps for the rows above the image: never used
        const int ragged = (w & 255) ? 1 : 0;
        const bool plain = rr_lo == 0 && rr_hi == srh && (srh & 3) == 0; // the strip's rows need no validity selects at all
        uint32_t dk1 = (uint32_t)stride, dk2 = 2u * (uint32_t)stride, dk3 = 3u * (uint32_t)stride;
        asm volatile("" : "+s"(dk1), "+s"(dk2), "+s"(dk3)); // opaque: otherwise every row's offset is re-derived with its own multiply
        if (all_pass) {
            int rq = r_first, q = q_first;
            for (int it = tid; it < items; it += 256) {
                const int y = y0 - halo + rq;
                reinterpret_cast<uint16_t*>(T + __umul24(rq, ww))[q] = (y >= 0 && y < h) ? 0xFFFFu : 0u;
                q += q_step;
                rq += r_step;
                if (q >= wq) { q -= wq; rq++; }
            }
        } else if (FAST == 2) {
            // LINEAR items (stride == 3 w: the strip's rows are ONE contiguous run in memory, as they are in the LDS plane since w % 64
            // == 0): the strip is a sequence of 256-pixel blocks -- block j = pixels [256 j, 256 j + 256) of that run = 768 contiguous
            // bytes = words [4 j, 4 j + 4) of T -- and an item is FOUR CONSECUTIVE blocks: the wave's four loads of an item read 3 KB
            // in one piece (row-quad items: four 768-byte pieces a row apart), and a row whose width is no multiple of 256 (1920 =
            // 7.5 blocks) wastes nothing: 270 blocks = 68 items per strip instead of 9 x 8 = 72 with every eighth half empty.
            // Lane i loads pixels 4 i .. 4 i + 3 of each block; after the quad transpose lane l of a quad holds 16 pixels of block l.
            const uint32_t px_total = (uint32_t)__umul24(srh, w);      // a multiple of 64; of 256 for the common sizes, not always of 1024
            const int n_blk = (int)((px_total + 255u) >> 8);
            const int n_itl = (n_blk + 3) >> 2;
            const uint32_t px_lo = (uint32_t)__umul24(rr_lo, w), px_span = (uint32_t)__umul24(rr_hi - rr_lo, w); // the run's pixels inside the image
            const uint32_t q_lo = (uint32_t)(4 * w), q_hi = (uint32_t)__umul24(srh - 4, w); // pixels of the first / last four rows: shared with the neighbours
            const bool whole = rr_lo == 0 && rr_hi == srh;             // every row of the strip is inside the image
            uint16_t* const T16 = reinterpret_cast<uint16_t*>(T);
            const uint32_t lds_l = (uint32_t)(lane & 3) * 16u + (uint32_t)(lane >> 2); // halfword of this lane's 16 pixels inside an item's 64 halfwords
            for (int it0 = wv; it0 < n_itl; it0 += 4 * U) {
                auto batch = [&](auto chk) {
                    constexpr bool CHK = decltype(chk)::value;
                    u32x3v v[U][4];
                    int itv[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int it_ = it0 + 4 * u;
                        const int it = (L & 1) ? it_ : n_itl - 1 - it_; // sweep direction: neighbouring strips meet at their shared rows
                        itv[u] = (CHK && it_ >= n_itl) ? -1 : it;
                        const uint32_t blk0 = (uint32_t)it * 4u;
#ifdef RMCV_K1_NOLOAD
                        const uint32_t base = OOB_S - 2304u;
#else
                        const uint32_t base = strip_base + blk0 * 768u;
#endif
                        uint32_t vo[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            vo[k] = base + (uint32_t)k * 768u + lane_off;
                            if (CHK) { // this lane's four pixels of block k: inside the strip's blocks and inside the image?
                                const uint32_t pix = (blk0 + (uint32_t)k) * 256u + (uint32_t)lane * 4u;
                                if (it_ >= n_itl || (int)(blk0 + k) >= n_blk || pix - px_lo >= px_span) vo[k] = OOB_S + lane_off;
                            }
                        }
                        const uint32_t p0 = blk0 * 256u;
                        if (halo && !halo_nt && (p0 < q_lo || p0 + 1024u > q_hi)) {
#pragma unroll
                            for (int k = 0; k < 4; k++) v[u][k] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo[k], 0, RMCV_K1_HALOAUX);
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; k++) v[u][k] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo[k], 0, RMCV_K1_LDAUX);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const uint32_t d[12] = {v[u][0].x, v[u][0].y, v[u][0].z, v[u][1].x, v[u][1].y, v[u][1].z,
                                                v[u][2].x, v[u][2].y, v[u][2].z, v[u][3].x, v[u][3].y, v[u][3].z};
                        const uint32_t m = K1_THRESH(d);
                        const uint32_t p1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xB1, 0xF, 0xF, true);
                        const uint32_t t1 = (m & M1) | (((p1 << 8) >> S1) & ~M1);
                        const uint32_t p2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)t1, 0x4E, 0xF, 0xF, true);
                        const uint32_t t2 = __builtin_amdgcn_perm(p2, t1, P2);
                        uint16_t* dst = T16 + (uint32_t)itv[u] * 64u + lds_l;
                        // an item beyond the strip's, or 16 pixels beyond the strip's last (the ragged end of its last item)
                        if (CHK && (itv[u] < 0 || (uint32_t)itv[u] * 1024u + (uint32_t)(lane & 3) * 256u + (uint32_t)(lane >> 2) * 16u >= px_total)) dst = s_spare + tid;
                        *dst = (uint16_t)t2;
                    }
                };
                // unchecked: every row inside the image, a full batch, and not the strip's last item if that one is ragged
                const bool has_last = (L & 1) ? (it0 + 4 * (U - 1) >= n_itl - 1) : (it0 == 0);
                if (whole && it0 + 4 * (U - 1) < n_itl && ((px_total & 1023u) == 0 || !has_last)) batch(std::false_type{});
                else batch(std::true_type{});
            }
        } else
        for (int it0 = wv; it0 < n_it; it0 += 4 * U) {
            // One batch = U items of the wave: all 4 * U loads are issued, then thresholded.  CHK = false is the common case (a strip
            // with every row inside the image, whole row quads, a full batch): no validity selects.
            auto batch = [&](auto chk) {
                constexpr bool CHK = decltype(chk)::value;
                u32x3v v[U][4];
                int info[U]; // LDS byte offset of the item's (row quad, block) | ragged-block flag; -1: beyond the strip's items
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int it = it0 + 4 * u; // wave-uniform: everything up to the four vector adds runs on the scalar unit
                    const int jq0 = div_r(it, r_nb), b = it - jq0 * nb;
                    const int jq = (L & 1) ? jq0 : nq - 1 - jq0; // sweep direction, see below
                    const int rr0 = 4 * jq;
                    info[u] = (int)(__umul24(rr0, ww) * 8u + (uint32_t)b * 32u) | (b == nb - 1 ? ragged : 0); // bit 0: ragged block
                    if (CHK && it >= n_it) info[u] = -1;
#ifdef RMCV_K1_NOLOAD
                    const uint32_t base = OOB_S - dk3; // ablation build: nothing is read
#else
                    const uint32_t base = strip_base + (uint32_t)rr0 * (uint32_t)stride + (uint32_t)b * 768u;
#endif
                    const uint32_t rowk[4] = {base, base + dk1, base + dk2, base + dk3};
                    uint32_t vo[4];
                    // rows rr_lo <= rr < rr_hi of the strip are inside the image; the others (and a whole item beyond the
                    // strip's) are "loaded" from beyond the extent: zeros, no traffic
                    const uint32_t t0 = (uint32_t)(rr0 - rr_lo), span = it < n_it ? rr_span : 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) vo[k] = (!CHK || t0 + (uint32_t)k < span ? rowk[k] : OOB_S) + lane_off;
                    // the first and the last row quad hold the rows this strip shares with its neighbours: those stay
                    // cacheable (the neighbour finds them in L2), everything else is read once and says so
                    // (RMCV_OPT_PIXEL_HALO_NT, a measurement knob: on some boxes the pixel kernels alone run at 0.2537 ms per launch
                    // with cacheable shared rows and at 0.2446 with the hint for them too, on the others the hint costs 1-5 %; the
                    // whole path hardly notices at 1280 px and loses 6 % at 1920 px: DESIGN.md 6g)
                    if (halo && !halo_nt && (jq == 0 || jq == nq - 1)) {
#pragma unroll
                        for (int k = 0; k < 4; k++) v[u][k] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo[k], 0, RMCV_K1_HALOAUX);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) v[u][k] = __builtin_amdgcn_raw_buffer_load_b96(r_in, vo[k], 0, RMCV_K1_LDAUX);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t d[12] = {v[u][0].x, v[u][0].y, v[u][0].z, v[u][1].x, v[u][1].y, v[u][1].z,
                                            v[u][2].x, v[u][2].y, v[u][2].z, v[u][3].x, v[u][3].y, v[u][3].z};
                    uint32_t m = K1_THRESH(d);
                    const bool last_ragged = (info[u] & 1) != 0; // wave-uniform: the row's last block when w % 256 != 0
                    // pixels beyond the row's end: the lane has read the next row's bytes
                    if (last_ragged && lane * 4 >= w - ((nb - 1) << 8)) m = 0;
                    // 4x4 nibble transpose within the quad: exchange with lane^1 (nibbles), then with lane^2 (bytes)
                    const uint32_t p1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xB1, 0xF, 0xF, true);
                    const uint32_t t1 = (m & M1) | (((p1 << 8) >> S1) & ~M1);
                    const uint32_t p2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)t1, 0x4E, 0xF, 0xF, true);
                    const uint32_t t2 = __builtin_amdgcn_perm(p2, t1, P2);
                    uint16_t* dst = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(T) + ((uint32_t)info[u] & ~1u) + lds_lane);
                    if (CHK && info[u] < 0) dst = s_spare + tid; // an item beyond the strip's
                    // the quad's 16 pixels of the last block may lie beyond the row: those go to a spare word
                    if (last_ragged && (lane >> 2) * 16 >= w - ((nb - 1) << 8)) dst = s_spare + tid;
                    *dst = (uint16_t)t2;
                }
            };
            if (plain && it0 + 4 * (U - 1) < n_it) batch(std::false_type{});
            else batch(std::true_type{});
        }
    } else {
        const int items = srh * wq;
        int rr = tid / wq, q = tid - rr * wq;
        const int dr = 256 / wq, dq = 256 - dr * wq;
        for (int it = tid; it < items; it += 256) {
            const int y = y0 - halo + rr;
            uint32_t m = 0;
            if (y >= 0 && y < h) {
                const uint8_t* row = frame + (int64_t)y * stride;
                for (int p = 0; p < 16; p++) {
                    int x = q * 16 + p;
                    if (x < w) {
                        int a = row[3 * x + CA], bb = row[3 * x + CB];
                        m |= (uint32_t)(all_pass || K1_PASS(a, bb)) << p;
                    }
                }
            }
            // merge the 4 lanes of a word (lanes are word-aligned: wq % 4 == 0, 256 % 4 == 0)
            uint32_t v = m << (16 * (q & 1));
            v |= __shfl_xor(v, 1);
            uint32_t o = __shfl_xor(v, 2);
            if ((q & 3) == 0) T[rr * ww + (q >> 2)] = ((uint64_t)o << 32) | v;
            rr += dr;
            q += dq;
            if (q >= wq) { q -= wq; rr++; }
        }
    }
#if K1_CAMP
    };
    // (frame_key_eff: channel A is 0 for B-R, 1 for G-R, 2 for R-B)
    if (key_ca == 1) phase1(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}, w_k, ww_k, stride_k);
    else if (key_ca == 0) phase1(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{}, w_k, ww_k, stride_k);
    else phase1(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, w_k, ww_k, stride_k);
#endif
    __syncthreads();

    const uint64_t last_valid = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull; // valid bits of the last word
    uint64_t* R = T; // plane holding the result rows, result row s at R[(s + halo) * ww + k]

    if (morph != RMCV_MORPH_NONE) {
        // ---------------- phase 2: dilate -> D (rows 1 .. srh-2)
        const int items = (srh - 2) * ww;
        int r_ = s_first, k = k_first; // (row, word) of item it, stepped (see the kernel's prologue)
        for (int it = tid; it < items; it += 256, k += k_step, r_ += s_step) {
            if (k >= ww) { k -= ww; r_++; }
            const int rr = 1 + r_;
            const int y = y0 - halo + rr;
            const int row = FAST ? (int)__umul24(rr, ww) : rr * ww;
            uint64_t d;
            if (y < 0 || y >= h) {
                d = ~0ull; // outside the image: never wins the erode
            } else {
                const uint64_t* t0 = T + row - ww;
                const uint64_t* t1 = T + row;
                const uint64_t* t2 = T + row + ww;
                uint64_t c = t0[k] | t1[k] | t2[k];
                uint64_t l = (k > 0) ? (t0[k - 1] | t1[k - 1] | t2[k - 1]) >> 63 : 0;
                uint64_t r = (k < ww - 1) ? (t0[k + 1] | t1[k + 1] | t2[k + 1]) & 1 : 0;
                d = c | (c << 1) | l | (c >> 1) | (r << 63);
                if (k == ww - 1) {
                    d &= last_valid;
                    if (morph == RMCV_MORPH_CLOSE) d |= ~last_valid; // columns >= w never win the erode
                }
            }
            D[row + k] = d;
        }
        __syncthreads();
        R = D;
        if (morph == RMCV_MORPH_CLOSE) {
            // ---------------- phase 3: erode -> T (rows 2 .. srh-3 = the strip)
            const int items3 = sr * ww;
            int r3 = s_first, k = k_first;
            for (int it = tid; it < items3; it += 256, k += k_step, r3 += s_step) {
                if (k >= ww) { k -= ww; r3++; }
                const int rr = 2 + r3;
                const int row = FAST ? (int)__umul24(rr, ww) : rr * ww;
                const uint64_t* d0 = D + row - ww;
                const uint64_t* d1 = D + row;
                const uint64_t* d2 = D + row + ww;
                uint64_t c = d0[k] & d1[k] & d2[k];
                uint64_t l = (k > 0) ? (d0[k - 1] & d1[k - 1] & d2[k - 1]) >> 63 : 1;
                uint64_t r = (k < ww - 1) ? (d0[k + 1] & d1[k + 1] & d2[k + 1]) & 1 : 1;
                uint64_t e = c & ((c << 1) | l) & ((c >> 1) | (r << 63));
                if (k == ww - 1) e &= last_valid;
                T[row + k] = e;
            }
            __syncthreads();
            R = T;
        }
    }

    // ---------------- row masks for the contour stage: bit k = word k of the row is non-zero
    if (ww <= 32 && tid < sr && y0 + tid < h) {
        uint32_t m = 0;
        for (int k = 0; k < ww; k++) m |= (uint32_t)(R[(tid + halo) * ww + k] != 0) << k;
        rowmask[(int64_t)f * h + y0 + tid] = m;
    }
    // ---------------- phase 4: expand to bytes + bit plane
    if (FAST) {
        const __amdgpu_buffer_rsrc_t r_bin = __builtin_amdgcn_make_buffer_rsrc(binary, 0, binary ? (int)((int64_t)n_frames * w * h) : 0, RSRC3);
        const __amdgpu_buffer_rsrc_t r_plane = __builtin_amdgcn_make_buffer_rsrc(bits, 0, (int)((int64_t)n_frames * plane_pitch * 8), RSRC3);
        const uint32_t plane_base = (uint32_t)((int64_t)f * plane_pitch);
        // ... and the two pad words behind every row's last word (always zero), so that the plane's cache lines are written whole (see
        // k_binary_ws.inc: with a 16-byte hole in every line the plane costs 3-15 % of the kernel once it falls out of the Infinity Cache)
        if (tid < sr && y0 + tid < h) {
            const u32x2v z = {0u, 0u};
            const uint32_t pp = (plane_base + __umul24(y0 + tid + 1, prow) + 1u + (uint32_t)ww) * 8u;
            __builtin_amdgcn_raw_buffer_store_b64(z, r_plane, pp, 0, RMCV_K1_PLAIN_PLAUX);
            __builtin_amdgcn_raw_buffer_store_b64(z, r_plane, pp + 8u, 0, RMCV_K1_PLAIN_PLAUX);
        }
        { // the strip's words -> the frame's bit plane (8 contiguous bytes per lane)
            const int nw = sr * ww;
            int s_ = s_first, k = k_first;
            for (int it = tid; it - (tid & 63) < nw; it += 256) {
                const int y = y0 + s_;
                const bool ok = it < nw && y < h;
                uint64_t word = 0;
                if (ok) word = R[__umul24(s_ + halo, ww) + k];
                const uint32_t po = ok ? (plane_base + __umul24(y + 1, prow) + 1u + (uint32_t)k) * 8u : OOB;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, word), r_plane, po, 0, RMCV_K1_PLAIN_PLAUX); // (plain: the sparse kernel of the same batch finds the words in L2)
                k += k_step;
                s_ += s_step;
                if (k >= ww) { k -= ww; s_++; }
            }
        }
        if (binary) { // RMCV_STAGE_NO_IMAGE: the 0/255 byte image is not wanted
            // w % 64 == 0: the strip's rows are contiguous both in the LDS plane (ww * 64 == w bits per row) and in the byte
            // image, so the strip is ONE run of 16-pixel items: no (row, group) bookkeeping, and the loop bound is wave-uniform
            const int n_valid = min(sr, h - y0) * wq;
            const uint16_t* R16 = reinterpret_cast<const uint16_t*>(R + __umul24(halo, ww));
            const uint32_t out0 = (uint32_t)((int64_t)f * w * h) + (uint32_t)y0 * (uint32_t)w;
            const int lane = tid & 63;
            for (int base = __builtin_amdgcn_readfirstlane(tid - lane); base < n_valid; base += 256) {
                const int it = base + lane;
                const bool ok = it < n_valid;
                const uint32_t m = R16[ok ? it : 0];
                const uint64_t lo = s_lut[m & 0xFF], hi = s_lut[m >> 8];
                const u32x4v o = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
#ifdef RMCV_K1_NOSTORE
                const uint32_t off = OOB;
#else
                const uint32_t off = ok ? out0 + (uint32_t)it * 16u : OOB;
#endif
                __builtin_amdgcn_raw_buffer_store_b128(o, r_bin, off, 0, RMCV_K1_STAUX /* nt: written once, read by nobody here */);
            }
        }
    } else {
        const int items = sr * wq;
        int s = tid / wq, q = tid - s * wq;
        const int dr = 256 / wq, dq = 256 - dr * wq;
        uint8_t* bin = binary ? binary + (int64_t)f * w * h : nullptr;
        uint64_t* plane = bits + (int64_t)f * plane_pitch;
        for (int it = tid; it < items; it += 256) {
            const int y = y0 + s;
            if (y < h) {
                const uint64_t word = R[(s + halo) * ww + (q >> 2)];
                const uint32_t m = (uint32_t)(word >> (16 * (q & 3))) & 0xFFFFu;
                if (binary) { // RMCV_STAGE_NO_IMAGE: the 0/255 byte image is not wanted, only the bit plane below
                    for (int p = 0; p < 16; p++) {
                        int x = q * 16 + p;
                        if (x < w) bin[(int64_t)y * w + x] = ((m >> p) & 1) ? 255 : 0;
                    }
                }
                if ((q & 3) == 0) {
                    plane[(int64_t)(y + 1) * prow + 1 + (q >> 2)] = word;
                }
            }
            s += dr;
            q += dq;
            if (q >= wq) { q -= wq; s++; }
        }
    }
    } // strip loop
    // Leaving: this workgroup has drawn its last index.  strip_ctr[8] counts the leavers; the last one of the launch knows that
    // nobody will draw again and zeroes the eight heads and the count for the next launch (launches of one context are ordered:
    // rmcv_host.hip chains them with an event when the caller changes streams).
#ifdef RMCV_PROFILE_HANDOVER
    if (tid == 0) printf("[kbx] %d %lld\n", xcd, (long long)wall_clock64()); // when this workgroup left: the XCDs' tails
#endif
    if (tid < 64) {
        int left = 0;
        if (tid == 0) left = atomicAdd(&strip_ctr[8 * CTR_STRIDE], 1);
        left = __builtin_amdgcn_readfirstlane(left);
        if (left == (int)gridDim.x - 1 && tid < 9) atomicExch(&strip_ctr[tid * CTR_STRIDE], 0);
#ifdef RMCV_PROFILE_HANDOVER
        if (left == (int)gridDim.x - 1 && tid == 0) printf("[kb end] %lld\n", (long long)wall_clock64());
#endif
    }
}
