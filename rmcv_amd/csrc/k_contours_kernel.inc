// k_contours_kernel.inc -- the body of the per-frame sparse kernel (findContours + the fused filter_lightblobs / filter_armours
// tail), included by k_contours.hip once per workgroup size: KC_KERNEL = kernel name, KC_THREADS = 512 or 256.  (Two textual
// copies instead of a template: as a template the two instantiations shared out-of-line copies of the big device functions,
// which cost 21 VGPRs and a stack frame -- enough to lose the co-residency with the pixel kernel the 8-wavefront form relies on.)
#define CT_THREADS KC_THREADS
#ifndef RMCV_KC_ATTR
#define RMCV_KC_ATTR // dev knob: e.g. -DRMCV_KC_ATTR='__attribute__((amdgpu_waves_per_eu(4,4)))' caps the kernel at 128 VGPRs (and spills)
#endif
__global__ __launch_bounds__(CT_THREADS) RMCV_KC_ATTR void KC_KERNEL(const uint64_t* __restrict__ bits, const uint32_t* __restrict__ rowmasks,
                                                        int rm_pitch, uint64_t* lab, uint64_t* neg, int w, int h, int ww, int prow,
                                                        int64_t plane_pitch, rmcv_point* points, int32_t* cont_start,
                                                        int32_t* cont_len, int32_t* n_contours, int32_t* n_points,
                                                        int32_t* status, int max_contours, int max_points, int force_literal,
                                                        int32_t* __restrict__ elig, int32_t* __restrict__ n_elig,
                                                        int32_t* __restrict__ slot_kind, SparseTail X, uint32_t* __restrict__ visit_xy,
                                                        uint8_t* __restrict__ mid_base, int64_t mid_stride, int mid_slot_cap, SparseSched Q, int rows_cap)
{
    extern __shared__ unsigned long long smem_raw[];
    // Issue priority 3: the kernel is latency-bound and issues ahead of the streaming pixel kernel of the next batch that shares the
    // CU (0-2 measured nothing or worse in round 3, by alternating regions of one process)
#ifndef RMCV_KC_PRIO
#define RMCV_KC_PRIO 3
#endif
    __builtin_amdgcn_s_setprio(RMCV_KC_PRIO);
    ContoursLds& S = *reinterpret_cast<ContoursLds*>(smem_raw);
    const RowTabs RT = row_tabs(smem_raw, rows_cap); // the row tables lie behind the struct, sized by the frame's height
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    enum { FL_COMPLEX = 1, FL_MID = 2 }; // the frame needs the literal scanner / is beyond the LDS tables (mid tier)
    // Workgroup b takes frame order[b]: the frames in the order k_binary completes them, interleaved over the XCDs the way workgroups
    // are dealt to them (rmcv_host.hip: frame_order), so the hardware's own dispatch order is "next frame to become ready, on the
    // XCD whose L2 its planes were written through".
    const int f = Q.order ? Q.order[blockIdx.x] : (int)blockIdx.x;
#ifdef RMCV_PROFILE_HANDOVER
    const long long th0_ = wall_clock64(), th1_ = th0_;
#endif
    // Two-launch form for dense frames (k_contours.hip: launch_contours_x): the 4-wavefront launch does not walk a frame that is
    // beyond its LDS tables -- it marks it RMCV_FRAME_DEFERRED_ and leaves --, and a launch of the 8-wavefront kernel behind it takes
    // the marked frames only (a workgroup of any other frame reads one word and ends).
    const bool defer_mid = (force_literal & 4) != 0, deferred_only = (force_literal & 8) != 0;
    force_literal &= 3;
    if (deferred_only && status[f] != RMCV_FRAME_DEFERRED_) return;
    const uint64_t* F = bits + (int64_t)f * plane_pitch;
    uint64_t* LAB = lab + (int64_t)f * plane_pitch;
    uint64_t* NEG = neg + (int64_t)f * plane_pitch;
    rmcv_point* pts = points + (int64_t)f * max_points;
    int32_t* cs = cont_start + (int64_t)f * max_contours;
    int32_t* cl = cont_len + (int64_t)f * max_contours;
#if defined(RMCV_PROFILE) || defined(RMCV_PROFILE_HANDOVER)
    long long t_[8]; int ti_ = 0;
#define STAMP() do { __syncthreads(); if (ti_ < 8) t_[ti_++] = wall_clock64(); } while (0)
#else
#define STAMP() do {} while (0)
#endif
    STAMP();
    const bool summarised = (h <= rows_cap && ww <= 32);
    if (tid == 0) {
        S.nkept = 0; S.cursor = 0; S.nrows = 0; S.nslots = 0; S.nelig = 0;
        S.flags = (force_literal == 1 || !summarised) ? FL_COMPLEX : (force_literal == 2 ? FL_MID : 0);
    }
    // ---------------- row tables: masks from k_binary, slot bases by a workgroup prefix sum, list of non-empty rows
    if (summarised) {
        const int per = (h + CT_THREADS - 1) / CT_THREADS; // consecutive rows per thread
        int cnt = 0;
        // the masks of a thread's rows are loaded TOGETHER (summarised: h <= CT_MAXH, so at most CT_MAXH / 256 rows per thread): one
        // global round trip instead of one per row -- each costs microseconds while other batches stream through the memory system
        constexpr int MAXPER = (CT_MAXH + CT_THREADS - 1) / CT_THREADS; // = the largest `per` a summarised frame can have
        uint32_t mrow[MAXPER];
#pragma unroll
        for (int u = 0; u < MAXPER; u++) {
            const int y = tid * per + u;
            mrow[u] = (u < per && y < h) ? rowmasks[(int64_t)f * rm_pitch + y] : 0u;
        }
#pragma unroll
        for (int u = 0; u < MAXPER; u++) {
            const int y = tid * per + u;
            if (u < per && y < h) RT.rowmask[y] = mrow[u];
            cnt += __popc(mrow[u]);
        }
        S.scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < CT_THREADS; d <<= 1) { // Hillis-Steele inclusive scan
            const int v = tid >= d ? S.scan[tid - d] : 0;
            __syncthreads();
            S.scan[tid] += v;
            __syncthreads();
        }
        int base = S.scan[tid] - cnt;
        for (int u = 0; u < per; u++) {
            const int y = tid * per + u;
            if (y < h) {
                const uint32_t m = RT.rowmask[y];
                RT.rowbase[y] = (uint16_t)(base < 65535 ? base : 65535);
                base += __popc(m);
                if (m) RT.rows[atomicAdd(&S.nrows, 1)] = (uint16_t)y;
            }
        }
        if (tid == CT_THREADS - 1) {
            S.nslots = S.scan[tid];
            if (S.scan[tid] > SLOT_CAP) S.flags |= FL_MID;
        }
    }
    __syncthreads();
    const int nrows = S.nrows;
    // (no zeroing of the label planes here: cycles_frame uses their storage for the words' border masks first and zeroes it when the
    // labels move in, at the head of every round of N7)
    LabelStore LS;
    LS.rowmask = RT.rowmask;
    LS.rowbase = RT.rowbase;
    LS.lab = S.lab;
    LS.neg = S.neg;
    STAMP();

    // ---------------- C: borders as cycles of visits
    if (!S.flags) cycles_frame<CT_THREADS>(S, RT, F, prow, h, ww, nrows, tid, pts, max_points, max_contours, FL_COMPLEX, FL_MID, visit_xy + (int64_t)f * NN_CAP);
    __syncthreads();
    STAMP();
    // ---------------- V: verification against the merged labels (all in LDS)
    const int nkept = S.nkept;
    if (!S.flags) {
        // V1: every kept start was acceptable: nearest labelled pixel to its left is negative, or there is none
        for (int e = tid; e < nkept; e += CT_THREADS) {
            const uint32_t key = S.kkey[e];
            const int x0 = (int)(key & 0xFFFFu), y0 = (int)(key >> 16);
            const uint32_t occ = RT.rowmask[y0];
            int k = x0 >> 6;
            unsigned long long l = S.lab[LS.slot(y0, k)] & ((1ull << (x0 & 63)) - 1);
            uint32_t left = occ & ((1u << k) - 1u);
            while (!l && left) {
                k = 31 - __clz((int)left);
                left &= ~(1u << k);
                l = S.lab[LS.slot(y0, k)];
            }
            if (l) {
                const int top = 63 - __clzll((long long)l);
                if (!((S.neg[LS.slot(y0, k)] >> top) & 1ull)) atomicOr(&S.flags, FL_COMPLEX);
            }
        }
        // V2: every unlabelled run start would have been rejected
        for (int r = tid; r < nrows; r += CT_THREADS) {
            const int y = RT.rows[r];
            const int64_t base = (int64_t)(y + 1) * prow + 1;
            const uint32_t occ = RT.rowmask[y];
            int slot = RT.rowbase[y];
            uint64_t carry = 0;
            bool last_pos = false;
            // the row's non-empty words, four at a time: their loads are issued together (a word's carry needs its left neighbour
            // only when that one is non-empty too, i.e. the previous word of the walk)
            uint32_t rem = occ;
            int kprev = -2;
            while (rem) {
                int kk[4];
                uint64_t fw[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    kk[i] = rem ? __ffs((int)rem) - 1 : -1;
                    if (rem) rem &= rem - 1;
                    fw[i] = kk[i] >= 0 ? F[base + kk[i]] : 0ull;
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (kk[i] < 0) break;
                    const uint64_t fwd = fw[i];
                    if (kk[i] != kprev + 1) carry = 0;
                    kprev = kk[i];
                    const unsigned long long l = S.lab[slot], ng = S.neg[slot];
                    slot++;
                    uint64_t cand = fwd & ~((fwd << 1) | carry) & ~l;
                    while (cand) {
                        const int b = __ffsll((long long)cand) - 1;
                        cand &= cand - 1;
                        const uint64_t below = l & ((1ull << b) - 1);
                        const bool pos = below ? !((ng >> (63 - __clzll((long long)below))) & 1ull) : last_pos;
                        if (!pos) atomicOr(&S.flags, FL_COMPLEX);
                    }
                    if (l) last_pos = !((ng >> (63 - __clzll((long long)l))) & 1ull);
                    carry = fwd >> 63;
                }
            }
        }
    }
    __syncthreads();
    STAMP();
    // ---------------- M: a frame beyond the LDS tables -- the same formulation on the workgroup's scratch block in global memory
    if (defer_mid && (S.flags & FL_MID) && !(S.flags & FL_COMPLEX) && summarised && mid_base) {
        if (tid == 0) status[f] = RMCV_FRAME_DEFERRED_; // every list of this frame is written by the launch that follows
        return;
    }
    if ((S.flags & FL_MID) && !(S.flags & FL_COMPLEX) && summarised && mid_base) {
        __syncthreads();
        if (tid == 0) S.flags = 0;
        __syncthreads();
        const MidTables M = mid_tables(mid_base + (int64_t)f * mid_stride, mid_slot_cap);
        int nc = 0, np = 0;
        cycles_frame_mid<CT_THREADS>(S, RT, M, F, prow, h, ww, nrows, tid, pts, cs, cl, max_points, max_contours, FL_COMPLEX, &nc, &np);
        __syncthreads();
        if (tid == 0) {
            if (S.flags & FL_COMPLEX) S.flags = FL_COMPLEX;
            else { S.flags = FL_MID; S.lit[0] = nc; S.lit[1] = np; S.lit[2] = RMCV_FRAME_MID_PATH; }
        }
        __syncthreads();
    } else if (S.flags & FL_MID) { // no scratch (or not summarised): the literal scanner
        __syncthreads();
        if (tid == 0) S.flags = FL_COMPLEX;
        __syncthreads();
    }
    const bool literal = (S.flags & FL_COMPLEX) != 0;
    const bool complex = S.flags != 0; // the frame's lists are in global memory only (mid tier or literal scanner)

    if (complex) {
        if (literal) {
        // ---------------- F: literal scanner (one wavefront), exact for nested components
        if (wave == 0) {
            int nc, np, st;
            literal_frame(lane, F, LAB, NEG, h, ww, prow, pts, cs, cl, max_contours, max_points,
                          summarised ? RT.rowmask : nullptr, &nc, &np, &st);
            if (lane == 0) { S.lit[0] = nc; S.lit[1] = np; S.lit[2] = st | RMCV_FRAME_SLOW_PATH; }
        }
        __threadfence();
        __syncthreads();
        // the literal scanner labels in the global planes: clear what it set (labels only exist where F is set)
        for (int y = tid; y < h; y += CT_THREADS) {
            const int64_t base = (int64_t)(y + 1) * prow + 1;
            const uint32_t occ = summarised ? RT.rowmask[y] : ~0u;
            for (int k = 0; k < ww; k++)
                if ((k >= 32 || ((occ >> k) & 1u)) && F[base + k]) { LAB[base + k] = 0; NEG[base + k] = 0; }
        }
        }
        { // work list of the fit stage: contours with at least 6 points (objdetect.cpp:64); the others are "skipped"
            const int nc = S.lit[0];
            int32_t* el = elig + (int64_t)f * max_contours;
            for (int k = tid; k < nc; k += CT_THREADS) {
                if (cl[k] >= 6) el[atomicAdd(&S.nelig, 1)] = k;
                else slot_kind[(int64_t)f * max_contours + (nc - 1 - k)] = 0;
            }
        }
        __syncthreads();
        if (tid == 0) {
            n_contours[f] = S.lit[0];
            n_points[f] = S.lit[1];
            n_elig[f] = S.nelig;
            status[f] = S.lit[2];
        }
    } else {
    STAMP();
#ifdef RMCV_PROFILE
    if (tid == 0 && (f == 0 || f == 100))
        printf("[f%d] rows=%d slots=%d nodes=%d kept=%d pts=%d | tables %.1f cycles %.1f V %.1f us\n", f, nrows, S.nslots, S.nnodes,
               nkept, S.cursor, (t_[1] - t_[0]) / 100.0, (t_[2] - t_[1]) / 100.0, (t_[3] - t_[2]) / 100.0);
#endif
    // discovery order = raster order of the starts: rank the kept entries by key
    for (int e = tid; e < nkept; e += CT_THREADS) {
        const uint32_t key = S.kkey[e];
        int rank = 0;
        for (int j = 0; j < nkept; j++) rank += S.kkey[j] < key;
        cs[rank] = S.koff[e];
        cl[rank] = S.klen[e];
        // work list of the fit stage: contours with at least 6 points (objdetect.cpp:64); the others are "skipped".  A copy of
        // the entry (discovery index, start, length) stays in LDS for the fused tail (the node tables are free again)
        if (S.klen[e] >= 6) {
            const int pos = atomicAdd(&S.nelig, 1);
            elig[(int64_t)f * max_contours + pos] = rank;
            S.n_d[pos] = (uint16_t)rank;
            S.w_off[pos] = (uint32_t)S.koff[e];
            S.w_cnt[pos] = (uint32_t)S.klen[e];
        } else slot_kind[(int64_t)f * max_contours + (nkept - 1 - rank)] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        n_contours[f] = nkept;
        n_points[f] = S.cursor;
        n_elig[f] = S.nelig;
        status[f] = 0;
    }
    }
#if defined(RMCV_PROFILE) || defined(RMCV_PROFILE_HANDOVER)
    const long long tt0_ = wall_clock64();
#endif
    if (!X.fused) return;
    // ---------------- fused tail: rm::filter_lightblobs + rm::filter_armours of THIS frame in the same workgroup, so a batch
    // has one sparse launch and a frame's stages follow each other without waiting for the slowest frame of every stage.
    // The 8 wavefronts take the contours of the work list (one contour each at a time), then wavefront 0 compacts and pairs.
    __syncthreads(); // the lists this workgroup wrote to global memory are visible to all of its wavefronts
    const int nc = complex ? S.lit[0] : S.nkept;
    const int ne_all = S.nelig;
    // (a mid-tier or literal-path frame can have thousands of eligible contours: the all-pairs ranking below is kept to the first
    // 1024 of them, the rest goes unsorted)
    // (the sorted part keeps 16-bit contour indices)
    const int ne_cap = !complex ? NN_CAP : (nc > 65535 ? 0 : 1024);
    const int ne = ne_all > ne_cap ? ne_cap : ne_all;
    // work list sorted by contour length, longest first, and pulled dynamically: the long fits (the general-conic fallback of
    // > ~200-point contours takes twice as long as a direct fit) start first instead of ending up behind another fit
    const int32_t* el = elig + (int64_t)f * max_contours;
    uint16_t* const w_len = S.n_b;  // the node tables are free again (and lie beyond the fit's wave-private rows)
    uint16_t* const w_idx = S.n_d;
    uint16_t* const w_sorted = S.n_a;
    const uint32_t* const w_off = S.w_off;   // cycle path: starts and lengths of the work
    const uint32_t* const w_cnt = S.w_cnt;   // list's contours (<= KEPT_CAP entries)
    static_assert(KEPT_CAP <= NN_CAP, "the work list fits the node tables");
    for (int e = tid; e < ne; e += CT_THREADS) {
        int len;
        if (complex) { // the literal scanner wrote its lists to global memory only
            const int k = el[e];
            len = cl[k];
            w_idx[e] = (uint16_t)k;
        } else len = (int)w_cnt[e];
        w_len[e] = (uint16_t)(len > 65535 ? 65535 : len);
    }
    if (tid == 0) S.wnext = 0;
    __syncthreads();
    for (int e = tid; e < ne; e += CT_THREADS) {
        const int len = w_len[e];
        int rank = 0;
        for (int j = 0; j < ne; j++) rank += (w_len[j] > len) || (w_len[j] == len && j < e);
        w_sorted[rank] = (uint16_t)e; // position in the work list
    }
    __syncthreads(); // also: everybody has read the counters, the contour tables make room for the fit's wave-private rows
    {
        static_assert(offsetof(ContoursLds, n_a) >= (CT_THREADS_MAX / 64) * sizeof(WaveLds), "the work list must outlive the tables");
        static_assert(offsetof(ContoursLds, w_off) >= (CT_THREADS_MAX / 64) * sizeof(WaveLds), "... and so must its LDS copies of starts / lengths");
        WaveLds& L = reinterpret_cast<WaveLds*>(smem_raw)[wave];
        for (;;) {
            const int got = atomicAdd(lane == 0 ? &S.wnext : &S.sink[lane], lane == 0 ? 1 : 0); // every lane issues the atomic
            const int e = __shfl(got, 0);
            if (e >= ne_all) break;
            if (!complex) { // everything the fit needs to find its points is in LDS
                const int pos = w_sorted[e];
                fit_contour_slot_at(f, (int)w_idx[pos], nc, pts, (int)w_off[pos], (int)w_cnt[pos], max_contours, max_points, X.G, slot_kind,
                                    X.slot_ell, L, lane);
            } else {
                const int k = e < ne ? (int)w_idx[w_sorted[e]] : el[e];
                fit_contour_slot(f, k, nc, pts, cs, cl, max_contours, max_points, X.G, slot_kind, X.slot_ell, L, lane);
            }
        }
    }
    __syncthreads();
#if defined(RMCV_PROFILE) || defined(RMCV_PROFILE_HANDOVER)
    const long long tt1_ = wall_clock64();
#endif
    if (wave == 0) {
        const FitTail& T = X.T;
        const int enemy = tail_enemy(T, f);
        const int np = blob_compact_frame(f, lane, slot_kind, X.slot_ell, nc, max_contours, enemy, T.blobs, T.blob_src, T.ellipses,
                                          T.neg_idx, T.n_blobs, T.n_neg, T.status, T.max_blobs);
        if (T.do_pairs) {
            // the pair loop re-reads, across lanes, the blobs this wave has just written: workgroup scope is enough (one CU, one L1) -- at
            // device scope the fence is an L2 write-back + invalidate (buffer_wbl2 sc1, buffer_inv sc1) per frame, on the XCD whose
            // L2 the pixel kernels of the other batches are streaming through: it cost the step 3 % (DESIGN.md 6g)
            __threadfence_block();
            armours_frame(f, lane, T.blobs, np, T.max_blobs, T.angle_diff_max, T.shear_max, T.length_ratio_max, enemy, T.armours,
                          T.n_armours, T.status, T.max_armours, T.ov);
        }
    }
#ifdef RMCV_PROFILE
    __syncthreads();
    if (tid == 0 && blockIdx.x < 2) printf("[tail b%d] eligible %d of %d contours: fits %.1f us, compaction + pairing %.1f us\n", (int)blockIdx.x, ne_all, nc, (tt1_ - tt0_) / 100.0, (wall_clock64() - tt1_) / 100.0);
#endif
#ifdef RMCV_PROFILE_HANDOVER
    __syncthreads();
    if (tid == 0) // frame, start, frame ready, done | tables, cycles, verification + ranking, fits, compaction + pairing (us)
        printf("[sp] %d %lld %lld %lld | %.1f %.1f %.1f %.1f %.1f | elig %d\n", f, th0_, th1_, (long long)wall_clock64(), (t_[1] - t_[0]) / 100.0,
               (t_[2] - t_[1]) / 100.0, (tt0_ - t_[2]) / 100.0, (tt1_ - tt0_) / 100.0, (wall_clock64() - tt1_) / 100.0, ne_all);
#endif
#ifndef KC_NO_CLASSIFY // (the lean build's LDS has no room for the feature rows: its launcher never takes classifier batches)
    if (X.C.enabled) {
        // ---------------- executable/main.cpp:178-181 for this frame's armours: icon rectification + flatten + SVM vote, one
        // wavefront per armour (device_classify.h); the features live in the LDS the contour tables no longer need
        __threadfence_block();
        __syncthreads(); // wavefront 0's armours and their count are visible to the others
        constexpr int NW = CT_THREADS / 64;
        static_assert((CT_THREADS_MAX / 64) * sizeof(WaveLds) + NW * (NFEAT * sizeof(float) + 32 * sizeof(double)) <= sizeof(ContoursLds), "feature rows fit");
        unsigned char* base = reinterpret_cast<unsigned char*>(smem_raw) + (CT_THREADS_MAX / 64) * sizeof(WaveLds);
        double* sums = reinterpret_cast<double*>(base) + wave * 32;
        float* feat = reinterpret_cast<float*>(base + NW * 32 * sizeof(double)) + wave * NFEAT;
        int na = X.T.n_armours[f];
        if (na > X.T.max_armours) na = X.T.max_armours;
        classify_frame(f, lane, wave, NW, na, X.C, X.T.armours, X.T.max_armours, feat, sums);
    }
#endif
}

#undef CT_THREADS
