// k_binary_launch.inc -- the launcher of the kernel k_binary_kernel.inc has just defined: geometry -> loader form, chunks of frames below
// 4 GiB, the persistent grid.  The includer defines K1_LAUNCH_T and K1_EXTRA (trailing kernel arguments); with K1_ENH 0 it has also
// included k_binary_ws.inc and defined g_ws_launches.  K1_WIN (k_binary_win.hip): window rows are not contiguous -- never the linear
// loader, never k_binary_ws; FAST 2 is not even instantiated.
// img (nullable; the K1_ENH 0, K1_WIN 0 build alone reads it): what the context knows about its byte image (image_plan.h).  It decides how
// k_binary_ws stores the image and is rewritten once every chunk has been enqueued -- or left UNKNOWN by an error.
#ifndef K1_WIN
#define K1_WIN 0
#endif
// K1_CAMP (k_binary_camp.hip, k_binary_camp_win.hip): per-frame detection keys -- the launcher is no template (the kernel picks the channel pair
// per strip), `lower_bound` is ignored, K1_EXTRA carries the launch's slice of Bufs::key_eff; k_binary's shape, never k_binary_ws.
#ifndef K1_CAMP
#define K1_CAMP 0
#endif
#if K1_CAMP
#define K1_INST(F) K1_KERNEL<F>
#else
#define K1_INST(F) K1_KERNEL<CA, CB, F>
template <int CA, int CB>
#endif
static hipError_t K1_LAUNCH_T(const Geom& g, const Bufs& b, int lower_bound, int morph, bool image, const RunPlan& plan,
                                  hipStream_t s, ImageState* img = nullptr)
{
    const int strips = (g.h + SR - 1) / SR;
    int lb = lower_bound, all_pass = 0;
    if (lb <= 0) { all_pass = 1; lb = 1; }
    if (lb > 256) lb = 256;
    const size_t planes = (size_t)2 * (SR + 4) * g.ww * sizeof(uint64_t);
    const bool aligned = (g.w % 64 == 0) && (g.stride % 16 == 0) && (g.frame_pitch % 16 == 0) && ((uintptr_t)b.frames % 16 == 0);
    // The FAST path addresses its buffers with 32-bit offsets, so one launch covers at most as many frames as keep every extent
    // (input, byte image, bit plane) below 4 GiB - 256; a larger batch (288 GB of HBM hold 70 000 frames) is a few launches in a
    // row on the same stream, each with its pointers advanced -- not a fall-back to the byte-wise loader.
    const int64_t lim = 0xFFFFF000ll;
    const int64_t per_frame = std::max<int64_t>(std::max<int64_t>(g.frame_pitch, g.plane_pitch * 8), (int64_t)g.w * g.h);
    const int chunk = aligned ? (int)std::min<int64_t>(g.n_frames, std::max<int64_t>(1, (lim - 1) / per_frame)) : g.n_frames;
    const bool fast = aligned && (int64_t)chunk * per_frame < lim;
    // rows contiguous in memory: the linear loader (Geom::pixel_rowquad, hidden option 1001: the row-quad loader everywhere -- for A/B runs)
#if K1_WIN
    const bool linear = false;
#else
    const bool linear = fast && !g.pixel_rowquad && g.stride == 3 * g.w;
#endif
    // persistent grid: RMCV_OPT_PIXEL_GROUPS workgroups per CU: alone the kernel is equally fast with 2 and 3 and slower with 4 and
    // more; 2 leaves room on every CU for the kernels of the other batches in flight
    const int bpc = plan.pixel_groups;
#if !K1_ENH && !K1_WIN && !K1_CAMP
    // the chunks of a batch share one state: the mode from what held before the batch, the next state from what all of them ran as
    const ImageState img_before = img ? *img : IMAGE_STATE_UNKNOWN;
    const ImageLaunch img_launch = {IMAGE_KERNEL_WS, image, g.w, g.h, g.ww, g.n_frames};
    const ImageMode img_mode = image_step(img_before, img_launch, true).mode;
    bool all_ws = true;
    if (img) *img = image_step(img_before, img_launch, false).next; // (until every chunk is enqueued: what an error return leaves behind)
#endif
    for (int f0 = 0; f0 < g.n_frames; f0 += chunk) {
        const int nf = std::min(chunk, g.n_frames - f0);
        const int n_blocks = nf * strips;
        int grid = (g.n_cu > 0 ? g.n_cu : 256) * (bpc > 0 ? bpc : 4); // n_cu: of the context's own device
        if (grid > ((n_blocks + 7) & ~7)) grid = (n_blocks + 7) & ~7;
        grid = (grid + 7) & ~7;
        const int per_xcd = (n_blocks + 7) >> 3;
        int taper_head = 0, taper_tail = 0;
        // A launch with fewer strips than half the CUs (one camera frame = 32 strips on 256 CUs: the per-frame drop-in chain) hands
        // EVERY strip out as four 8-row pieces: four times the workgroups, a quarter of the rows each (15 -> 7 us for one frame).
        if (n_blocks * 2 <= (g.n_cu > 0 ? g.n_cu : 256)) {
            taper_head = per_xcd;
            taper_tail = 0;
            grid = (4 * n_blocks + 7) & ~7;
        }
        const uint8_t* frames = b.frames + (int64_t)f0 * g.frame_pitch;
        uint8_t* binary = image ? b.binary + (int64_t)f0 * g.w * g.h : nullptr;
        uint64_t* bits = b.bits + (int64_t)f0 * g.plane_pitch;
        uint32_t* rowmask = b.rowmask + (int64_t)f0 * g.h;
        // beyond 64 KiB of dynamic LDS (frames wider than ~6700 pixels) the kernel has to be told; per device and instantiation
        static size_t lds_set[MAX_DEVICES][3] = {};
        const int mode = fast ? (linear ? 2 : 1) : 0;
        const int inst = mode;
        if (planes > 60 * 1024 && planes > lds_set[g.device][inst]) {
#if K1_WIN
            const void* fn = mode == 1 ? reinterpret_cast<const void*>(K1_INST(1)) : reinterpret_cast<const void*>(K1_INST(0));
#else
            const void* fn = mode == 2 ? reinterpret_cast<const void*>(K1_INST(2)) : mode == 1 ? reinterpret_cast<const void*>(K1_INST(1)) : reinterpret_cast<const void*>(K1_INST(0));
#endif
            const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes);
            if (ea != hipSuccess) return ea;
            lds_set[g.device][inst] = planes;
        }
#if !K1_ENH && !K1_WIN && !K1_CAMP // (a batch with enhancement or windows takes the k_binary shape whatever the plan says)
        // whole batches with contiguous rows, when the caller asks for it (RMCV_OPT_PIXEL_SHAPE; a pipeline does for its calm batches):
        // the wave-specialised kernel, ONE 1024-thread workgroup per CU -- 8 loader wavefronts with 2 items (8 loads) in flight each, 8 storers
        constexpr int WS_NL = 8, WS_NS = 8, WS_RING = 2, WS_AUX = 2 /* nt */;
        const size_t planes_ws = ((size_t)2 * (SR + 4) + SR) * g.ww * sizeof(uint64_t);
        if (plan.pixel_ws && linear && !all_pass && taper_head == 0 && planes_ws <= 60 * 1024) {
            K1Args ka;
            ka.frames = frames; ka.frame_pitch = g.frame_pitch; ka.stride = g.stride; ka.n_frames = nf; ka.w = g.w; ka.h = g.h; ka.ww = g.ww;
            ka.lb = lb; ka.morph = morph; ka.binary = binary; ka.bits = bits; ka.prow = g.prow; ka.plane_pitch = g.plane_pitch;
            ka.strips = strips; ka.n_blocks = n_blocks; ka.rowmask = rowmask; ka.strip_ctr = b.strip_ctr;
            ka.imgmask = b.imgmask + (int64_t)f0 * g.h; ka.delta = img_mode == IMAGE_DELTA;
            int grid_ws = ((g.n_cu > 0 ? g.n_cu : 256) + 7) & ~7;
            if (grid_ws > ((n_blocks + 7) & ~7)) grid_ws = (n_blocks + 7) & ~7;
            g_ws_launches.fetch_add(1, std::memory_order_relaxed);
            if (ka.delta && binary) g_image_delta_launches.fetch_add(1, std::memory_order_relaxed);
            // (issue priority 3 for loaders and storers, the sparse kernel's own: in-process A/B against 0 / (2,1) / (3,0) / (1,1):
            // 0.991 / 1.008 / 1.017 / 1.006 of the step; again with the delta stores of the image, against (2,2) / (1,1) / (0,0): 0.988 /
            // 0.997 / 0.999 with the pairs disagreeing in sign -- profiles/image_delta_schedule_ab.txt)
            // (in the pipeline, in-process A/B against this shape: ring of 3 items 1.005, of 4 1.005; 12 loaders + 4 storers 1.087, 10 + 4
            // 1.017, 8 + 4 1.024; loads without the nt hint 1.062)
            const hipError_t e = launch(k_binary_ws<CA, CB, WS_NL, WS_NS, WS_RING, WS_AUX, 3, 3>, dim3(grid_ws), dim3((WS_NL + WS_NS) * 64), planes_ws, s, ka);
            if (e != hipSuccess) return e;
            continue;
        }
        all_ws = false;
#endif
#define RMCV_K1_LAUNCH(F)                                                                                                             \
    launch(K1_INST(F), dim3(grid), dim3(256), planes, s, frames, g.frame_pitch, g.stride, nf, g.w, g.h, g.ww, lb, all_pass, \
           morph, binary, bits, g.prow, g.plane_pitch, strips, n_blocks, rowmask, b.strip_ctr, taper_head, taper_tail,               \
           g.pixel_halo_nt K1_EXTRA)
#if K1_WIN
        const hipError_t e = mode == 1 ? RMCV_K1_LAUNCH(1) : RMCV_K1_LAUNCH(0);
#else
        const hipError_t e = mode == 2 ? RMCV_K1_LAUNCH(2) : mode == 1 ? RMCV_K1_LAUNCH(1) : RMCV_K1_LAUNCH(0);
#endif
#undef RMCV_K1_LAUNCH
        if (e != hipSuccess) return e;
    }
#if !K1_ENH && !K1_WIN && !K1_CAMP
    if (img) *img = image_step(img_before, {all_ws ? IMAGE_KERNEL_WS : IMAGE_KERNEL_OTHER, image, g.w, g.h, g.ww, g.n_frames}, true).next;
#endif
    return hipSuccess;
}
#undef K1_INST
