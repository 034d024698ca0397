// k_binary_launch.inc -- the launcher of the kernel k_binary_kernel.inc has just defined.  Loader form, chunks of frames below 4 GiB, the
// persistent grid, the taper and whether a chunk is k_binary_ws come from pixel_plan.h (pixel_shape, pixel_chunk); what is left here needs
// HIP: the chunks' pointers, function attributes, counters, the launches.  The includer defines K1_LAUNCH_T and K1_EXTRA (trailing kernel
// arguments); with K1_ENH 0 it has also included k_binary_ws.inc and defined g_ws_launches.  K1_WIN (k_binary_win.hip): window rows are not
// contiguous -- never the linear loader, never k_binary_ws; FAST 2 is not even instantiated.
// img (nullable; the K1_ENH 0, K1_WIN 0 build alone reads it): what the context knows about its byte image (image_plan.h).  It decides how
// k_binary_ws stores the image and is rewritten once every chunk has been enqueued -- or left UNKNOWN by an error.
// plane (nullable, beside img): the frames whose bit plane and row masks are in step with the image (image_plan.h: plane_step), kept the same way.
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
                                  hipStream_t s, ImageState* img = nullptr, int* plane = nullptr)
{
    // everything about the launches but the HIP calls: pixel_plan.h
    constexpr PixelVariant variant = K1_CAMP ? (K1_WIN ? PIXEL_CAMP_WIN : PIXEL_CAMP) : K1_WIN ? PIXEL_WIN : K1_ENH ? PIXEL_ENH : PIXEL_BGR;
    const PixelShape ps = pixel_shape(pixel_batch(g, b, variant, lower_bound, plan));
    const int strips = ps.strips, lb = ps.lb, all_pass = ps.all_pass, mode = ps.mode;
    const size_t planes = ps.planes;
#if !K1_ENH && !K1_WIN && !K1_CAMP
    // the chunks of a batch share one state: the mode from what held before the batch, the next state from what all of them ran as
    const ImageState img_before = img ? *img : IMAGE_STATE_UNKNOWN;
    const ImageLaunch img_launch = {IMAGE_KERNEL_WS, image, g.w, g.h, g.ww, g.n_frames};
    const ImageMode img_mode = image_step(img_before, img_launch, true).mode;
    const int plane_before = plane ? *plane : 0;
    const bool plane_delta = plane_step(plane_before, img_mode, img_launch, true).delta;
    bool all_ws = true;
    if (img) *img = image_step(img_before, img_launch, false).next; // (until every chunk is enqueued: what an error return leaves behind)
    if (plane) *plane = plane_step(plane_before, img_mode, img_launch, false).next;
#endif
    for (int f0 = 0; f0 < g.n_frames; f0 += ps.chunk) {
        const int nf = std::min(ps.chunk, g.n_frames - f0);
        const PixelChunk pc = pixel_chunk(ps, nf);
        const int n_blocks = pc.n_blocks, grid = pc.grid, taper_head = pc.taper_head, taper_tail = pc.taper_tail;
        const uint8_t* frames = b.frames + (int64_t)f0 * g.frame_pitch;
        uint8_t* binary = image ? b.binary + (int64_t)f0 * g.w * g.h : nullptr;
        uint64_t* bits = b.bits + (int64_t)f0 * g.plane_pitch;
        uint32_t* rowmask = b.rowmask + (int64_t)f0 * g.h;
        // beyond 64 KiB of dynamic LDS (frames wider than ~6700 pixels) the kernel has to be told; per device and instantiation
        static size_t lds_set[MAX_DEVICES][3] = {};
        if (planes > 60 * 1024 && planes > lds_set[g.device][mode]) {
#if K1_WIN
            const void* fn = mode == 1 ? reinterpret_cast<const void*>(K1_INST(1)) : reinterpret_cast<const void*>(K1_INST(0));
#else
            const void* fn = mode == 2 ? reinterpret_cast<const void*>(K1_INST(2)) : mode == 1 ? reinterpret_cast<const void*>(K1_INST(1)) : reinterpret_cast<const void*>(K1_INST(0));
#endif
            const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes);
            if (ea != hipSuccess) return ea;
            lds_set[g.device][mode] = planes;
        }
#if !K1_ENH && !K1_WIN && !K1_CAMP // (every other variant takes the k_binary shape whatever the plan says: PixelChunk::ws is never set for them)
        // the wave-specialised kernel: 8 loader wavefronts with 2 items (8 loads) in flight each, 8 storers
        constexpr int WS_NL = 8, WS_NS = 8, WS_RING = 2, WS_AUX = 2 /* nt */;
        if (pc.ws) {
            K1Args ka;
            ka.frames = frames; ka.frame_pitch = g.frame_pitch; ka.stride = g.stride; ka.n_frames = nf; ka.w = g.w; ka.h = g.h; ka.ww = g.ww;
            ka.lb = lb; ka.morph = morph; ka.binary = binary; ka.bits = bits; ka.prow = g.prow; ka.plane_pitch = g.plane_pitch;
            ka.strips = strips; ka.n_blocks = n_blocks; ka.rowmask = rowmask; ka.strip_ctr = b.strip_ctr;
            ka.imgmask = b.imgmask + (int64_t)f0 * g.h; ka.delta = img_mode == IMAGE_DELTA;
            ka.plane_delta = plane_delta;
            g_ws_launches.fetch_add(1, std::memory_order_relaxed);
            if (ka.delta && binary) g_image_delta_launches.fetch_add(1, std::memory_order_relaxed);
            if (ka.delta && binary && plane_delta) g_plane_delta_launches.fetch_add(1, std::memory_order_relaxed);
            // (issue priority 3 for loaders and storers, the sparse kernel's own: in-process A/B against 0 / (2,1) / (3,0) / (1,1):
            // 0.991 / 1.008 / 1.017 / 1.006 of the step; again with the delta stores of the image, against (2,2) / (1,1) / (0,0): 0.988 /
            // 0.997 / 0.999 with the pairs disagreeing in sign -- profiles/image_delta_schedule_ab.txt)
            // (in the pipeline, in-process A/B against this shape: ring of 3 items 1.005, of 4 1.005; 12 loaders + 4 storers 1.087, 10 + 4
            // 1.017, 8 + 4 1.024; loads without the nt hint 1.062)
            const hipError_t e = launch(k_binary_ws<CA, CB, WS_NL, WS_NS, WS_RING, WS_AUX, 3, 3>, dim3(pc.grid_ws), dim3((WS_NL + WS_NS) * 64), ps.planes_ws, s, ka);
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
    const ImageLaunch img_ran = {all_ws ? IMAGE_KERNEL_WS : IMAGE_KERNEL_OTHER, image, g.w, g.h, g.ww, g.n_frames};
    if (img) *img = image_step(img_before, img_ran, true).next;
    if (plane) *plane = plane_step(plane_before, img_mode, img_ran, true).next;
#endif
    return hipSuccess;
}
#undef K1_INST
