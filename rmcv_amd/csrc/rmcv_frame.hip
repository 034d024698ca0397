// rmcv_frame.hip -- the per-frame drop-in chain of include/rmcv_abi.h: rmcv_extract_color -> rmcv_filter_lightblobs ->
// rmcv_filter_armours, the loop an unchanged executable/main.cpp:172-176 runs on every camera frame, with its staging, its upload and
// export paths and the stage-wise rmcv_fit_ellipse.  Its state is rmcv_ctx::chain (rmcv_ctx.h), its host-side rules frame_plan.h.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rmcv_ctx.h"

using namespace rmcv;

hipError_t FrameChain::init()
{
    hipError_t e = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, 0);
    if (e != hipSuccess) return e;
    if (getenv("RMCV_IMAGE_EXPORT")) image_export = atoi(getenv("RMCV_IMAGE_EXPORT")); // (the options' defaults for hosts that cannot call them: tools/frame_chain.c)
    if (getenv("RMCV_FRAME_UPLOAD")) frame_upload = atoi(getenv("RMCV_FRAME_UPLOAD"));
    return e;
}

void FrameChain::release()
{
    if (side) hipStreamDestroy(side);
    if (ev_fork) hipEventDestroy(ev_fork);
    for (auto& r : registered) hipHostUnregister(const_cast<void*>(r.p));
    if (h_image) hipHostFree(h_image);
    if (h_iflags) hipHostFree(h_iflags);
    for (void* h : {(void*)h_frame, (void*)h_hdr, (void*)h_pts, (void*)h_offs, (void*)h_blobs, (void*)h_blob_src, (void*)h_neg, (void*)h_armours})
        if (h) hipHostFree(h);
}

void rmcv::resident_none(rmcv_ctx* c)
{
    c->chain.res_nc = c->chain.res_nb = -1;
    c->chain.ahead_lb = c->chain.ahead_ar = false;
}

// pinned host staging + the device header word of the per-frame path (lazy: batch users never pay for it)
static int ensure_staging(rmcv_ctx* c)
{
    FrameChain& ch = c->chain;
    if (ch.h_hdr) return RMCV_OK;
    const Limits& L = c->lim;
    hipError_t e = hipHostMalloc((void**)&ch.h_hdr, 16 * sizeof(int32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_pts, (size_t)L.max_points * sizeof(rmcv_point), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_offs, (size_t)(L.max_contours + 1) * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_blobs, (size_t)L.max_blobs * sizeof(rmcv_lightblob), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_blob_src, (size_t)L.max_blobs * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_neg, (size_t)L.max_contours * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ch.h_armours, (size_t)L.max_armours * sizeof(rmcv_armour), hipHostMallocDefault);
    if (e == hipSuccess) e = dalloc(c, &ch.d_hdr, 16);
    if (e != hipSuccess) return fail(c, RMCV_ERR_NOMEM, "pinned staging", e);
    memset(ch.h_hdr, 0, 16 * sizeof(int32_t));
    if (hipHostGetDevicePointer((void**)&ch.hd_hdr, ch.h_hdr, 0) != hipSuccess || hipHostGetDevicePointer((void**)&ch.hd_pts, ch.h_pts, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&ch.hd_offs, ch.h_offs, 0) != hipSuccess || hipHostGetDevicePointer((void**)&ch.hd_blobs, ch.h_blobs, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&ch.hd_blob_src, ch.h_blob_src, 0) != hipSuccess || hipHostGetDevicePointer((void**)&ch.hd_neg, ch.h_neg, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&ch.hd_armours, ch.h_armours, 0) != hipSuccess) {
        (void)hipGetLastError();
        ch.hd_hdr = nullptr; // k_export is not used
    }
    return RMCV_OK;
}

namespace rmcv {
// The byte image of one frame on its way to the caller (rmcv_extract_color's `binary_out`) WITHOUT the HIP runtime's pageable copy
// (RMCV_OPT_IMAGE_EXPORT = 1; round 5).  hipMemcpyAsync to pageable memory does its work INSIDE the call: 35 us when all is well,
// 160-280 us in some processes (bench.py's C-host child, every time; a process started right behind the GPU test suite, once: the
// per-frame chain then takes 0.28-0.40 ms instead of 0.18 -- VERDICT r4 weak #4; not reproduced by an idle process with three
// full-size pipelines beside the chain, by 12 hardware queues, or by how the caller's buffer is backed: tools/chain_ab.sh,
// chain_beside.sh, chain_queues.sh).  This path has no runtime-internal wait: a kernel on the side stream copies the image into pinned host
// memory chunk by chunk and raises a flag word per chunk (system-scope release behind the chunk's stores); the host polls the flags
// in memory -- no HIP call -- and copies each chunk into the caller's buffer while the next ones cross PCIe.  Measured: 0.190 ms per
// chain alone (the runtime's copy: 0.186), 0.19-0.20 where the runtime's copy reads 0.28-0.40.
// All IMG_GROUPS workgroups work on chunk 0 first, then on chunk 1, ...: the chunks reach the host ONE AFTER THE OTHER (the CPU copies
// chunk g into the caller's buffer while chunk g + 1 crosses PCIe), not all at the end.  A workgroup that has stored its slice of a
// chunk (system-scope fence behind the stores) counts itself in; the last one raises the chunk's flag in host memory.
__global__ __launch_bounds__(256) void k_image_export(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long bytes,
                                                      uint32_t* __restrict__ flags, uint32_t seq, uint32_t* __restrict__ arrived, int n_chunks)
{
    const int wg = blockIdx.x, tid = threadIdx.x;
    const long long per = image_chunk_bytes(bytes, n_chunks);
    for (int g = 0; g < n_chunks; g++) {
        const ImageChunk ck = image_chunk_at(bytes, per, g); // (frame_plan.h: the host takes the same chunks, image_chunk)
        const long long lo = ck.lo, hi = ck.hi;
        const long long hv = lo + ((hi - lo) & ~15ll);
        for (long long o = lo + ((long long)wg * 256 + tid) * 16; o < hv; o += (long long)gridDim.x * 256 * 16)
            *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(src + o);
        if (wg == 0 && hv + tid < hi) dst[hv + tid] = src[hv + tid]; // (the image's last bytes: fewer than 16)
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            const uint32_t before = __hip_atomic_fetch_add(&arrived[g], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (before == gridDim.x - 1) {
                __hip_atomic_store(&arrived[g], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (for the next frame: launches of one context are ordered)
                __hip_atomic_store(&flags[g], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}
} // namespace rmcv

extern "C" {

int rmcv_ctx_frame_timing(const rmcv_ctx* c, double* us, int cap)
{
    if (!c || !us || cap < 7) return RMCV_ERR_BAD_ARG;
    const FrameChain& ch = c->chain;
    for (int i = 0; i < 7; i++) us[i] = ch.marks[i + 1] - ch.marks[i];
    if (cap >= 9) { us[7] = ch.upload_now; us[8] = ch.image_now; }
    return RMCV_OK;
}

int rmcv_ctx_forget_frame_buffer(rmcv_ctx* c, const void* frame)
{ // RMCV_OPT_FRAME_UPLOAD = 2 keys its pinnings by address: a buffer must be forgotten before it is freed (see the header)
    if (!c) return RMCV_ERR_BAD_ARG;
    FrameChain& ch = c->chain;
    hipSetDevice(c->device);
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    for (size_t i = 0; i < ch.registered.size();) {
        if (!frame || ch.registered[i].p == frame) {
            hipHostUnregister(const_cast<void*>(ch.registered[i].p));
            ch.registered.erase(ch.registered.begin() + i);
        } else i++;
    }
    return RMCV_OK;
}

/* ---------------- single-frame, host-buffer entry points ----------------
 * The chain an unchanged executable/main.cpp:172-176 runs on every camera frame.  Each call is ONE stream sequence with ONE
 * synchronisation: upload (pinned staging) -> kernels -> a header word + fixed windows of the results copied back
 * speculatively (a frame has ~1000 contour points, ~10 blobs, ~3 armours; what does not fit a window is fetched by a second
 * copy).  Results stay on the device: when the next call is handed exactly the bytes the previous one returned, it runs on the
 * resident buffers instead of uploading them again. */

// the windows of this context's results (frame_plan.h)
static FrameWindows result_windows(const rmcv_ctx* c) { return frame_windows(c->lim.max_contours, c->lim.max_points, c->lim.max_blobs, c->lim.max_armours); }
// rmcv_default_params with the chain's parameter sets written over them
static rmcv_params chain_run_params(const LbParams* lb, const ArParams* ar)
{
    rmcv_params p;
    rmcv_default_params(&p);
    chain_params(&p, lb, ar);
    return p;
}

// bring one frame (BGR, or a mosaic: rowb = 3 w or w bytes per row) into own_frames (frame slot 0) on the context's stream;
// RMCV_OPT_FRAME_UPLOAD selects how
static int upload_one(rmcv_ctx* c, const uint8_t* bgr, int rowb, int h, int stride, int dstride)
{
    FrameChain& ch = c->chain;
    const size_t dpitch = (size_t)dstride * h;
    hipStream_t s = c->stream;
    const int mode = copy_path(COPY_UPLOAD, ch.frame_upload, ch.copy_up);
    ch.upload_now = mode;
    if (mode == 2) { // pin the caller's buffer once (camera SDKs hand out a small ring of frame buffers) and DMA from it
        const size_t span = (size_t)stride * (h - 1) + (size_t)rowb;
        bool known = false;
        for (auto& r : ch.registered) known |= (r.p == bgr && r.bytes >= span);
        if (!known) {
            if (ch.registered.size() >= 16) { // a ring larger than this is not a ring: forget the oldest
                hipHostUnregister(const_cast<void*>(ch.registered.front().p));
                ch.registered.erase(ch.registered.begin());
            }
            if (hipHostRegister(const_cast<uint8_t*>(bgr), span, hipHostRegisterDefault) == hipSuccess) {
                ch.registered.push_back({bgr, span});
                known = true;
            } else {
                (void)hipGetLastError(); // e.g. already registered by the application: plain copy below
            }
        }
        HIPCHK(c, hipMemcpy2DAsync(c->own_frames, dstride, bgr, stride, (size_t)rowb, h, hipMemcpyHostToDevice, s), "H2D frame");
        return RMCV_OK;
    }
    if (mode == 0) { // the runtime's own pageable path
        HIPCHK(c, hipMemcpy2DAsync(c->own_frames, dstride, bgr, stride, (size_t)rowb, h, hipMemcpyHostToDevice, s), "H2D frame");
        return RMCV_OK;
    }
    if (dpitch > ch.h_frame_bytes) {
        if (ch.h_frame) hipHostFree(ch.h_frame);
        ch.h_frame = nullptr;
        ch.h_frame_bytes = 0;
        size_t cap = (size_t)((3 * c->lim.max_width + 15) & ~15) * c->lim.max_height;
        if (cap < dpitch) cap = dpitch;
        HIPCHK(c, hipHostMalloc((void**)&ch.h_frame, cap, hipHostMallocDefault), "pinned frame staging");
        ch.h_frame_bytes = cap;
    }
    // two halves: the DMA of the first runs while the CPU copies the second (eight pieces, measured in round 5: 0.254-0.281 ms per chain
    // against 0.223 -- every further hipMemcpyAsync costs the host 4-5 us, more than the earlier start of the DMA buys)
    const int parts = 2;
    for (int part = 0; part < parts; part++) {
        const int y0 = (int)((long long)h * part / parts), y1 = (int)((long long)h * (part + 1) / parts);
        if (y1 <= y0) continue;
        if (stride == dstride) memcpy(ch.h_frame + (size_t)y0 * dstride, bgr + (size_t)y0 * stride, (size_t)(y1 - y0) * dstride);
        else
            for (int y = y0; y < y1; y++) memcpy(ch.h_frame + (size_t)y * dstride, bgr + (size_t)y * stride, (size_t)rowb);
        HIPCHK(c, hipMemcpyAsync(c->own_frames + (size_t)y0 * dstride, ch.h_frame + (size_t)y0 * dstride, (size_t)(y1 - y0) * dstride,
                                 hipMemcpyHostToDevice, s), "H2D frame");
    }
    return RMCV_OK;
}

// the blob stage on frame slot 0 + its results on their way to pinned memory (header at h_hdr[4..6]); no synchronisation
static int enqueue_blobs(rmcv_ctx* c, const LbParams& q, bool compute = true, bool download = true)
{
    FrameChain& ch = c->chain;
    const rmcv_params p = chain_run_params(&q, nullptr);
    const Geom g1 = one_frame_geom(c);
    const Bufs& b = c->bufs;
    hipStream_t s = c->stream;
    if (compute) {
        HIPCHK(c, launch_status_clear(g1, b, RMCV_FRAME_OVF_BLOBS | RMCV_FRAME_OVF_ARMOURS | RMCV_FRAME_HULL, s), "k_status_clear");
        HIPCHK(c, launch_blobs(g1, b, c->lim, p, s), "k_blobs");
    }
    if (!download) return RMCV_OK; // (the caller sends everything home with one k_export)
    HIPCHK(c, launch_gather3(b.n_blobs, b.n_neg, b.status, ch.d_hdr + 4, s), "k_gather3");
    HIPCHK(c, hipMemcpyAsync(ch.h_hdr + 4, ch.d_hdr + 4, 3 * 4, hipMemcpyDeviceToHost, s), "D2H");
    const FrameWindows W = result_windows(c);
    const int bw = W.blobs, nw = W.neg;
    HIPCHK(c, hipMemcpyAsync(ch.h_blobs, b.blobs, (size_t)bw * sizeof(rmcv_lightblob), hipMemcpyDeviceToHost, s), "D2H blobs");
    HIPCHK(c, hipMemcpyAsync(ch.h_blob_src, b.blob_src, (size_t)bw * 4, hipMemcpyDeviceToHost, s), "D2H blob_src");
    HIPCHK(c, hipMemcpyAsync(ch.h_neg, b.neg_idx, (size_t)nw * 4, hipMemcpyDeviceToHost, s), "D2H neg");
    return RMCV_OK;
}

// after the stream has been synchronised: what did not fit the windows, then the hand-over to the caller
static int finish_blobs(rmcv_ctx* c, rmcv_lightblob* blobs_out, int blobs_cap, int32_t* n_blobs, int32_t* blob_src, int32_t* neg_idx_out,
                        int32_t* n_neg)
{
    FrameChain& ch = c->chain;
    const Bufs& b = c->bufs;
    const FrameWindows W = result_windows(c);
    const int bw = W.blobs, nw = W.neg;
    const int32_t nb = ch.h_hdr[4], nn = ch.h_hdr[5], st = ch.h_hdr[6];
    if (n_blobs) *n_blobs = nb;
    if (n_neg) *n_neg = nn;
    if (st & RMCV_FRAME_OVF_BLOBS) return fail(c, RMCV_ERR_CAPACITY, "context limit exceeded (max_blobs)");
    if (nb > bw) {
        HIPCHK(c, hipMemcpy(ch.h_blobs + bw, b.blobs + bw, (size_t)(nb - bw) * sizeof(rmcv_lightblob), hipMemcpyDeviceToHost), "D2H blobs");
        HIPCHK(c, hipMemcpy(ch.h_blob_src + bw, b.blob_src + bw, (size_t)(nb - bw) * 4, hipMemcpyDeviceToHost), "D2H blob_src");
    }
    if (nn > nw) HIPCHK(c, hipMemcpy(ch.h_neg + nw, b.neg_idx + nw, (size_t)(nn - nw) * 4, hipMemcpyDeviceToHost), "D2H neg");
    ch.res_nb = nb; // the device holds this positive list, h_blobs its bytes
    if (nb > blobs_cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (blobs_out && nb) memcpy(blobs_out, ch.h_blobs, (size_t)nb * sizeof(rmcv_lightblob));
    if (blob_src && nb) memcpy(blob_src, ch.h_blob_src, (size_t)nb * 4);
    if (neg_idx_out && nn) memcpy(neg_idx_out, ch.h_neg, (size_t)nn * 4);
    return RMCV_OK;
}

static int enqueue_armours(rmcv_ctx* c, const ArParams& q, bool compute = true, bool download = true)
{
    FrameChain& ch = c->chain;
    const rmcv_params p = chain_run_params(nullptr, &q);
    const Geom g1 = one_frame_geom(c);
    const Bufs& b = c->bufs;
    hipStream_t s = c->stream;
    if (compute) {
        HIPCHK(c, launch_status_clear(g1, b, RMCV_FRAME_OVF_ARMOURS, s), "k_status_clear");
        HIPCHK(c, launch_armours(g1, b, c->lim, p, s), "k_armours");
    }
    if (!download) return RMCV_OK;
    HIPCHK(c, launch_gather3(b.n_armours, b.status, b.status, ch.d_hdr + 8, s), "k_gather3");
    HIPCHK(c, hipMemcpyAsync(ch.h_hdr + 8, ch.d_hdr + 8, 3 * 4, hipMemcpyDeviceToHost, s), "D2H");
    const int aw = result_windows(c).armours;
    HIPCHK(c, hipMemcpyAsync(ch.h_armours, b.armours, (size_t)aw * sizeof(rmcv_armour), hipMemcpyDeviceToHost, s), "D2H armours");
    return RMCV_OK;
}

static int finish_armours(rmcv_ctx* c, rmcv_armour* armours_out, int armours_cap, int32_t* n_armours)
{
    FrameChain& ch = c->chain;
    const Bufs& b = c->bufs;
    const int aw = result_windows(c).armours;
    const int32_t na = ch.h_hdr[8], st = ch.h_hdr[9];
    if (n_armours) *n_armours = na;
    if (st & RMCV_FRAME_OVF_ARMOURS) return fail(c, RMCV_ERR_CAPACITY, "context limit exceeded (max_armours)");
    if (na > aw) HIPCHK(c, hipMemcpy(ch.h_armours + aw, b.armours + aw, (size_t)(na - aw) * sizeof(rmcv_armour), hipMemcpyDeviceToHost), "D2H armours");
    if (na > armours_cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (armours_out && na) memcpy(armours_out, ch.h_armours, (size_t)na * sizeof(rmcv_armour));
    return RMCV_OK;
}

// the pinned, device-mapped landing buffer of the byte image + its chunk flags (lazy; false: not to be had -> the runtime's copy)
static bool image_ready(rmcv_ctx* c, size_t bytes)
{
    FrameChain& ch = c->chain;
    if (copy_path(COPY_IMAGE, ch.image_export, ch.copy_img) != 1) return false; // RMCV_OPT_IMAGE_EXPORT
    if (!ch.h_iflags) {
        if (hipHostMalloc((void**)&ch.h_iflags, IMG_CHUNKS * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&ch.hd_iflags, ch.h_iflags, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (ch.h_iflags) hipHostFree(ch.h_iflags);
            ch.h_iflags = ch.hd_iflags = nullptr;
            return false;
        }
        memset(ch.h_iflags, 0, IMG_CHUNKS * sizeof(uint32_t));
        if (dalloc(c, &ch.d_iarrived, IMG_CHUNKS) != hipSuccess || hipMemset(ch.d_iarrived, 0, IMG_CHUNKS * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            hipHostFree(ch.h_iflags);
            ch.h_iflags = ch.hd_iflags = nullptr;
            return false;
        }
    }
    if (bytes > ch.h_image_bytes) {
        if (ch.h_image) hipHostFree(ch.h_image);
        ch.h_image = ch.hd_image = nullptr;
        ch.h_image_bytes = 0;
        size_t cap = (size_t)c->lim.max_width * c->lim.max_height;
        if (cap < bytes) cap = bytes;
        if (hipHostMalloc((void**)&ch.h_image, cap, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void**)&ch.hd_image, ch.h_image, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (ch.h_image) hipHostFree(ch.h_image);
            ch.h_image = ch.hd_image = nullptr;
            return false;
        }
        ch.h_image_bytes = cap;
    }
    return true;
}

static int extract_color_body(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, int camp, int lower_bound, int morph,
                              uint8_t* binary_out, rmcv_point* pts_out, int pts_cap, int32_t* offs_out, int contours_cap,
                              int32_t* n_contours, int32_t* n_points);

int rmcv_extract_color(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, int camp, int lower_bound, int morph,
                       uint8_t* binary_out, rmcv_point* pts_out, int pts_cap, int32_t* offs_out, int contours_cap,
                       int32_t* n_contours, int32_t* n_points)
{
    const int rc = extract_color_body(c, bgr, w, h, stride, camp, lower_bound, morph, binary_out, pts_out, pts_cap, offs_out,
                                      contours_cap, n_contours, n_points);
    // The body enqueues an upload FROM the caller's frame and a download INTO the caller's `binary_out`.  An error return after
    // the first of them must not leave either in flight: the caller owns those buffers again the moment this function returns.
    // (RMCV_ERR_TIMEOUT is the exception: the wait has just run out -- see the header.)
    if (rc != RMCV_OK && rc != RMCV_ERR_TIMEOUT && c) {
        hipError_t e = hipSuccess;
        (void)wait_stream_deadline(c->stream, c->wait_timeout_ms, &e);
        if (c->chain.side) (void)wait_stream_deadline(c->chain.side, c->wait_timeout_ms, &e);
    }
    return rc;
}

static int extract_color_body(rmcv_ctx* c, const uint8_t* bgr, int w, int h, int stride, int camp, int lower_bound, int morph,
                              uint8_t* binary_out, rmcv_point* pts_out, int pts_cap, int32_t* offs_out, int contours_cap,
                              int32_t* n_contours, int32_t* n_points)
{
    if (!c || !bgr) return RMCV_ERR_BAD_ARG;
    FrameChain& ch = c->chain;
    if (morph < RMCV_MORPH_NONE || morph > RMCV_MORPH_CLOSE) return fail(c, RMCV_ERR_BAD_ARG, "bad morph");
    hipSetDevice(c->device);
    ch.marks[0] = now_us();
    int rc = rmcv_batch_sync(c);
    if (rc) return rc;
    resident_none(c);
    if ((rc = ensure_staging(c))) return rc;
    if ((rc = check_layout(c)) || (rc = check_sample_ptr(c, bgr))) return rc;
    const int rowb = ctx_pixel_bytes(c) * w; // a mosaic (RMCV_OPT_INPUT_FORMAT): one sample per pixel, 1 or 2 bytes
    const int dstride = (rowb + 15) & ~15;
    if ((rc = set_geom(c, 1, w, h, dstride, (int64_t)dstride * h))) return rc;
    reset_modes(c);
    if (stride < rowb) return fail(c, RMCV_ERR_BAD_ARG, "bad stride");
    if (c->geom.sample_bytes == 2 && (stride & 1)) return fail(c, RMCV_ERR_BAD_ARG, "16-bit samples (RMCV_OPT_INPUT_SAMPLE_BITS): stride is bytes and must be even");
    if ((rc = ensure_own_frames(c, (size_t)dstride * h))) return rc;
    if ((rc = upload_one(c, bgr, rowb, h, stride, dstride))) return rc;
    ch.marks[1] = now_us(); // the upload is enqueued (pageable: the runtime may have copied it by now)
    c->bufs.frames = c->own_frames;
    const Geom& g = c->geom;
    const Bufs& b = c->bufs;
    hipStream_t s = c->stream;
    RunPlan plan = ctx_plan(c);
    plan.sparse_waves = 8; // one frame: the latency setting
    if (c->test_delay_us) { // RMCV_OPT_TEST_DELAY_US: a stand-in for a kernel that does not finish in time (one shot)
        HIPCHK(c, launch_delay((unsigned long long)c->test_delay_us * 1000ull, s), "k_delay (RMCV_OPT_TEST_DELAY_US)");
        c->test_delay_us = 0;
    }
    if (g.enhance) HIPCHK(c, launch_enhance_tables(g, b, lower_bound, s), "k_frame_sums + k_enhance_table"); // RMCV_OPT_ENHANCE: the frame is read through its table
    HIPCHK(c, launch_binary(g, b, camp, lower_bound, morph, binary_out != nullptr, plan, s, &c->image, &c->plane_sync), PIXEL_VARIANTS[geom_variant(g)].kernel);
    if (binary_out) HIPCHK(c, hipEventRecord(ch.ev_fork, s), "image download: mark");
    // running ahead with both parameter sets known: the frame's whole sparse part is ONE kernel (the fused per-frame kernel of
    // the batch path: findContours, fits and pairing back to back), not three
    const bool fused_ahead = ch.run_ahead && ch.last_lb_valid && ch.last_ar_valid && ch.last_lb.enemy == ch.last_ar.enemy;
    if (fused_ahead) {
        const rmcv_params p = chain_run_params(&ch.last_lb, &ch.last_ar);
        HIPCHK(c, launch_sparse(g, b, c->lim, p, true, false, plan, s), "k_contours (fused)");
    } else {
        HIPCHK(c, launch_contours(g, b, c->lim, s), "k_contours");
    }
    // Results go home by kernel stores into the pinned buffers (ExportArgs) instead of a row of small copies -- each of those is a
    // hand-over from the compute queue to the copy engine and back, 5-8 us apiece, nine of them when the chain runs ahead
    // (0.256 -> 0.202 ms per chain, tools/frame_chain.py).  When the frame's whole sparse part has run already (fused_ahead) the
    // kernel that packs the contours does it on its way out; otherwise one k_export behind the last stage.
    static const bool use_export = !(getenv("RMCV_EXPORT") && atoi(getenv("RMCV_EXPORT")) == 0); // dev knob for A/B runs
    const bool exporting = use_export && ch.hd_hdr != nullptr;
    const bool will_lb = ch.last_lb_valid && ch.run_ahead, will_ar = will_lb && ch.last_ar_valid;
    const FrameWindows W = result_windows(c);
    ExportArgs ex;
    memset(&ex, 0, sizeof(ex));
    if (exporting) {
        ex.hdr_dst = ch.hd_hdr;
        ex.hdr_src[0] = ch.d_hdr; ex.hdr_src[1] = ch.d_hdr + 1; ex.hdr_src[2] = ch.d_hdr + 2;
        ex.sec[ex.n_sec++] = {c->pack_offs, ch.hd_offs, ch.d_hdr, 1, 4, W.offs + 1};
        ex.sec[ex.n_sec++] = {c->pack_pts, ch.hd_pts, ch.d_hdr + 1, 0, (int)sizeof(rmcv_point), W.pts};
        if (will_lb) {
            ex.hdr_src[4] = b.n_blobs; ex.hdr_src[5] = b.n_neg; ex.hdr_src[6] = b.status;
            ex.sec[ex.n_sec++] = {b.blobs, ch.hd_blobs, b.n_blobs, 0, (int)sizeof(rmcv_lightblob), W.blobs};
            ex.sec[ex.n_sec++] = {b.blob_src, ch.hd_blob_src, b.n_blobs, 0, 4, W.blobs};
            ex.sec[ex.n_sec++] = {b.neg_idx, ch.hd_neg, b.n_neg, 0, 4, W.neg};
        }
        if (will_ar) {
            ex.hdr_src[8] = b.n_armours; ex.hdr_src[9] = b.status; ex.hdr_src[10] = b.status;
            ex.sec[ex.n_sec++] = {b.armours, ch.hd_armours, b.n_armours, 0, (int)sizeof(rmcv_armour), W.armours};
        }
    }
    const bool export_in_pack = exporting && fused_ahead; // (fused_ahead: the blobs and armours exist before the contours are packed)
    HIPCHK(c, launch_pack_contours(g, b, c->lim, c->pack_pts, c->pack_offs, ch.d_hdr, s, export_in_pack ? &ex : nullptr), "k_pack_contours");
    if (!exporting) {
        HIPCHK(c, hipMemcpyAsync(ch.h_hdr, ch.d_hdr, 3 * 4, hipMemcpyDeviceToHost, s), "D2H");
        HIPCHK(c, hipMemcpyAsync(ch.h_offs, c->pack_offs, (size_t)(W.offs + 1) * 4, hipMemcpyDeviceToHost, s), "D2H offs");
        HIPCHK(c, hipMemcpyAsync(ch.h_pts, c->pack_pts, (size_t)W.pts * sizeof(rmcv_point), hipMemcpyDeviceToHost, s), "D2H pts");
    }
    // the byte image goes straight to the caller's buffer (the runtime's pageable path: 37 us for 1.3 MB); through the pinned
    // staging buffer it cost a 65 us CPU copy on top of the DMA
    bool ahead_lb = false, ahead_ar = false;
    if (will_lb) { // the filters of this frame, with the previous frame's parameters (see FrameChain::last_lb)
        if ((rc = enqueue_blobs(c, ch.last_lb, !fused_ahead, !exporting))) return rc;
        ahead_lb = true;
        if (will_ar) {
            if ((rc = enqueue_armours(c, ch.last_ar, !fused_ahead, !exporting))) return rc;
            ahead_ar = true;
        }
    }
    if (exporting && !export_in_pack) HIPCHK(c, launch_export(ex, s), "k_export");
    // The byte image is complete when k_binary is: its download (1.3 MB, 37 us) runs on the side stream BESIDE the sparse kernels
    // instead of behind them.  Enqueued last: the runtime's pageable copy may keep this thread busy, and by now everything else of
    // the frame is on the GPU's queues.
    ch.marks[2] = now_us(); // every kernel of the frame is enqueued
    if (binary_out && image_ready(c, (size_t)w * h)) {
        // k_image_export on the side stream, behind the pixel kernel and beside the sparse kernels; the host takes the chunks as their flags come up
        const long long bytes = (long long)w * h;
        if (++ch.img_seq == 0) ch.img_seq = 1;
        HIPCHK(c, hipStreamWaitEvent(ch.side, ch.ev_fork, 0), "image download: fork");
        const int n_chunks = IMG_CHUNKS_DEFAULT;
        HIPCHK(c, launch(k_image_export, dim3(IMG_GROUPS), dim3(256), 0, ch.side, b.binary, ch.hd_image, bytes, ch.hd_iflags, ch.img_seq, ch.d_iarrived, n_chunks), "k_image_export");
        c->last_what = "k_binary, k_image_export";
        const volatile uint32_t* fl = ch.h_iflags;
        const double t0w = now_us();
        for (int gch = 0; gch < n_chunks; gch++) {
            for (unsigned spins = 0; fl[gch] != ch.img_seq; spins++) {
                __builtin_ia32_pause();
                if ((spins & 1023u) == 1023u) {
                    const double dtw = now_us() - t0w;
                    if (c->wait_timeout_ms > 0 && dtw > c->wait_timeout_ms * 1000.0) return wait_failed(c, 1, "rmcv_extract_color: waiting for the byte image", hipSuccess);
                    if (dtw > 20000.0) { timespec nap = {0, 200000}; nanosleep(&nap, nullptr); } // (20 ms in: something is wrong; stop burning the core)
                }
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if (gch == 0) ch.marks[3] = now_us(); // upload and pixel kernel are through, the first chunk is home
            const ImageChunk ck = image_chunk(bytes, n_chunks, gch);
            if (ck.hi > ck.lo) memcpy(binary_out + ck.lo, ch.h_image + ck.lo, (size_t)(ck.hi - ck.lo));
        }
        ch.marks[4] = now_us(); // the byte image is in the caller's buffer
        ch.image_now = 1;
    } else if (binary_out) {
        ch.image_now = 0; // (no mapped pinned memory to be had: the runtime's pageable copy)
        c->last_what = "k_binary";
        WAITCHK(c, wait_event(c, ch.ev_fork, "rmcv_extract_color: waiting for the pixel kernel"));
        ch.marks[3] = now_us();
        HIPCHK(c, hipMemcpyAsync(binary_out, b.binary, (size_t)w * h, hipMemcpyDeviceToHost, ch.side), "D2H binary");
        ch.marks[4] = now_us();
        WAITCHK(c, wait_stream(c, ch.side, "rmcv_extract_color: waiting for the byte image's download"));
    } else ch.marks[3] = ch.marks[4] = ch.marks[2];
    ch.marks[5] = now_us();
    c->last_what = fused_ahead ? "k_binary, k_contours (fused), k_pack_contours + export" : "k_binary, k_contours, k_pack_contours, k_export";
    WAITCHK(c, wait_stream(c, s, "rmcv_extract_color: waiting for the frame's kernels"));
    ch.marks[6] = now_us();
    const int32_t nc = ch.h_hdr[0], total = ch.h_hdr[1], st = ch.h_hdr[2];
    if (n_contours) *n_contours = nc;
    if (n_points) *n_points = total;
    if (st & (RMCV_FRAME_OVF_CONTOURS | RMCV_FRAME_OVF_POINTS)) return fail(c, RMCV_ERR_CAPACITY, "context limits exceeded (max_contours/max_points)");
    if (nc > W.offs) HIPCHK(c, hipMemcpy(ch.h_offs + W.offs + 1, c->pack_offs + W.offs + 1, (size_t)(nc - W.offs) * 4, hipMemcpyDeviceToHost), "D2H offs");
    if (total > W.pts) HIPCHK(c, hipMemcpy(ch.h_pts + W.pts, c->pack_pts + W.pts, (size_t)(total - W.pts) * sizeof(rmcv_point), hipMemcpyDeviceToHost), "D2H pts");
    ch.res_nc = nc; // the device holds these contours (discovery order + the fit work list) and h_pts / h_offs their CSR
    ch.res_total = total;
    ch.ahead_lb = ahead_lb;
    ch.ahead_ar = ahead_ar;
    if (nc > contours_cap || total > pts_cap) return fail(c, RMCV_ERR_CAPACITY, "output capacity exceeded");
    if (offs_out) memcpy(offs_out, ch.h_offs, (size_t)(nc + 1) * 4);
    if (pts_out && total) memcpy(pts_out, ch.h_pts, (size_t)total * sizeof(rmcv_point));
    ch.marks[7] = now_us();
    if (binary_out) { // what the runtime's copies cost this frame (see frame_plan.h: copy_path_step)
        const double up_us = ch.marks[3] - ch.marks[1] + ch.test_slow_us, img_us = ch.marks[4] - ch.marks[3] + ch.test_slow_us;
        // (the upload moves what the frame holds: 3 B/px of BGR, 1 or 2 B/px of a mosaic -- RMCV_OPT_INPUT_FORMAT, _SAMPLE_BITS)
        const double frame_bytes = (double)geom_pixel_bytes(c->geom) * w * h, image_bytes = (double)w * h;
        ch.copy_up = copy_path_step(COPY_UPLOAD, ch.frame_upload, ch.copy_up, ch.upload_now, up_us, frame_bytes);
        ch.copy_img = copy_path_step(COPY_IMAGE, ch.image_export, ch.copy_img, ch.image_now, img_us, image_bytes);
    }
    return RMCV_OK;
}

} // extern "C"

int rmcv::load_contours(rmcv_ctx* c, const rmcv_point* pts, const int32_t* offs, int n)
{
    int rc = rmcv_batch_sync(c); // frame slot 0 may belong to a batch in flight on a caller stream
    if (rc) return rc;
    resident_none(c);
    if (n < 0 || n > c->lim.max_contours) return fail(c, RMCV_ERR_CAPACITY, "too many contours for this context");
    const int total = n ? offs[n] : 0;
    if (total > c->lim.max_points) return fail(c, RMCV_ERR_CAPACITY, "too many points for this context");
    std::vector<int32_t> cs(n > 0 ? n : 1), cl(n > 0 ? n : 1), el;
    for (int i = 0; i < n; i++) {
        if (offs[i + 1] < offs[i]) return fail(c, RMCV_ERR_BAD_ARG, "offs not monotone");
        cs[n - 1 - i] = offs[i];
        cl[n - 1 - i] = offs[i + 1] - offs[i];
    }
    // cv::findContours never returns a negative coordinate, and the fit's rule "a float sum of coordinates is exact below 2^24"
    // (wave_detect.h: fit_ellipse_wave) holds for non-negative terms only: such a list is refused here, on the host, before anything
    // is copied (rmcv_abi.h: rmcv_fit_ellipse, rmcv_filter_lightblobs, rmcv_match_lightblob)
    for (int i = 0; i < total; i++)
        if (pts[i].x < 0 || pts[i].y < 0) return fail(c, RMCV_ERR_BAD_ARG, "contour point with a negative coordinate");
    for (int k = 0; k < n; k++)
        if (cl[k] >= 6) el.push_back(k); // the fit stage's work list (what k_contours writes in the batch path)
    const int32_t ne = (int32_t)el.size();
    if (c->geom.n_frames < 1) c->geom.n_frames = 1;
    const Bufs& b = c->bufs;
    int32_t z = 0;
    if (total) HIPCHK(c, hipMemcpy(b.points, pts, (size_t)total * sizeof(rmcv_point), hipMemcpyHostToDevice), "H2D points");
    if (n) {
        HIPCHK(c, hipMemcpy(b.cont_start, cs.data(), (size_t)n * 4, hipMemcpyHostToDevice), "H2D");
        HIPCHK(c, hipMemcpy(b.cont_len, cl.data(), (size_t)n * 4, hipMemcpyHostToDevice), "H2D");
    }
    HIPCHK(c, hipMemcpy(b.n_contours, &n, 4, hipMemcpyHostToDevice), "H2D");
    HIPCHK(c, hipMemcpy(b.n_points, &total, 4, hipMemcpyHostToDevice), "H2D");
    if (n) HIPCHK(c, hipMemset(b.slot_kind, 0, (size_t)n * 4), "memset slot_kind");
    if (ne) HIPCHK(c, hipMemcpy(b.elig, el.data(), (size_t)ne * 4, hipMemcpyHostToDevice), "H2D elig");
    HIPCHK(c, hipMemcpy(b.n_elig, &ne, 4, hipMemcpyHostToDevice), "H2D");
    HIPCHK(c, hipMemcpy(b.status, &z, 4, hipMemcpyHostToDevice), "H2D");
    return RMCV_OK;
}

extern "C" {

int rmcv_filter_lightblobs(rmcv_ctx* c, const rmcv_point* pts, const int32_t* offs, int n_contours, float tilt_max,
                           float ratio_lo, float ratio_hi, double area_lo, double area_hi, int enemy,
                           rmcv_lightblob* blobs_out, int blobs_cap, int32_t* n_blobs, int32_t* blob_src,
                           int32_t* neg_idx_out, int32_t* n_neg)
{
    if (!c || n_contours < 0 || (n_contours > 0 && (!pts || !offs))) return RMCV_ERR_BAD_ARG;
    FrameChain& ch = c->chain;
    hipSetDevice(c->device);
    int rc = ensure_staging(c);
    if (rc) return rc;
    // handed exactly what rmcv_extract_color returned last?  then the contours (and the fit work list) are already on the device
    const bool resident = ch.res_nc >= 0 && n_contours == ch.res_nc &&
                          (n_contours == 0 || (offs[n_contours] == ch.res_total && memcmp(offs, ch.h_offs, (size_t)(n_contours + 1) * 4) == 0 &&
                                               memcmp(pts, ch.h_pts, (size_t)ch.res_total * sizeof(rmcv_point)) == 0));
    if (!resident) {
        rc = load_contours(c, pts, offs, n_contours);
        if (rc) return rc;
    }
    ch.res_nb = -1;
    const LbParams q = {tilt_max, ratio_lo, ratio_hi, area_lo, area_hi, enemy};
    const bool ran_ahead = resident && ch.ahead_lb && memcmp(&q, &ch.last_lb, sizeof(q)) == 0; // extract_color did it already
    ch.last_lb = q;
    ch.last_lb_valid = true;
    if (!ran_ahead) {
        ch.ahead_ar = false; // the armours run ahead (if any) belong to other blobs
        if (c->geom.n_frames < 1) c->geom.n_frames = 1;
        if ((rc = enqueue_blobs(c, q))) return rc;
        WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    }
    ch.ahead_lb = false;
    return finish_blobs(c, blobs_out, blobs_cap, n_blobs, blob_src, neg_idx_out, n_neg);
}

int rmcv_filter_armours(rmcv_ctx* c, const rmcv_lightblob* blobs, int n_blobs, float angle_diff_max, float shear_max,
                        float length_ratio_max, int enemy, rmcv_armour* armours_out, int armours_cap, int32_t* n_armours)
{
    if (!c || (n_blobs > 0 && !blobs) || n_blobs < 0) return RMCV_ERR_BAD_ARG;
    FrameChain& ch = c->chain;
    if (n_blobs > c->lim.max_blobs) return fail(c, RMCV_ERR_CAPACITY, "too many blobs for this context");
    hipSetDevice(c->device);
    int rc = ensure_staging(c);
    if (rc) return rc;
    const Bufs& b = c->bufs;
    hipStream_t s = c->stream;
    // handed exactly the positive list rmcv_filter_lightblobs returned last?  then it is already on the device
    const bool resident = ch.res_nb >= 0 && n_blobs == ch.res_nb &&
                          (n_blobs == 0 || memcmp(blobs, ch.h_blobs, (size_t)n_blobs * sizeof(rmcv_lightblob)) == 0);
    if (!resident) {
        rc = rmcv_batch_sync(c);
        if (rc) return rc;
        resident_none(c);
        int32_t z = 0;
        if (n_blobs) HIPCHK(c, hipMemcpy(b.blobs, blobs, (size_t)n_blobs * sizeof(rmcv_lightblob), hipMemcpyHostToDevice), "H2D blobs");
        HIPCHK(c, hipMemcpy(b.n_blobs, &n_blobs, 4, hipMemcpyHostToDevice), "H2D");
        HIPCHK(c, hipMemcpy(b.status, &z, 4, hipMemcpyHostToDevice), "H2D");
    }
    const ArParams q = {angle_diff_max, shear_max, length_ratio_max, enemy};
    const bool ran_ahead = resident && ch.ahead_ar && memcmp(&q, &ch.last_ar, sizeof(q)) == 0;
    ch.last_ar = q;
    ch.last_ar_valid = true;
    ch.ahead_ar = false;
    if (!ran_ahead) {
        if ((rc = enqueue_armours(c, q))) return rc;
        WAITCHK(c, wait_stream(c, s, "waiting for the stream"));
    }
    return finish_armours(c, armours_out, armours_cap, n_armours);
}

int rmcv_fit_ellipse(rmcv_ctx* c, const rmcv_point* pts, int n, rmcv_rrect* out)
{
    if (!c || !pts || !out || n < 5) return RMCV_ERR_BAD_ARG;
    // run the blob stage on one contour with every gate open.  The fitted ellipse is read from the contour's own slot (k_fit writes it
    // whatever the ratio and tilt tests then say): a zero-width result has ratio = inf, 0 / 0 has ratio = NaN, and neither may keep a
    // finite ellipse from the caller (the positive list, which the ratio test guards, once did)
    int32_t offs[2] = {0, n};
    hipSetDevice(c->device);
    int rc = load_contours(c, pts, offs, 1);
    if (rc) return rc;
    rmcv_params p;
    rmcv_default_params(&p);
    p.tilt_max = 1e30f;
    p.ratio_lo = -1e30f;
    p.ratio_hi = 1e30f;
    p.area_lo = -1.0;
    p.area_hi = 1e300;
    const Geom g1 = one_frame_geom(c);
    HIPCHK(c, launch_blobs(g1, c->bufs, c->lim, p, c->stream), "k_blobs");
    WAITCHK(c, wait_stream(c, c->stream, "waiting for the context's stream"));
    int32_t kind = 0;
    rmcv_rrect ell;
    HIPCHK(c, hipMemcpy(&kind, c->bufs.slot_kind, 4, hipMemcpyDeviceToHost), "D2H");
    if ((kind & 15) == 0) return fail(c, RMCV_ERR_BAD_ARG, n < 6 ? "contour has fewer than 6 points" : "the contour was not fitted");
    HIPCHK(c, hipMemcpy(&ell, c->bufs.slot_ell, sizeof(rmcv_rrect), hipMemcpyDeviceToHost), "D2H ellipse");
    if (!(std::isfinite(ell.cx) && std::isfinite(ell.cy) && std::isfinite(ell.w) && std::isfinite(ell.h) && std::isfinite(ell.angle)))
        return fail(c, RMCV_ERR_BAD_ARG, "ellipse fit produced NaN");
    *out = ell;
    return RMCV_OK;
}

} // extern "C"
