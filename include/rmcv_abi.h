/*
 * rmcv_abi.h -- C-ABI of the MI355X-native rmcv detection path (librmcv_hip.so).
 *
 * The reference has no plugin/FFI layer: its boundary is the C++ linkage of the
 * static library `rmcv` (/root/reference/CMakeLists.txt:13-16) consumed through
 * include/rmcv.h by executable/main.cpp:172-176.  This header is the thin C-ABI
 * that boundary is re-hosted on: plain pointers and sizes, PODs only, error
 * codes instead of exceptions.  include/rmcv_shim.hpp layers the reference's own
 * rm:: signatures on top of it where OpenCV headers exist.
 *
 * Every entry point runs on the GPU (hand-written HIP, gfx950).  There is no CPU
 * fallback: without a usable device rmcv_ctx_create() fails with
 * RMCV_ERR_NO_DEVICE.
 *
 * Threading (reference: one caller thread, executable/main.cpp:55): a context is
 * single-owner; calls on one context must not overlap.  Input memory is borrowed
 * read-only and must stay valid until the call (or, for the batch API, the
 * matching rmcv_batch_sync) returns.  The library never frees caller memory.
 */
#ifndef RMCV_ABI_H
#define RMCV_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMCV_ABI_VERSION 1

/* error codes (0 = ok) */
#define RMCV_OK 0
#define RMCV_ERR_BAD_ARG (-1)   /* null pointer, bad size, unsupported value            */
#define RMCV_ERR_CAPACITY (-2)  /* an output did not fit; the counts report what is needed */
#define RMCV_ERR_NOMEM (-3)
#define RMCV_ERR_HIP (-4)       /* a HIP runtime call failed: see rmcv_last_error        */
#define RMCV_ERR_NO_DEVICE (-5) /* no gfx950 device: this library has no CPU path        */
#define RMCV_ERR_RCCL (-6)      /* librccl could not be loaded, or an RCCL call failed: see rmcv_comm_last_error */
#define RMCV_ERR_TIMEOUT (-7)   /* work on the GPU did not finish within the deadline (RMCV_OPT_WAIT_TIMEOUT_MS /
                                 * rmcv_pipeline_set_wait_timeout); the message names the kernel or copy enqueued last */

/* rm::camp -- include/core.h:20-23 */
#define RMCV_CAMP_RED 0
#define RMCV_CAMP_BLUE 1
#define RMCV_CAMP_GUIDELIGHT 2
#define RMCV_CAMP_NEUTRAL (-1)

/* morphology after the threshold.  The snapshot does MORPH_CLOSE (src/imgproc.cpp:68-69);
 * the older ExtractColor API (docs/namespacerm.html:854) did a dilate only, which is what
 * BASELINE.json config 2 names. */
#define RMCV_MORPH_NONE 0
#define RMCV_MORPH_DILATE 1
#define RMCV_MORPH_CLOSE 2

typedef struct { int32_t x, y; } rmcv_point;               /* cv::Point, rm::contour element (core.h:87) */
typedef struct { float cx, cy, w, h, angle; } rmcv_rrect;  /* cv::RotatedRect */

typedef struct {            /* rm::lightblob, include/core.h:89-99 */
    float   angle;          /* vertical = 90 */
    int32_t target;         /* rm::camp */
    float   center[2];
    float   vertices[4][2]; /* left-down, left-up, right-up, right-down (core.cpp:265-283) */
    float   size[2];        /* width = min side, height = max side */
} rmcv_lightblob;           /* 56 bytes */

typedef struct {            /* the per-frame data members of rm::armour, include/core.h:110-112 */
    float   icon[4][2];
    float   vertices[4][2]; /* the bit-exact deliverable */
    float   bbox[4];        /* cv::Rect2f bounding_box: x, y, width, height */
    int32_t blob_i, blob_j; /* indices of the two light blobs in the positive list */
} rmcv_armour;              /* 88 bytes */

typedef struct {            /* the literals of executable/main.cpp:172-176 are the defaults */
    int32_t camp;           /* enemy colour, CAMP_BLUE     */
    int32_t lower_bound;    /* 80                          */
    int32_t morph;          /* RMCV_MORPH_CLOSE            */
    float   tilt_max;       /* 70                          */
    float   ratio_lo, ratio_hi; /* 1.5, 80                 */
    double  area_lo, area_hi;   /* 10, 99999               */
    float   angle_diff_max; /* 12                          */
    float   shear_max;      /* 22                          */
    float   length_ratio_max; /* 0.4                       */
    int32_t _pad;
} rmcv_params;

typedef struct {            /* capacities of one context; 0 = default */
    int32_t max_frames;     /* frames per batch                  (256)   */
    int32_t max_width;      /*                                   (1920)  */
    int32_t max_height;     /*                                   (1200)  */
    int32_t max_contours;   /* contours per frame                (2048)  */
    int32_t max_points;     /* contour points per frame          (65536) */
    int32_t max_blobs;      /* positive light blobs per frame    (256)   */
    int32_t max_armours;    /* armours per frame                 (256)   */
    int32_t _pad;
} rmcv_limits;

/* stages of rmcv_batch_run (bit mask); each stage needs the ones below it */
#define RMCV_STAGE_BINARY 1   /* extract_color up to morphologyEx    src/imgproc.cpp:52-69    */
#define RMCV_STAGE_CONTOURS 2 /* findContours                        src/imgproc.cpp:71-72    */
#define RMCV_STAGE_BLOBS 4    /* filter_lightblobs                   src/objdetect.cpp:55-87  */
#define RMCV_STAGE_ARMOURS 8  /* filter_armours                      src/objdetect.cpp:114-166 */
#define RMCV_STAGE_ALL 15
#define RMCV_STAGE_POSE 32     /* solve_PnP + world position per armour, src/mobility.cpp:166-190, executable/main.cpp:183-192;
                                 needs rmcv_pnp_load */
#define RMCV_STAGE_NO_IMAGE 64 /* modifier of RMCV_STAGE_BINARY: do not write the 0/255 byte image (rmcv_batch_get_binary then returns
                                 stale data).  The reference returns `binary` from extract_color but only its debug view reads
                                 it (executable/main.cpp:200-201); a detection-only deployment saves 1 of the 4 bytes per pixel. */
#define RMCV_STAGE_IDENTITY 16 /* affine_correction + flatten + svm->predict per armour (BASELINE config 5),
                                 src/imgproc.cpp:9-35, src/core.cpp:202-216, executable/main.cpp:180-181; needs rmcv_svm_load */

/* per-frame status bits reported by rmcv_batch_counts */
#define RMCV_FRAME_OVF_CONTOURS 1
#define RMCV_FRAME_OVF_POINTS 2
#define RMCV_FRAME_OVF_BLOBS 4
#define RMCV_FRAME_OVF_ARMOURS 8
#define RMCV_FRAME_SLOW_PATH 16 /* informational: the sequential (literal) scanner was used -- the last resort: a frame beyond the mid tier
                                 * too (> 131072 border visits, wider than 2048 px or taller than the row tables) */
#define RMCV_FRAME_MID_PATH 64  /* informational: findContours of this frame ran on the mid tier (tables in global memory: the frame is
                                 * beyond the LDS tables -- > 4096 border visits, > 1024 non-empty words, > 512 contours -- but was not
                                 * handed to the sequential scanner) */
#define RMCV_FRAME_HULL 32      /* legacy matcher: a contour exceeded the hull tables (dimensions > 4096) or is not a closed border */

typedef struct rmcv_ctx rmcv_ctx;

int  rmcv_abi_version(void);
void rmcv_default_params(rmcv_params* p);
void rmcv_default_limits(rmcv_limits* l);

int  rmcv_ctx_create(int device, const rmcv_limits* limits /* nullable */, rmcv_ctx** out);
void rmcv_ctx_destroy(rmcv_ctx* ctx);
const char* rmcv_last_error(const rmcv_ctx* ctx);
/* tuning knobs of a context.  RMCV_OPT_SPARSE_WAVES: wavefronts per frame of the fused sparse kernel (findContours + fits +
 * pairing) in batch runs -- 8 (default): lowest latency of a lone batch; 4: highest throughput when several batches are in flight
 * on different streams (leaves register-file room on every CU for the pixel kernels of the next batches).  Results are identical. */
#define RMCV_OPT_SPARSE_WAVES 1
/* RMCV_OPT_PIXEL_GROUPS: persistent workgroups per CU of the pixel kernel, 1..8 -- 3 (default): fastest for a lone batch (2 is
 * 5 % slower, 4 within 3 %); 2: leaves wave slots and registers on every CU to the kernels of the other batches in flight
 * (two pixel launches of consecutive batches then overlap, i.e. 4 workgroups per CU are resident).  Results are identical. */
#define RMCV_OPT_PIXEL_GROUPS 2
/* RMCV_OPT_FRAME_UPLOAD: how rmcv_extract_color brings the caller's host frame to the device -- 0: the HIP runtime's
 * pageable copy (the fastest of the two safe ways when all is well: 0.186 ms per frame chain against 0.22); 1: through the context's
 * pinned staging buffer (a CPU copy, then DMA: nothing of it depends on the runtime pinning the caller's pages); 3 (default): 0, and
 * 1 WHILE 0 IS SLOW -- the library times the upload of every frame whose byte image it returns, moves to the staging buffer after three
 * slow frames in a row (the runtime's pageable copies were measured 120-250 us slower each for tens of seconds after a large GPU
 * process had exited: the chain 0.28-0.40 ms instead of 0.18), stays there for 512 frames and tries again; 2: the caller's buffer is pinned in place on first sight (hipHostRegister, kept for the context's
 * lifetime, at most 16 buffers) and read by DMA with no CPU copy (0.35 ms) -- for camera SDKs that hand out a fixed ring of
 * frame buffers (the reference's cameras do, hardware/src/daheng.cpp:83).  A pinning is keyed by ADDRESS (and size): the
 * buffers must stay mapped while the context lives, or be handed to rmcv_ctx_forget_frame_buffer BEFORE they are freed -- memory
 * that is freed and mapped again at the same address would otherwise be read through the stale pinning (the same contract
 * hipHostRegister itself has).  Results are identical. */
#define RMCV_OPT_FRAME_UPLOAD 3
/* RMCV_OPT_RUN_AHEAD: 1 (default): rmcv_extract_color also enqueues the blob and armour stages with the parameters the PREVIOUS
 * frame's rmcv_filter_lightblobs / rmcv_filter_armours calls used; when this frame's calls come with the same parameters and the
 * lists rmcv_extract_color / rmcv_filter_lightblobs returned, they hand over results that are already on the host -- the whole
 * chain of executable/main.cpp:172-176 is then one stream sequence with one synchronisation.  0: every call does its own work.
 * Results are identical. */
#define RMCV_OPT_RUN_AHEAD 4
/* RMCV_OPT_CONTOUR_TIER: which form of findContours a frame takes -- 0 (default): chosen per frame (tables in LDS; beyond their
 * capacity the same formulation with tables in global memory, RMCV_FRAME_MID_PATH; beyond that the sequential scanner,
 * RMCV_FRAME_SLOW_PATH); 1: the sequential scanner for every frame; 2: the mid tier for every frame.  A test / diagnosis knob:
 * results are identical. */
#define RMCV_OPT_CONTOUR_TIER 5
/* (option id 6 was RMCV_OPT_HANDOVER, the frame-level hand-over from the pixel kernel to the sparse kernel of rounds 3-4: correct,
 * tested, and measured equal or slower in every schedule, twice -- removed with its progress words, its write-through stores and
 * the second instantiation of every pixel kernel; HISTORY.md 5b has the design) */
/* RMCV_OPT_DENSE_DEFER: 1: with RMCV_OPT_SPARSE_WAVES = 4, a frame beyond the LDS tables of findContours (hundreds of borders:
 * RMCV_FRAME_MID_PATH) is left to a second launch with 8 wavefronts per frame right behind the first; 0 (default): every frame is
 * finished by the first launch.  Results are identical.  Measured: worth 14 % where EVERY frame is that dense, costs
 * 20-30 % where a few frames per batch are (they then run after the others instead of beside them). */
#define RMCV_OPT_DENSE_DEFER 7
/* (option ids 8-10 were round 3's measurement knobs PIXEL_STAGGER, SPARSE_PRIO, PIXEL_TAPER: every setting measured 1.000 or worse;
 * removed together with their kernel branches -- rmcv_ctx_set_option answers RMCV_ERR_BAD_ARG) */
/* RMCV_OPT_PIXEL_HALO_NT: cache policy of the pixel kernel's loads of the rows a strip shares with its neighbours -- 0 (default):
 * cacheable (the neighbouring strip finds them in L2); 1: non-temporal like every other load.  Which is faster depends on the
 * device the process finds itself on and on the workload (the pixel kernels alone gain 3.6 % with 1 on some boxes and
 * lose 1-5 % on others; the whole path moved by -0.4 % at 1280 px and +6 % at 1920 px on a box of the first kind).  A measurement
 * knob; results are identical. */
#define RMCV_OPT_PIXEL_HALO_NT 11
/* RMCV_OPT_OVERLOADS: which functions the reference's UNQUALIFIED abs / atan2 / sin / cos on floats are (src/objdetect.cpp:24, 79,
 * 131-143, 153, 157; src/core.cpp:335-337) -- that depends on the headers the reference's translation units see:
 * bit 0: abs(float) is int abs(int), the argument truncated towards zero (<cmath> alone under libstdc++); bit 1: atan2 / sin / cos
 * are the double functions, the arithmetic around them double.  0 (default): the float overloads everywhere.  Changes results --
 * by design: it follows the reference build it replaces.  INTEGRATION.md has the probe that tells which value a build needs. */
#define RMCV_OPT_OVERLOADS 13
/* RMCV_OPT_PIXEL_SHAPE: which kernel is the pixel stage of a WHOLE batch whose rows are contiguous (stride == 3 w, w % 64 == 0, more
 * strips than half the CUs, lb > 0; anything else is k_binary's whatever this says).
 * 1 (default): k_binary_ws -- ONE 1024-thread workgroup per CU, 8 wavefronts loading strip k+1 while 8 store strip k: alone 8 % faster
 * than k_binary (0.227 against 0.247 ms per 256 x 1280x1024, 5.9 TB/s of the bare copy's 6.25).  It fills the CU: a second launch
 * of it waits for the first, and the 8-wavefront sparse kernel cannot run beside it.
 * 0: k_binary -- 256-thread workgroups, 2-3 per CU, each loading, thresholding, closing and storing its strip in turn; launches of
 * consecutive batches and the sparse kernels share every CU.  A pipeline chooses per batch (rmcv_pipeline_config::hot_contexts)
 * and overrides this.  Same results. */
#define RMCV_OPT_PIXEL_SHAPE 14
/* RMCV_OPT_WAIT_TIMEOUT_MS: the deadline of every wait a call of this context makes for its work on the GPU, in milliseconds
 * (default 5000; 0: none).  The reference's process loop is real-time and latest-wins (executable/main.cpp:157, 169, 197): a drop-in
 * must not park its caller for good behind a kernel that never finishes.  No entry point calls hipStreamSynchronize /
 * hipEventSynchronize: waits poll the stream (spinning for the first 2 ms -- the runtime's own wait parks the thread after ~0.1 ms,
 * and its wake-up costs the per-frame chain another 0.1 ms --, then yielding, then sleeping 0.2 ms at a time) and give up at the
 * deadline with RMCV_ERR_TIMEOUT; rmcv_last_error then names the kernel or copy enqueued last.  After RMCV_ERR_TIMEOUT the work is
 * STILL IN FLIGHT: the buffers handed to the call (frame, binary_out) stay borrowed until a later call on the context succeeds
 * (every call first waits, with the same deadline, for what is in flight) or the context is destroyed; rmcv_ctx_destroy waits
 * once more and, if the work has still not finished, leaks the context's device memory instead of freeing it under a kernel. */
#define RMCV_OPT_WAIT_TIMEOUT_MS 15
/* RMCV_OPT_IMAGE_EXPORT: how rmcv_extract_color brings the byte image to `binary_out` -- 0: the HIP runtime's pageable
 * device-to-host copy, issued once the pixel kernel has finished (the library polls for that with the deadline first): fastest when all
 * is well (0.186 ms per 1280x1024 chain from a C host), but the copy happens INSIDE the runtime's call and was measured at 160-280 us
 * instead of 35 in some processes (bench.py's C-host child: the chain 0.28-0.40 ms); 1: a kernel on the library's side stream copies
 * the image into pinned host memory chunk by chunk, raising a flag per chunk that the host polls in memory, and the library copies
 * the chunks into `binary_out` as they arrive -- no runtime-internal wait anywhere in the chain: 0.190 ms alone, 0.19-0.20 ms where
 * the runtime's copy is slow; 2 (default): 0, and 1 while 0 is slow (three slow frames in a row -> 512 frames on the library's
 * path, then another try; see RMCV_OPT_FRAME_UPLOAD).  Same bytes. */
#define RMCV_OPT_IMAGE_EXPORT 17
/* RMCV_OPT_TEST_SLOW_US: microseconds added to what the library MEASURES of the runtime's two copies (not to the copies): the switch of
 * RMCV_OPT_FRAME_UPLOAD 3 / RMCV_OPT_IMAGE_EXPORT 2 on demand.  A test hook (tests/test_gpu_deadline.py). */
#define RMCV_OPT_TEST_SLOW_US 18
/* RMCV_OPT_TEST_DELAY_US: the next rmcv_extract_color / rmcv_batch_run of the context first holds its stream back for this many
 * microseconds (one sleeping wavefront): a stand-in for a kernel that does not finish in time.  One shot.  A test hook
 * (tests/test_gpu_deadline.py). */
#define RMCV_OPT_TEST_DELAY_US 16
/* RMCV_OPT_INPUT_FORMAT: what the frame pointers of this context hold -- RMCV_INPUT_BGR (0, default): CV_8UC3 BGR, 3 bytes per
 * pixel; or one of the four RMCV_BAYER_* patterns: a raw 8-bit mosaic straight from the sensor, 1 byte per pixel (rows `stride >= w`
 * bytes apart, frames `frame_pitch >= stride * (h - 1) + w` apart, w >= 3, h >= 3; 10/12-bit data, mirror and flip: the three
 * RMCV_OPT_INPUT_* options below).  Every
 * result for a mosaic m is, bit for bit, what the BGR path gives for the frame D(m), the library's demosaic (rmcv_demosaic): bilinear
 * in integers as OpenCV's 8-bit COLOR_Bayer*2BGR is recalled to do it (not pinned against OpenCV), the outermost rows and columns
 * repeating their interior neighbour.  The pixel kernel reads the mosaic itself (k_binary_bayer: 1 B/px instead of 3); no colour frame
 * is ever made.  Batch calls record the format when frames are bound (rmcv_batch_upload, rmcv_batch_set_device_frames,
 * rmcv_pipeline_submit); rmcv_extract_color and rmcv_classify_armours read their frame as a mosaic while it is set.  The legacy matcher
 * (rmcv_find_lightblobs, rmcv_batch_run_legacy, rmcv_pipeline_submit_legacy) votes camps from BGR means and answers RMCV_ERR_BAD_ARG
 * under a Bayer format.
 * The pattern values are those of the Daheng SDK's DX_PIXEL_COLOR_FILTER, so a camera host passes its value straight through; each
 * name gives the top-left 2x2 block of the mosaic.  OpenCV names the same layouts by the second row's pair (as recalled, not pinned
 * here): RMCV_BAYER_RG is its COLOR_BayerBG2BGR, GB its GR, GR its GB, BG its RG. */
#define RMCV_OPT_INPUT_FORMAT 19
#define RMCV_INPUT_BGR 0
#define RMCV_BAYER_RG 1 /* R G / G B */
#define RMCV_BAYER_GB 2 /* G B / R G */
#define RMCV_BAYER_GR 3 /* G R / B G */
#define RMCV_BAYER_BG 4 /* B G / G R */
/* The raw frame AS THE SENSOR DELIVERS IT (Bayer formats only).  A delivered buffer r of w x h samples is read as the 8-bit mosaic
 *     T(r)(x, y) = n(r(mirror ? w-1-x : x, flip ? h-1-y : y)),     n(s) = s for 1-byte samples, (s >> valid_bit) & 0xFF for 2-byte ones
 * and every result for r is, bit for bit, what the 8-bit Bayer path gives for the mosaic T(r): all coordinates (byte image, contour
 * points, blobs, armours, icons, poses) are those of the ORIENTED frame.  The pattern of RMCV_OPT_INPUT_FORMAT stays that of the buffer
 * as delivered (what the SDK reports as the colour filter); the library derives the pattern of T(r): the R site's column parity becomes
 * (w-1-rx) & 1 under mirror, its row parity (h-1-ry) & 1 under flip.  The pixel kernel does all of it while it loads; no oriented or
 * narrowed copy is ever made.
 *   RMCV_OPT_INPUT_SAMPLE_BITS  8 (default) or 16: bytes per sample 1 or 2, little-endian.  With 16, `stride` and `frame_pitch` stay
 *                               in BYTES: stride >= 2 w and even, frame_pitch >= stride (h-1) + 2 w and even, frame pointers 2-byte
 *                               aligned; anything else is RMCV_ERR_BAD_ARG.
 *   RMCV_OPT_INPUT_VALID_BIT    0 (default) .. 4, the Daheng SDK's DX_VALID_BIT values (DX_BIT_0_7 .. DX_BIT_4_11): bits v .. v+7 of a
 *                               16-bit sample are the pixel.  Bits above the window are DROPPED (the literal reading of the vendor
 *                               header's "bit 2~9"); what the SDK's closed DxRaw16toRaw8 does with them is not known and not pinned --
 *                               for data inside its nominal depth (12-bit data with DX_BIT_4_11, 10-bit with DX_BIT_2_9) dropping and
 *                               saturating agree.  Read only with 16-bit samples.
 *   RMCV_OPT_INPUT_ORIENT       bit 0 RMCV_ORIENT_MIRROR (left-right), bit 1 RMCV_ORIENT_FLIP (top-bottom); 0 (default): as delivered.
 * Like the format they are recorded when frames are bound and read per call by rmcv_extract_color / rmcv_classify_armours.  Unknown
 * values are refused and leave the option as it was.  BGR frames have neither: binding or reading a BGR frame while the sample bits
 * are not 8 or the orientation is not 0 is RMCV_ERR_BAD_ARG (the reference's BGR frames are already oriented). */
#define RMCV_OPT_INPUT_SAMPLE_BITS 20
#define RMCV_OPT_INPUT_VALID_BIT 21
#define RMCV_OPT_INPUT_ORIENT 22
#define RMCV_ORIENT_MIRROR 1
#define RMCV_ORIENT_FLIP 2
/* RMCV_OPT_ENHANCE: 1: every frame is read through rm::AutoEnhance (src/imgproc.cpp:77-98), the reference's answer to changing light --
 * 0 (default): as it is.  For a BGR frame f of w x h pixels and the gains (max_gain, min_gain) of rmcv_ctx_set_enhance_gains:
 *     S_c      = exact integer sum of channel c over the frame                                  (c = B, G, R)
 *     m_c      = (double)S_c * (1.0 / (double)(w h))                                            cv::mean, as recalled (not pinned against OpenCV)
 *     meanC3   = (float)(m_B + m_G + m_R) / 3.0f
 *     k        = 2.0f / (max_gain - min_gain);  b = 3.0f - max_gain * k;  g = k * meanC3 + b    float, no contraction
 *     g        = 1.0f + (g - 1.0f) / 4.0f  if -3 <= g <= 1;   0.0f  if g < -3;   unchanged otherwise
 *     LUT_g[i] = saturate_cast<uchar>(pow(i / 255.0, (double)g) * 255.0)                        round half to even; pow(0, 0) = 1
 *     E(f)     = LUT_g applied to every byte of f
 * and every result for f -- byte image, contours, blobs, armours, icons, identities, poses -- is, bit for bit, what the same call gives for
 * the frame E(f) with the option off.  No enhanced frame is ever written: a pass over the frames sums the channels (k_frame_sums), one
 * workgroup per frame builds the table (k_enhance_table; pow is the library's own, pinned against the host libm by the CPU tests), and the
 * pixel kernel (k_binary_enh) and the classifier read the frame through it.  Like the input format the option (with the gains) is recorded
 * when frames are bound and read per call by rmcv_extract_color / rmcv_classify_armours; sums and tables are computed by every run that
 * includes RMCV_STAGE_BINARY, at run time (a run without that stage reads the tables the last one with it left).  Batches with the
 * option take the k_binary shape (never k_binary_ws) and the stand-alone classifier; a pipeline keeps them out of its hot rotation and
 * refuses a submit (RMCV_ERR_BAD_ARG) while its contexts disagree about the option.  The frame is read TWICE (the mean precedes the
 * table): with RMCV_OPT_FRAME_UPLOAD 2 on a device that reads the registered buffer in place, both reads cross the host link.
 * RMCV_ERR_BAD_ARG: binding or reading a frame with the option on while a Bayer input format is set (the mean of a demosaiced frame is no
 * function of the mosaic's sums), and the legacy matcher (rmcv_find_lightblobs, rmcv_batch_run_legacy, rmcv_pipeline_submit_legacy: it
 * votes camps from BGR means) with the option on. */
#define RMCV_OPT_ENHANCE 23
int  rmcv_ctx_set_option(rmcv_ctx* ctx, int option, int value);
/* the gains of RMCV_OPT_ENHANCE: defaults 100, 50 (include/imgproc.h:35).  RMCV_ERR_BAD_ARG (and nothing changes) unless both are finite and
 * differ.  For a pipeline: every slot's context (rmcv_pipeline_context), like the option. */
int  rmcv_ctx_set_enhance_gains(rmcv_ctx* ctx, float max_gain, float min_gain);
/* what the context is set to: RMCV_OPT_ENHANCE and the gains (any pointer may be NULL) -- for code that sets them for one call and puts
 * back what it found (rm::extract_color_enhanced in rmcv_shim.hpp does) */
int  rmcv_ctx_get_enhance(const rmcv_ctx* ctx, int32_t* on, float* max_gain, float* min_gain);
/* launches of k_binary_ws (RMCV_OPT_PIXEL_SHAPE 1) by this process so far: a diagnostic -- an option that is set but whose
 * conditions a batch does not meet falls back to k_binary silently (tests/test_gpu_pixel_shape.py) */
int64_t rmcv_pixel_ws_launches(void);
/* ... and those of them that stored the byte image in DELTA mode: only the 64-byte words that are non-zero now or were when the same
 * context wrote its image last (a context remembers, per row, which words of its image are non-zero; k_binary_ws alone keeps that
 * record, any other writer of the image drops it, and the next k_binary_ws launch stores every byte again).  A diagnostic, like the above. */
int64_t rmcv_pixel_image_delta_launches(void);
/* ... and of those, the launches that stored the bit plane the same way: only the words that are or were non-zero, no pad words, only the row
 * masks that changed.  Possible while plane and image of the context come from the same launches; a pixel launch without the image
 * (RMCV_STAGE_NO_IMAGE) ends that until the next launch with it, which stores the whole plane.  A diagnostic, like the above. */
int64_t rmcv_pixel_plane_delta_launches(void);
/* every device buffer of a context lies between two 4 KiB guard zones holding a fixed pattern: count the damaged ones (0 in a
 * correct build; rmcv_last_error names the first).  Synchronises the context.  A test/diagnosis hook (tests/test_gpu_canary.py). */
int  rmcv_ctx_check_guards(rmcv_ctx* ctx, int32_t* n_damaged);
/* where the last rmcv_extract_color spent its time on the HOST, seven figures in microseconds: us[0] waiting for earlier work, binding,
 * enqueuing the upload; us[1] enqueuing the kernels; us[2] until the byte image's first chunk is home (upload + pixel kernel + PCIe);
 * us[3] the other chunks, copied into binary_out as they arrive; us[4] (the runtime's copy where there is no mapped pinned memory);
 * us[5] waiting for the frame's kernels; us[6] handing the lists over.  cap >= 7; with cap >= 9 also us[7] = the upload path the frame
 * took (0 pageable, 1 pinned staging, 2 registered) and us[8] = the image path (0 the runtime's copy, 1 the export kernel).  A diagnosis
 * hook (tools/frame_chain.c prints the medians). */
int  rmcv_ctx_frame_timing(const rmcv_ctx* ctx, double* us, int cap);
/* drop the pinning RMCV_OPT_FRAME_UPLOAD = 2 made for `frame` (NULL: all of them); drains the context's stream first */
int  rmcv_ctx_forget_frame_buffer(rmcv_ctx* ctx, const void* frame);

/* ---- single frame, host buffers: one call per reference function ---------------------- */

/* rm::extract_color (include/imgproc.h:29, src/imgproc.cpp:50-75).  bgr: CV_8UC3, row pitch
 * `stride` bytes.  binary_out (h*w bytes, 0/255) may be NULL.  Contours come back as CSR in
 * cv::findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) order: offs_out has n_contours+1 entries. */
int rmcv_extract_color(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int camp, int lower_bound,
                       int morph, uint8_t* binary_out, rmcv_point* pts_out, int pts_cap, int32_t* offs_out,
                       int contours_cap, int32_t* n_contours, int32_t* n_points);

/* rm::filter_lightblobs (include/objdetect.h:47-49, src/objdetect.cpp:55-87).  The negative
 * list is returned as contour indices.  blob_src (nullable) = contour index of each positive.
 * Points are what cv::findContours returns: a list with a negative coordinate is refused with
 * RMCV_ERR_BAD_ARG before anything runs (the context stays usable).  The gates compare as the
 * reference does: a zero-width ellipse has ratio = inf, which ratio_hi = +inf admits; 0 / 0 is NaN
 * and goes to the negative list whatever the bounds. */
int rmcv_filter_lightblobs(rmcv_ctx* ctx, const rmcv_point* pts, const int32_t* offs, int n_contours,
                           float tilt_max, float ratio_lo, float ratio_hi, double area_lo, double area_hi,
                           int enemy, rmcv_lightblob* blobs_out, int blobs_cap, int32_t* n_blobs,
                           int32_t* blob_src, int32_t* neg_idx_out, int32_t* n_neg);

/* rm::filter_armours (include/objdetect.h:70-71, src/objdetect.cpp:114-166) */
int rmcv_filter_armours(rmcv_ctx* ctx, const rmcv_lightblob* blobs, int n_blobs, float angle_diff_max,
                        float shear_max, float length_ratio_max, int enemy, rmcv_armour* armours_out,
                        int armours_cap, int32_t* n_armours);

/* cv::fitEllipseDirect on one contour (the step of src/objdetect.cpp:68), for stage-wise parity.
 * RMCV_OK and the fitted ellipse for every contour of six or more points whose result is finite -- zero
 * width or height included (collinear or coinciding points).  RMCV_ERR_BAD_ARG: fewer than six points, a
 * negative coordinate (see rmcv_filter_lightblobs), or a result with a NaN or infinite field, which is
 * not handed out. */
int rmcv_fit_ellipse(rmcv_ctx* ctx, const rmcv_point* pts, int n, rmcv_rrect* out);

/* D(m) of one host mosaic (RMCV_OPT_INPUT_FORMAT) as a host BGR frame, for stage-wise parity and for callers that still want a
 * colour frame (a recorder).  raw: h rows of `stride >= w` bytes; bgr_out: h rows of `out_stride >= 3 w` bytes; w, h >= 3;
 * pattern RMCV_BAYER_RG .. RMCV_BAYER_BG.  Independent of the context's RMCV_OPT_INPUT_FORMAT. */
int rmcv_demosaic(rmcv_ctx* ctx, const uint8_t* raw, int w, int h, int stride, int pattern, uint8_t* bgr_out, int out_stride);
/* D(T(r)) of one delivered host buffer r (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT above, here as arguments): the BGR frame
 * of the ORIENTED mosaic.  pattern: that of r as delivered.  sample_bits 8 or 16 (then `stride >= 2 w` bytes and even, raw 2-byte
 * aligned), valid_bit 0 .. 4 (read only with 16), orient a combination of RMCV_ORIENT_*.  Independent of the context's options. */
int rmcv_demosaic_raw(rmcv_ctx* ctx, const void* raw, int w, int h, int stride, int pattern, int sample_bits, int valid_bit, int orient,
                      uint8_t* bgr_out, int out_stride);

/* ---- rm::CalcGamma / rm::AutoEnhance (include/imgproc.h:33-35, src/imgproc.cpp:37-48, 77-98): see RMCV_OPT_ENHANCE for the arithmetic ---- */
/* LUT_gamma, host-side (no context, no device): the table builder is a function of gamma alone.  RMCV_ERR_BAD_ARG: gamma negative or not
 * finite (rm::AutoEnhance never yields one). */
int rmcv_gamma_lut(float gamma, uint8_t lut[256]);
/* the gamma rm::AutoEnhance derives from a frame's channel sums, host-side.  RMCV_ERR_BAD_ARG: n_pixels < 1, gains not finite or equal. */
int rmcv_enhance_gamma(const uint64_t sums_bgr[3], int64_t n_pixels, float max_gain, float min_gain, float* gamma);
/* rm::CalcGamma on a host image of any channel count (the table acts on bytes): `rows` rows of `row_bytes` bytes, `src_stride` /
 * `dst_stride` >= row_bytes apart; dst == src allowed, as the reference calls it.  RMCV_ERR_BAD_ARG: gamma negative or not finite. */
int rmcv_calc_gamma(rmcv_ctx* ctx, const uint8_t* src, int row_bytes, int rows, int src_stride, float gamma, uint8_t* dst, int dst_stride);
/* E(f) of one host BGR frame (w, h <= 65536), sums and table on the device; out == bgr allowed; gamma_out nullable.  Independent of the
 * context's RMCV_OPT_ENHANCE and gains.  RMCV_ERR_BAD_ARG: gains not finite or equal. */
int rmcv_auto_enhance(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, float max_gain, float min_gain, uint8_t* out, int out_stride,
                      float* gamma_out);

/* ---- batch of independent frames, resident on the device ------------------------------ */

/* copy n_frames host frames (each h rows of `stride` bytes, frames `frame_pitch` bytes apart)
 * into the context's own HBM buffer */
int rmcv_batch_upload(rmcv_ctx* ctx, const uint8_t* frames, int n_frames, int w, int h, int stride,
                      int64_t frame_pitch);
/* or borrow frames that are already in HBM (e.g. a torch tensor's data_ptr) */
int rmcv_batch_set_device_frames(rmcv_ctx* ctx, const void* d_frames, int n_frames, int w, int h, int stride,
                                 int64_t frame_pitch);
/* enqueue the selected stages on `hip_stream` (a hipStream_t, NULL = the context's stream);
 * asynchronous: results are valid after rmcv_batch_sync */
int rmcv_batch_run(rmcv_ctx* ctx, const rmcv_params* p, int stages, void* hip_stream);
int rmcv_batch_sync(rmcv_ctx* ctx);
/* same, but brackets every kernel with HIP events on that stream and, after syncing, reports the
 * milliseconds of each: stage_ms[0]=binary, [1]=contours, [2]=blobs, [3]=armours, [4]=total */
int rmcv_batch_run_timed(rmcv_ctx* ctx, const rmcv_params* p, int stages, void* hip_stream, float stage_ms[5]);

/* per-frame result sizes (arrays of n_frames entries, any may be NULL) */
int rmcv_batch_counts(rmcv_ctx* ctx, int32_t* n_contours, int32_t* n_points, int32_t* n_blobs,
                      int32_t* n_armours, int32_t* status);
int rmcv_batch_get_binary(rmcv_ctx* ctx, int frame, uint8_t* binary_out);
int rmcv_batch_get_contours(rmcv_ctx* ctx, int frame, rmcv_point* pts_out, int pts_cap, int32_t* offs_out,
                            int contours_cap, int32_t* n_contours, int32_t* n_points);
int rmcv_batch_get_blobs(rmcv_ctx* ctx, int frame, rmcv_lightblob* blobs_out, int cap, int32_t* n_blobs,
                         int32_t* blob_src);
/* the gamma each frame bound was read with by the last run (RMCV_OPT_ENHANCE; the one of the last rmcv_extract_color as frame 0): the
 * first min(cap, n_frames) entries; 1 for every frame while the option is off, and before the first such run of a context.
 * Synchronises the context. */
int rmcv_batch_get_gammas(rmcv_ctx* ctx, float* gamma_out, int cap);
/* all armours of the batch, frame-major: frame_offs has n_frames+1 entries */
int rmcv_batch_get_armours(rmcv_ctx* ctx, rmcv_armour* armours_out, int cap, int32_t* frame_offs,
                           int32_t* n_total);
/* device views for a zero-copy hand-over to a collective (RCCL gather of the detections):
 * d_armours[frame][per_frame_cap], d_counts[frame] */
int rmcv_batch_device_views(rmcv_ctx* ctx, void** d_armours, void** d_counts, int32_t* per_frame_cap,
                            int32_t* n_frames);

/* ---- windowed detection: look only where the target was (rm::utils::GetROI, src/core.cpp:218-263; extract_color on image(roi);
 * the ROI argument of rm::solve_PnP, src/mobility.cpp:168-185) ------------------------------------------------------------------
 * A windowed batch: the n frames bound (frame_w x frame_h, stride, frame_pitch as ever), ONE window size win_w x win_h for the batch and
 * one requested origin (x, y) per frame, int32 of any value.  The EFFECTIVE origin of a frame is computed on the device, in one place
 * (k_window_origins), written to a per-frame table and read from there by every consumer:
 *     x_eff = clamp(x, 0, frame_w - win_w) & ~15          y_eff = clamp(y, 0, frame_h - win_h)
 * The clamp is there because origins may come from a tracker on the device that the host never reads; the snap to 16 pixels (48 bytes)
 * keeps window rows 16-byte aligned for the pixel kernel's loader -- it is part of the semantics and always applied, whichever loader runs.
 * Every result for frame f is, bit for bit, what the same run gives for the cropped image frame[y_eff : y_eff + win_h, x_eff : x_eff +
 * win_w] bound as a whole frame -- what the reference computes on image(roi): the byte image is win_h x win_w; contours, light blobs and
 * armours are in WINDOW coordinates; RMCV_STAGE_IDENTITY clamps icons to win_w - 1, win_h - 1; the legacy matcher votes camps from the
 * crop's means.  RMCV_STAGE_POSE follows mobility.cpp:172, 182-185: every image point is vertex + (float)x_eff, vertex + (float)y_eff
 * in float before undistortion.  NOT promised: equality with whole-frame detection translated into the window -- window edges cut
 * contours, and the ellipse fit is not bit-translation-invariant (on the synthetic stream, 512x384 windows centred on the first
 * whole-frame armour: an armour in 64 of 64 windows, the whole-frame armour's exact vertices in 9).  rmcv_armours_to_frame is a
 * convenience, not a second detection.
 * The pixel pass reads 3 win_w win_h bytes per frame instead of 3 w h (k_binary_win: the pixel kernel at the effective origins; k_binary's
 * shape, never k_binary_ws); everything behind it runs on window-sized planes.
 * RMCV_ERR_BAD_ARG, with a message: windows with a Bayer RMCV_OPT_INPUT_FORMAT or with RMCV_OPT_ENHANCE (crop-then-demosaic and
 * crop-then-AutoEnhance have other border and mean semantics); win_w / win_h < 1, larger than the frames, or larger than the context's
 * limits; no frames bound.  One window size per batch. */
/* after the frames are bound (rmcv_batch_upload / rmcv_batch_set_device_frames; a new binding returns to whole frames): origins =
 * n_frames host points, copied.  win_w == 0: back to whole frames (origins ignored).  Synchronises the context. */
int rmcv_batch_set_windows(rmcv_ctx* ctx, const rmcv_point* origins, int win_w, int win_h);
/* the same with the origins in device memory (n_frames rmcv_point), BORROWED: every run that includes RMCV_STAGE_BINARY reads them again,
 * on its stream, in front of its pixel pass -- a tracker kernel enqueued before the run may have rewritten them */
int rmcv_batch_set_device_windows(rmcv_ctx* ctx, const void* d_origins, int win_w, int win_h);
/* the effective origins of the frames bound (the first min(cap, n_frames); (0, 0) without windows) and the window size (0, 0 without);
 * any pointer may be NULL with cap 0.  Synchronises the context. */
int rmcv_batch_get_windows(rmcv_ctx* ctx, rmcv_point* eff_out, int cap, int32_t* win_w, int32_t* win_h);
/* device view of the effective-origin table (n_frames rmcv_point; NULL without windows), valid behind the run on its stream: for a
 * consumer on the device that moves results to frame coordinates */
int rmcv_batch_device_windows(rmcv_ctx* ctx, void** d_eff, int32_t* win_w, int32_t* win_h);
/* Host-side helpers of the locked-target loop (no context, no device), detect -> track -> GetROI -> window -> detect:
 * rm::utils::GetROI, verbatim: points = n (x, y) float pairs; boundingRect on float points (floor of min, floor of max - floor of min + 1;
 * n == 0: the empty rect), + previous.x / .y (previous[4] = x, y, w, h; NULL: zeros); unless both scales are 1: margins
 * (int)((double)w * scale_w / 2.0), (int)((double)h * scale_h / 2.0), x -= mw, y -= mh, w += 2 mw, h += 2 MW -- the reference adds the
 * WIDTH's margin to the height (core.cpp:238), mirrored; x, y < 0 -> 0 (sizes unchanged); x + w >= frame_w -> w = frame_w - x - 1, same
 * for h; a negative size -> {0, 0, 0, 0}.  out[4] = x, y, w, h. */
int rmcv_get_roi(const float* points, int n, float scale_w, float scale_h, int frame_w, int frame_h, const int32_t previous[4], int32_t out[4]);
/* the requested origin of a win_w x win_h window centred on rect[4]: (x + w / 2 - win_w / 2, y + h / 2 - win_h / 2), integer arithmetic
 * (the library clamps and snaps it: see above) */
int rmcv_window_origin(const int32_t rect[4], int win_w, int win_h, int32_t out_xy[2]);
/* window -> frame coordinates: icon, vertices and bbox.x / .y of every armour + ((float)x, (float)y), one f32 add each (a convenience:
 * see NOT promised above) */
int rmcv_armours_to_frame(rmcv_armour* armours, int n, int x, int y);

/* ---- per-frame detection keys: the enemy colour arrives with every frame (serial_package::target, executable/main.cpp:142, carried in
 * frame_package to the process loop) ---------------------------------------------------------------------------------------------------
 * A batch is frame f = the next frame of stream f; in a match half of the streams hunt red and half blue, and their cameras are not
 * exposed alike.  With keys set, frame f is detected with camp camps[f] and lower bound lower_bounds[f] (or the run's p->lower_bound);
 * rmcv_params::camp and ::lower_bound of the run are otherwise not read, every other field of rmcv_params stays per batch (morph too).
 * Everything frame f produces -- byte image, bit plane, contours, light blobs including `target`, armours, with RMCV_STAGE_IDENTITY /
 * RMCV_STAGE_POSE identities, icons and poses, behind a tracker every track byte -- equals, bit for bit, what the same batch run gives for
 * frame f with p->camp = camps[f] and p->lower_bound = lower_bounds[f].
 * The raw values are any int32 (a device-side producer may write them).  The EFFECTIVE key of a frame is computed on the device, in one
 * place (k_frame_keys, in front of the pixel pass), written to a per-frame table and read from there by every consumer:
 *     channel pair (src/imgproc.cpp:56-65):  camp 2 -> G - R;  camp 1 -> B - R;  every other value -> R - B
 *     bound (inRange(gray, lb, 255) on a saturated u8 difference):  lb <= 0 -> every pixel passes;  lb > 255 -> none;  otherwise a - b >= lb
 *     enemy label: blobs[].target is camps[f] verbatim (objdetect.cpp:83), and pairing compares against the same value (:124-129)
 * The pixel pass is k_binary_camp (with windows k_binary_camp_win): k_binary's shape, the key read once per 32-row strip; never
 * k_binary_ws, which stays the faster path for a batch of ONE colour -- keys are for fleets that are mixed.
 * RMCV_ERR_BAD_ARG, with a message, before anything is enqueued -- the families windows refuse too: keys with a Bayer
 * RMCV_OPT_INPUT_FORMAT (the mosaic kernel takes one camp per run); with RMCV_OPT_ENHANCE (its threshold table folds one bound per run);
 * with the legacy matcher (rmcv_batch_run_legacy, rmcv_pipeline_submit_legacy: it votes a camp per blob); no frames bound. */
/* the effective key of (camp, lower_bound): out = channel A, channel B (byte inside a BGR pixel), effective bound 1 .. 256, all-pass flag.
 * Host-side, no context, no device: the function the prologue kernel runs, compiled for the host */
int rmcv_frame_key(int32_t camp, int32_t lower_bound, int32_t out[4]);
/* after the frames are bound (a new binding returns to per-run keys, as it returns to whole frames): n_frames host values each, copied.
 * lower_bounds NULL: every frame uses the run's p->lower_bound.  camps NULL: back to per-run keys.  Synchronises the context. */
int rmcv_batch_set_frame_camps(rmcv_ctx* ctx, const int32_t* camps, const int32_t* lower_bounds);
/* the same with the tables in device memory (n_frames int32 each; d_lower_bounds nullable), BORROWED: every run that includes
 * RMCV_STAGE_BINARY reads them again, on its stream, in front of its pixel pass */
int rmcv_batch_set_device_frame_camps(rmcv_ctx* ctx, const void* d_camps, const void* d_lower_bounds);
/* the effective keys of the last run with the pixel pass, keys_out[f] = {channel A, channel B, bound, all-pass} for the first min(cap,
 * n_frames) frames; without per-frame keys that is the run's key for every frame.  Synchronises the context. */
int rmcv_batch_get_frame_keys(rmcv_ctx* ctx, int32_t* keys_out /* [cap][4] */, int cap);

/* ---- icon classifier: the "next" row of the path (executable/main.cpp:178-181) ------------------------ */
#define RMCV_SVM_FEATURES 1200 /* 20 x 20 x BGR, executable/main.cpp:180 ({20, 20}), core.cpp:202-216 */
/* linear one-vs-one C_SVC as cv::ml::SVM keeps it after training (executable/svm/optimizer.cpp:16-19): one weight
 * vector + rho per class pair (i<j, row-major), class labels in training order.  n_class <= 8. */
int rmcv_svm_load(rmcv_ctx* ctx, const float* weights /* [n_class*(n_class-1)/2][1200] */, const double* rho,
                  const int32_t* labels, int n_class);
/* single frame: identity_out[i] = predict(flatten(affine_correction(frame, armours[i].icon, {20,20})));
 * armours[i].icon is clamped to the frame in place, exactly as the reference does.  icons_out (n*1200 B) may be NULL. */
int rmcv_classify_armours(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, rmcv_armour* armours, int n,
                          int32_t* identity_out, uint8_t* icons_out);
/* batch: identities in the order of rmcv_batch_get_armours (after a run that included RMCV_STAGE_IDENTITY) */
int rmcv_batch_get_identities(rmcv_ctx* ctx, int32_t* identity_out, int cap, int32_t* n_total);
int rmcv_batch_get_icons(rmcv_ctx* ctx, int frame, uint8_t* icons_out, int cap_armours, int32_t* n_armours);

/* ---- one model per colour, or per robot: a table of models, one chosen per frame on the device -------------------
 * The reference's loop owns one classifier per enemy colour, svm_red and svm_blue (executable/main.cpp:21-22).  A context holds a table
 * of up to RMCV_SVM_MAX_MODELS models; a batch classifies frame f with entry rmcv_frame_model(idx[f], n_models) of it.
 *
 * rmcv_svm_load_models copies the table, waiting for the context's work first.  Entry 0 is also what every single-model consumer reads
 * (rmcv_classify_armours, rmcv_svm_predict, rmcv_svm_predict_dataset, and every batch with selection off): exactly what
 * rmcv_svm_load(models[0]) gives.  rmcv_svm_load is a table of one.  Either call switches per-frame selection off; so does a new binding
 * of frames.  Refused with RMCV_ERR_BAD_ARG and a message, before any GPU work: n_models outside 1 .. RMCV_SVM_MAX_MODELS; an entry with
 * a null pointer, with n_class outside 2 .. 8, or with a weight or rho that is not finite (the message names the entry).
 *
 * Selection on: frame f's identities, icons and clamped icon vertices are, byte for byte, what the same batch gives after
 * rmcv_svm_load(models[eff(idx[f])]).  Models may differ in n_class and labels.  The indices are read on the run's stream, in front of
 * the classifier, by every run with RMCV_STAGE_IDENTITY: host indices are validated and copied (one outside the table: RMCV_ERR_BAD_ARG,
 * nothing changes); device indices are BORROWED and may hold any int32 -- every value outside 0 .. n_models - 1 reads model 0.
 *
 * Camps as indices: the raw camp values are RMCV_CAMP_RED 0, RMCV_CAMP_BLUE 1, guide light 2 and neutral -1.  With the table
 * {svm_red, svm_blue} the device camps table of rmcv_pipeline_submit_camps, or rmcv_tracker_device_camps, can be handed over as the model
 * index table as it is: red streams read svm_red, blue streams svm_blue, every other value model 0. */
#define RMCV_SVM_MAX_MODELS 64
typedef struct {
    const float*   weights; /* [n_class*(n_class-1)/2][1200] */
    const double*  rho;     /* [n_class*(n_class-1)/2] */
    const int32_t* labels;  /* [n_class] */
    int32_t n_class;        /* 2 .. 8 */
    int32_t reserved;
} rmcv_svm_model;
int rmcv_frame_model(int32_t idx, int32_t n_models);   /* the rule: host-side, no context, no device */
int rmcv_svm_load_models(rmcv_ctx* ctx, const rmcv_svm_model* models, int n_models);
/* idx: n_frames int32 of the host, copied; an index outside the table: RMCV_ERR_BAD_ARG, nothing changes; NULL: off */
int rmcv_batch_set_frame_models(rmcv_ctx* ctx, const int32_t* idx);
/* d_idx: n_frames int32 in DEVICE memory, BORROWED, read again by every run with RMCV_STAGE_IDENTITY; NULL: off */
int rmcv_batch_set_device_frame_models(rmcv_ctx* ctx, const void* d_idx);
/* the EFFECTIVE indices of the last such run for the first min(cap, n_frames) frames; 0 everywhere when off.  Synchronises the context. */
int rmcv_batch_get_frame_models(rmcv_ctx* ctx, int32_t* out, int cap);
/* rmcv_svm_predict with entry `model` of the table (0 .. n_models - 1; anything else: RMCV_ERR_BAD_ARG) */
int rmcv_svm_predict_model(rmcv_ctx* ctx, int model, const uint8_t* samples, int n, int32_t* identity_out);

/* ---- training the icon classifier (executable/svm/optimizer.cpp: C_SVC, LINEAR, trainAuto) -------------------------
 * The model rmcv_svm_load takes, trained from rows as rmcv_batch_get_icons / rmcv_classify_armours hand them out (1200 raw bytes each,
 * features = the bytes as f32, unscaled).  OpenCV's solver is not pinned, so the library defines its own exact rule, modelled on
 * cv::ml::SVM (first-order SMO on the exact integer Gram matrix; rmcv_amd/csrc/device_svm.h is its one source for host and device):
 * rmcv_svm_train runs it on the GPU, rmcv_svm_train_host sequentially on the CPU, and the two agree bit for bit in every output.
 * Folds of the grid search come from the caller's permutation, so a result is a function of its arguments alone. */
#define RMCV_SVM_MAX_GRID 16   /* C values of one grid search */
#define RMCV_SVM_MAX_DF 28     /* decision functions of 8 classes */
#define RMCV_SVM_MAX_FOLDS 64
#define RMCV_SVM_MAX_SAMPLES 8192      /* rows of one training set (the Gram matrix is rows x rows int32) */
#define RMCV_SVM_MAX_PAIR_SAMPLES 2048 /* rows of two classes together (one pair problem lives in one workgroup's LDS) */
typedef struct {
    double  eps;       /* stop when the maximal violation falls below it; >= 0, finite       (1e-3: optimizer.cpp's TermCriteria) */
    int32_t max_iter;  /* SMO iterations of one pair problem, >= 1; a model cut off here is a valid result               (1000) */
    int32_t k_fold;    /* folds of the grid search, <= RMCV_SVM_MAX_FOLDS; <= 1: no search, plain training at c_grid[0]    (10) */
    int32_t n_c;       /* 1 .. RMCV_SVM_MAX_GRID entries of c_grid; 1: plain training                                       (6) */
    int32_t reserved;  /* 0 */
    double  c_grid[RMCV_SVM_MAX_GRID]; /* each > 0 and finite           (0.1 * 5^k, k = 0 .. 5: cv::ml::SVM's default grid for C) */
} rmcv_svm_train_params;
typedef struct {
    double  best_c;                           /* the C of the returned model ...                                                   */
    int32_t best_index;                       /* ... and its grid entry: the lowest cv_errors, the earlier entry on a tie          */
    int32_t n_df;                             /* n_class * (n_class - 1) / 2                                                       */
    int32_t cv_errors[RMCV_SVM_MAX_GRID];     /* misclassified test rows over all folds per grid entry; -1: no search was run      */
    int32_t iterations[RMCV_SVM_MAX_DF];      /* of the returned model's pair problems (i < j, row-major) ...                      */
    int32_t converged[RMCV_SVM_MAX_DF];       /* ... 0: cut off at max_iter                                                        */
    double  objective[RMCV_SVM_MAX_DF];       /* ... their dual objectives, 1/2 a'Qa - e'a                                         */
    double  phase_ms[6];                      /* Gram; the search's solver, weights and predict; the returned model's solver and
                                               * weights: GPU time between events (rmcv_svm_train), wall time (rmcv_svm_train_host)  */
    double* alpha_out;                        /* IN, may be NULL: [n_df][n], the returned model's alphas by dataset row (0 for rows
                                               * of other classes)                                                                 */
    char    message[128];                     /* why the call was refused (RMCV_ERR_BAD_ARG); empty otherwise                      */
} rmcv_svm_train_report;
void rmcv_svm_train_defaults(rmcv_svm_train_params* out);
/* samples u8 [n][1200], responses i32 [n] (any values: the distinct ones in ascending order become labels_out, 2 .. 8 of them),
 * perm i32 [n] or NULL (identity): fold k of K tests rows perm[floor(k n / K) .. floor((k + 1) n / K)) and trains on the rest.
 * params NULL: the defaults.  weights_out [n_df][1200], rho_out [n_df], labels_out [n_class] are sized by the caller for 8 classes or
 * for what it knows; report may be NULL.  RMCV_ERR_BAD_ARG with a message (rmcv_last_error, report->message), decided before any GPU
 * work: fewer than 2 or more than 8 classes; perm not a permutation; a fold whose training part lacks a class; n or two classes' rows
 * beyond the limits above; a parameter outside its range.  The device workspace is allocated per call and freed on every path; waits
 * run against the context's deadline (RMCV_ERR_TIMEOUT names the kernel). */
int rmcv_svm_train(rmcv_ctx* ctx, const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm,
                   const rmcv_svm_train_params* params, float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out,
                   rmcv_svm_train_report* report);
/* the same without a context and without a GPU: the sequential form of the same header */
int rmcv_svm_train_host(const uint8_t* samples, const int32_t* responses, int n, const int32_t* perm,
                        const rmcv_svm_train_params* params, float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out,
                        rmcv_svm_train_report* report);
/* gram_out [n][n] int32: the exact dot products of the rows (each <= 1200 * 255^2 < 2^31); n <= RMCV_SVM_MAX_SAMPLES */
int rmcv_svm_gram(rmcv_ctx* ctx, const uint8_t* samples, int n, int32_t* gram_out);
int rmcv_svm_gram_host(const uint8_t* samples, int n, int32_t* gram_out);
/* identity_out[r] = the loaded model's (rmcv_svm_load) class label of row r of samples u8 [n][1200], in the arithmetic of RMCV_STAGE_IDENTITY */
int rmcv_svm_predict(rmcv_ctx* ctx, const uint8_t* samples, int n, int32_t* identity_out);
int rmcv_svm_predict_host(const float* weights, const double* rho, const int32_t* labels, int n_class, const uint8_t* samples, int n,
                          int32_t* identity_out);

/* device-side, frame-major compaction into caller-provided HBM (e.g. torch tensors): d_armours_out has room
 * for `cap` armours, d_frame_offs for n_frames+1 int32 (last entry = total, which may exceed cap: then only the
 * first `cap` were written).  Asynchronous on hip_stream.  This is the payload of the multi-GPU gather. */
int rmcv_batch_compact_armours(rmcv_ctx* ctx, void* d_armours_out, int cap, void* d_frame_offs, void* hip_stream);

/* ---- multi-GPU: the gather of the armour lists (BASELINE config 4) ------------------------------------------------
 * One process per GPU; frames are independent, so there is no collective on the data path.  After rmcv_batch_run +
 * rmcv_batch_compact_armours every rank holds a fixed-size record in HBM ([frame_offs : n_frames+1 int32, padded to 16 B |
 * armours : cap x 88 B], the layout of rmcv_amd/dist.py); rmcv_gather moves the records of all ranks to the root with RCCL
 * point-to-point transfers (each peer's own xGMI link to the root), asynchronously on the caller's stream.
 * RCCL is loaded on first use (librccl.so.1); a single-GPU user never needs it.  The reference is single-process
 * (executable/main.cpp:45-107): this is the north star's addition, not a reference interface. */
#define RMCV_COMM_ID_BYTES 128
typedef struct rmcv_comm rmcv_comm;
/* rank 0: make the group's id; hand the 128 bytes to the other ranks by any means (file, socket, MPI, a launcher's store) */
int  rmcv_comm_unique_id(uint8_t id_out[RMCV_COMM_ID_BYTES]);
/* every rank, collectively: join the group of n_ranks on its own GPU `device` */
int  rmcv_comm_create(const uint8_t id[RMCV_COMM_ID_BYTES], int n_ranks, int rank, int device, rmcv_comm** out);
void rmcv_comm_destroy(rmcv_comm* comm);
int  rmcv_comm_info(const rmcv_comm* comm, int32_t* n_ranks, int32_t* rank);
const char* rmcv_comm_last_error(const rmcv_comm* comm /* NULL: the loader's message */);
/* every rank, collectively: d_record (record_bytes, device memory) -> root's d_recv (n_ranks x record_bytes, rank order; ignored
 * on the other ranks).  Enqueued on hip_stream; the root's buffer is complete when that stream reaches this point. */
int  rmcv_gather(rmcv_comm* comm, const void* d_record, int64_t record_bytes, void* d_recv, int root, void* hip_stream);

/* ---- legacy per-contour matcher: the "next" row SURVEY 8f-2 (src/objdetect.cpp:9-53, 89-112) ---------- */
typedef struct {            /* the float arguments of rm::MatchLightBlob / rm::FindLightBlobs, include/objdetect.h:22-37 */
    float   min_ratio, max_ratio; /* aspect-ratio bounds (strict compares, src/objdetect.cpp:20)                */
    float   tilt_angle;           /* maximal tilt, always judged on the fitted ellipse (src/objdetect.cpp:23-24) */
    float   min_area, max_area;   /* contourArea bounds (strict compares, src/objdetect.cpp:12)                  */
    int32_t fit_ellipse;          /* 1: box = cv::fitEllipseDirect, 0: box = cv::minAreaRect (src/objdetect.cpp:16) */
} rmcv_legacy_params;

/* cv::minAreaRect on one contour (the call of src/objdetect.cpp:16, :69): convex hull + rotating calipers.  pts must be
 * a border as cv::findContours returns it (8-connected, closed: every column of its bounding box holds a point);
 * anything else is RMCV_ERR_BAD_ARG. */
int rmcv_min_area_rect(rmcv_ctx* ctx, const rmcv_point* pts, int n, rmcv_rrect* out);
/* rm::MatchLightBlob (include/objdetect.h:22-23, src/objdetect.cpp:9-28): *matched = 1 and *box_out set when the
 * contour passes every gate.  A list with a negative coordinate is RMCV_ERR_BAD_ARG (see rmcv_filter_lightblobs). */
int rmcv_match_lightblob(rmcv_ctx* ctx, const rmcv_point* pts, int n, const rmcv_legacy_params* lp, rmcv_rrect* box_out,
                         int32_t* matched);
/* rm::FindLightBlobs (include/objdetect.h:35-37, src/objdetect.cpp:30-53): every matching contour becomes a light blob
 * whose camp is voted from the mean B/G/R of `bgr` over the contour's bounding rectangle.  blob_src / boxes_out nullable. */
int rmcv_find_lightblobs(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const rmcv_point* pts,
                         const int32_t* offs, int n_contours, const rmcv_legacy_params* lp, rmcv_lightblob* blobs_out,
                         int blobs_cap, int32_t* n_blobs, int32_t* blob_src, rmcv_rrect* boxes_out);
/* rm::LightBlobOverlap (include/objdetect.h:62, src/objdetect.cpp:89-112).  Host-side predicate over caller memory (a few
 * float compares, no device work).  right == n reads past the end in the reference (its bound check is off by one):
 * that case is RMCV_ERR_BAD_ARG here. */
int rmcv_lightblob_overlap(const rmcv_lightblob* blobs, int n, int left, int right, int32_t* overlap);
/* batch: like rmcv_batch_run, but RMCV_STAGE_BLOBS runs FindLightBlobs with `lp` on every frame's contours (blobs of all
 * camps, in findContours order); RMCV_STAGE_ARMOURS then pairs the blobs whose camp is p->camp. */
int rmcv_batch_run_legacy(rmcv_ctx* ctx, const rmcv_params* p, const rmcv_legacy_params* lp, int stages, void* hip_stream);

/* ---- armour pose: the "next" row SURVEY 8f-3 (src/mobility.cpp:166-190, executable/main.cpp:183-192) -------- */
typedef struct {               /* what the process loop hands to rm::solve_PnP and the world transform */
    double camera_matrix[9];   /* cammat, row-major 3x3                        executable/main.cpp:7-10  */
    double dist[5];            /* discof: k1 k2 p1 p2 k3                       executable/main.cpp:11-13 */
    double gripper2camera[16]; /* h_gripper2camera, row-major 4x4              executable/main.cpp:14-19 */
    float  square_w, square_h; /* exactSize                                    executable/main.cpp:184 {27, 27} */
} rmcv_pnp_config;
void rmcv_default_pnp_config(rmcv_pnp_config* c); /* the literals of executable/main.cpp:7-19, 184 */
int  rmcv_pnp_load(rmcv_ctx* ctx, const rmcv_pnp_config* cfg);
/* single frame: for each armour rvec/tvec = rm::solve_PnP(armour.vertices, cammat, discof, exactSize) and
 * position = base2gripper * (gripper2camera * [tvec; 1]) (executable/main.cpp:186-192).  base2gripper: row-major 4x4
 * (h_base2gripper of executable/main.cpp:170), NULL = identity.  Outputs n x 3 doubles each, any may be NULL. */
int  rmcv_locate_armours(rmcv_ctx* ctx, const rmcv_armour* armours, int n, const double* base2gripper, double* rvecs,
                         double* tvecs, double* positions);
/* batch: one base2gripper per frame (n_frames x 16 doubles, host; default identity), used by RMCV_STAGE_POSE */
int  rmcv_batch_set_base2gripper(rmcv_ctx* ctx, const double* mats, int n_frames);
/* batch: poses in the order of rmcv_batch_get_armours (after a run that included RMCV_STAGE_POSE) */
int  rmcv_batch_get_poses(rmcv_ctx* ctx, double* rvecs, double* tvecs, double* positions, int cap, int32_t* n_total);

/* ---- tracker: the "next" row SURVEY 8f-4 (src/core.cpp:51-162, executable/main.cpp:57-88) --------------------------------
 * Two forms exist.  These are host-side functions over caller memory, one target or one list at a time, for a host that tracks a
 * single camera itself; the device-resident tracker further down (rmcv_tracker_*) keeps the state of a whole batch of streams in
 * HBM and steps it behind a batch without the host.  The two share every operation but ONE: the Jacobi rotation inside
 * cv::solve(DECOMP_SVD) calls hypot, which these functions (like the CPU oracle they are tested against) take from the host's libm
 * -- not correctly rounded, and not the same from one libm to the next -- and the device tracker takes from the library's own
 * correctly rounded pm_hypot.  The filter fields (state, covariances, gain) of the two forms may therefore differ in the last bits;
 * everything discrete (matching, counts, lost counts, histograms, timestamps) is the same. */
/* rm::armour::max_IoU (src/core.cpp:144-162): *index = the armour of `list` with the largest IoU of bounding boxes with `self`
 * (first on ties, -1 when none overlaps), *iou = that IoU */
int rmcv_max_iou(const rmcv_armour* self, const rmcv_armour* list, int n, int32_t* index, float* iou);
/* rm::armour::identity_max (src/core.cpp:124-142): soft-max vote over an identity histogram; ids ascending (the reference keeps a
 * std::map<int,int>); *max_id = -1 for an empty histogram */
int rmcv_identity_max(const int32_t* ids, const int32_t* counts, int n, int32_t* max_id, double* prob);

/* rm::armour as the tracking thread holds it, with every field readable (include/core.h:101-129).  The filter is
 * cv::KalmanFilter(6, 6, 0, CV_64F) (src/core.cpp:21): state [x y z vx vy vz], matrices row-major 6x6 doubles. */
#define RMCV_TRACK_IDS 32
typedef struct {
    rmcv_armour armour;      /* icon / vertices / bounding_box of the observation the target was created from (update() never refreshes them) */
    int64_t timestamp;       /* ticks of the last observation (core.h:114) */
    int32_t lost_count;      /* core.h:115 */
    int32_t identity;        /* core.h:117 */
    double  position[3];     /* core.h:116 */
    int32_t initialized;     /* core.h:107 */
    int32_t n_ids;           /* identity_history (core.h:103): ids ascending, as a std::map iterates */
    int32_t ids[RMCV_TRACK_IDS], counts[RMCV_TRACK_IDS];
    double  measurement[6];  /* core.h:106 */
    double  state_pre[6], state_post[6];
    double  transition[36], measurement_matrix[36], process_noise_cov[36], measurement_noise_cov[36];
    double  error_cov_pre[36], error_cov_post[36], gain[36];
} rmcv_track;
/* a freshly detected armour as executable/main.cpp:178-194 leaves it: constructor (filter initialised, src/core.cpp:21) +
 * identity, position, timestamp assigned; call rmcv_track_reset next, as main.cpp:195 does */
void rmcv_track_init(rmcv_track* t, const rmcv_armour* a, int32_t identity, int64_t timestamp, const double position[3]);
/* rm::armour::reset (src/core.cpp:51-72); the process loop uses (5e-5, 0.5, 0.05) */
void rmcv_track_reset(rmcv_track* t, double process_noise, double measurement_noise, double error);
/* rm::armour::update(const armour& new_observation) (src/core.cpp:74-108).  tick_frequency = cv::getTickFrequency() */
int  rmcv_track_update(rmcv_track* t, const rmcv_track* observation, double tick_frequency);
/* rm::armour::update(int64 new_timestamp) (src/core.cpp:110-122) */
int  rmcv_track_predict(rmcv_track* t, int64_t new_timestamp, double tick_frequency);
/* one pass of the tracking thread (executable/main.cpp:60-85) over this frame's observations: targets whose bounding box
 * overlaps an observation by IoU > 0.5 take it (and it leaves the list), the others age (dropped after 26 misses -- with
 * the reference's skip of the target behind an erased one) or coast; what is left of the observations becomes new targets.
 * *n_obs is 0 afterwards.  Any number of observations; RMCV_ERR_CAPACITY when the list the pass would leave behind (surviving
 * targets + unmatched observations, counted by a dry run before anything is changed) exceeds cap -- N targets re-observed by N
 * matching observations need cap >= N, as the reference's vectors do -- or when a target would see its 33rd distinct identity
 * (lists handed back consistent). */
int  rmcv_track_step(rmcv_track* tracking, int32_t* n_tracking, int cap, rmcv_track* observations, int32_t* n_obs, double tick_frequency);

/* ---- device-resident tracker: detect, track and re-window without the host -----------------------------------------
 * A tracker holds, in HBM, the tracking state of n_streams independent camera streams: frame f of every batch stepped against it is
 * the next frame of stream f.  Per stream: up to track_cap rmcv_track records, their number, a status word and ONE requested window
 * origin; per track a side record, the frame-coordinate vertices of the observation that created the track or matched it last
 * (rmcv_track::armour is never refreshed by update(), mirrored: the side record alone knows where the target is now).
 * One STEP, behind a run that included RMCV_STAGE_ARMOURS, does for every stream f:
 *  1. observations: the frame's armours in rmcv_batch_get_armours order, moved to frame coordinates as rmcv_armours_to_frame(a, n,
 *     x_eff, y_eff) does ((0, 0) without windows), each rmcv_track_init(armour, identity, timestamp, position) + rmcv_track_reset(
 *     process_noise, measurement_noise, error); identity from the run's RMCV_STAGE_IDENTITY, else -1; position from its
 *     RMCV_STAGE_POSE, else (0, 0, 0); timestamp: one int64 per step (all frames of a batch are one instant on different cameras);
 *  2. one pass of the tracking thread, exactly rmcv_track_step's (no observation: nothing happens, not even ageing) -- with the
 *     library's correctly rounded hypot in the filter (see the note above rmcv_max_iou);
 *  3. capacity: what the pass would leave behind is counted first, on indices.  If surviving targets + unmatched observations exceed
 *     track_cap, or a matched target would see its 33rd distinct identity, the stream's step is NOT APPLIED AT ALL -- lists, side
 *     records and origin stay as they were -- and RMCV_TRACKER_OVF is set in the stream's status, sticky until rmcv_tracker_reset;
 *  4. next window (win_w > 0): the target is the stream's track with the greatest timestamp, lowest index on ties; its side record's
 *     four vertices go through rmcv_get_roi(v, 4, roi_scale_w, roi_scale_h, frame_w, frame_h, NULL) and rmcv_window_origin(rect,
 *     win_w, win_h); the int32 pair becomes the stream's requested origin (k_window_origins clamps and snaps it in front of the next
 *     pixel pass, as for any origin).  No tracks: the origin stays.  (A step without observations changes no list but still does 4.)
 * Every byte of every rmcv_track, count, status, side record and origin equals the CPU restatement
 * (tests/track_ref.py: the oracle's tracker with only hypot replaced by an independent correctly rounded one). */
#define RMCV_TRACKER_OVF 1
#define RMCV_TRACKER_MAX_CAP 64
typedef struct rmcv_tracker rmcv_tracker;
typedef struct {
    int32_t n_streams;         /* camera streams = frames of every batch stepped against the tracker   (256)  */
    int32_t track_cap;         /* tracks per stream, 1 .. RMCV_TRACKER_MAX_CAP                         (64)   */
    double  process_noise, measurement_noise, error; /* rmcv_track_reset's                (5e-5, 0.5, 0.05)   */
    double  tick_frequency;    /* timestamp ticks per second, cv::getTickFrequency()                   (1e9)  */
    float   roi_scale_w, roi_scale_h; /* rmcv_get_roi's                                              (1, 1)   */
    int32_t frame_w, frame_h;  /* the streams' frames                                          (1280, 1024)   */
    int32_t win_w, win_h;      /* the window the origins are for; win_w == 0: track only, no origins (0, 0)   */
} rmcv_tracker_config;
void rmcv_default_tracker_config(rmcv_tracker_config* c);
/* RMCV_ERR_BAD_ARG: n_streams < 1, track_cap out of range, noises / tick_frequency not finite or tick_frequency <= 0, frame or window
 * sizes out of range (a window larger than the frame).  cfg NULL: the defaults. */
int  rmcv_tracker_create(int device, const rmcv_tracker_config* cfg, rmcv_tracker** out);
void rmcv_tracker_destroy(rmcv_tracker* trk);   /* waits for the step in flight first */
const char* rmcv_tracker_last_error(const rmcv_tracker* trk);
/* all lists empty, status cleared (origins stay).  Waits for the step in flight. */
int  rmcv_tracker_reset(rmcv_tracker* trk);
/* the initial requests: n_streams host points, copied.  Waits for the step in flight. */
int  rmcv_tracker_set_origins(rmcv_tracker* trk, const rmcv_point* origins);
/* device view of the requested origins (n_streams rmcv_point): what a caller hands to rmcv_batch_set_device_windows /
 * rmcv_pipeline_submit_windows.  Owned by the tracker. */
int  rmcv_tracker_device_origins(rmcv_tracker* trk, void** d_origins);
/* per-stream detection keys (see "per-frame detection keys"): a stream's colour is a property of the stream.  n_streams host values each,
 * copied into tables the tracker owns; lower_bounds NULL: the run's p->lower_bound; camps NULL: off.  Waits for the step in flight.
 * rmcv_pipeline_submit_tracked on such a tracker is an rmcv_pipeline_submit_camps with the tracker's tables; rmcv_batch_track needs nothing
 * new (the run before it had its keys: rmcv_batch_set_device_frame_camps with the tables below, or host values) */
int  rmcv_tracker_set_camps(rmcv_tracker* trk, const int32_t* camps, const int32_t* lower_bounds);
/* the tracker's two tables (n_streams int32 each), for a device-side writer and for rmcv_batch_set_device_frame_camps; either may be NULL */
int  rmcv_tracker_device_camps(rmcv_tracker* trk, void** d_camps, void** d_lower_bounds);
/* enqueue one step on `hip_stream` (NULL: the context's stream) behind the context's last run, on the batch bound to it.  Never
 * synchronises.  RMCV_ERR_BAD_ARG with a message: the batch's n_frames != n_streams; its frame size differs from the config's; the last
 * run had no RMCV_STAGE_ARMOURS; windows are set and their size differs from the config's; context and tracker on different devices. */
int  rmcv_batch_track(rmcv_ctx* ctx, rmcv_tracker* trk, int64_t timestamp, void* hip_stream);
/* synchronous downloads (they wait for the step in flight, with a 5 s deadline: RMCV_ERR_TIMEOUT).  counts: the first min(cap,
 * n_streams) entries, either pointer may be NULL.  get: one stream's list (RMCV_ERR_CAPACITY when *n > cap; tracks_out /
 * last_vertices_out ([cap][4][2] floats) / origin_out nullable). */
int  rmcv_tracker_counts(rmcv_tracker* trk, int32_t* n_tracking, int32_t* status, int cap);
int  rmcv_tracker_get(rmcv_tracker* trk, int stream, rmcv_track* tracks_out, int cap, int32_t* n, float* last_vertices_out, rmcv_point* origin_out);
/* the same step for ONE stream on the CPU over host arrays (no device; the same source the kernel is compiled from): tracks
 * [track_cap], last_vertices [track_cap][4][2], *n_tracking, *status, *origin are read and updated; the observations are n_obs armours
 * in WINDOW coordinates with the effective origin (x_eff, y_eff) they are moved by, identities (NULL: -1) and positions (n_obs x 3
 * doubles; NULL: zeros).  cfg->n_streams is not read.  A C host gets the device tracker's exact semantics for a single camera. */
int  rmcv_tracker_step_host(const rmcv_tracker_config* cfg, rmcv_track* tracks, float* last_vertices, int32_t* n_tracking, int32_t* status,
                            rmcv_point* origin, const rmcv_armour* armours, int n_obs, const int32_t* identities, const double* positions,
                            int x_eff, int y_eff, int64_t timestamp);

/* ---- aiming: rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance (src/mobility.cpp:36-82,127-164) ---------------
 * Host functions that need no device, no context and no tracker: the reference's statements one by one, evaluated left to right as
 * written, the transcendentals from the library's pinned functions (the same bits on the host and on the device), sqrt IEEE.
 * A NaN result is THE quiet NaN 0x7FF8000000000000, here and in every rmcv_aim (the sign of a computed NaN is the machine's).
 * Lengths of a translation vector are cm, v0 m/s, g m/s^2, angles in: rad, angles out (pitch, yaw): DEGREES, times s -- the reference's.
 * Mirrored as written: COMPENSATE_CLASSIC takes cos() of the launch angle it has just converted to degrees
 * (mobility.cpp:147,150), and SolveGEA's `h` -- documented in metres -- is divided by 100 like a length in cm (:145,147). */
#define RMCV_COMPENSATE_NONE 0     /* rm::COMPENSATE_NONE    (include/mobility.h:20) */
#define RMCV_COMPENSATE_CLASSIC 1  /* rm::COMPENSATE_CLASSIC */
#define RMCV_COMPENSATE_NI 2       /* rm::COMPENSATE_NI: the reference returns NAN before it writes anything (mobility.cpp:153) */
/* the launch angle (rad) of the root with the smaller magnitude; NAN without a real root */
double rmcv_projectile_angle(double v0, double g, double d, double h);
/* returns the flight time; gea_out = {pitch, yaw}, untouched for RMCV_COMPENSATE_NI (a mode that is none of the three falls through the
 * reference's switch with pitch = time = 0, and does here) */
double rmcv_solve_gea(const double tvec[3], double g, double v0, double h, float offset_x, float offset_y, double angle_offset, int mode,
                      double gea_out[2]);
/* motor_angle (rad) is not checked, here or in rmcv_aim_input: the pinned tangent is NaN for a non-finite argument and for one of 3.37e9 rad
 * or more (|x * 2 / pi| >= 2^31 - 1, pinned_math.h "the conversion's edge"), the same on the host and on the device, and so is the height */
double rmcv_delta_height(const double tvec[3], double motor_angle, float offset_y, double angle_offset);
double rmcv_distance(const double tvec[3]);
/* a rigid 4x4 (row-major) [R t; 0 1] -> [R^T  -R^T t; 0 1]; each entry of R^T t is summed left to right.  out == m allowed. */
int    rmcv_rigid_inverse(const double m[16], double out[16]);

/* ---- device-resident aiming: one rmcv_aim per stream behind the tracker's step, without the host ---------------------
 * With aiming on, every step of the tracker (rmcv_batch_track, rmcv_pipeline_submit_tracked) is followed, on the same stream and in front
 * of the tracker's event, by an AIM STEP with `now` = the step's timestamp; rmcv_tracker_aim enqueues the aim step alone.  Per stream:
 *  1. candidates: the tracks j of the current list with lost_count <= max_lost whose identity is allowed -- identity i in 0..30: bit i of
 *     identity_mask; any other identity (-1 included): bit 31;
 *  2. source: initialized == 0: p = position, v = 0; else RMCV_AIM_SRC_FILTER: p = state_post[0..2], v = state_post[3..5];
 *     RMCV_AIM_SRC_MEASUREMENT: p = measurement[0..2], v = measurement[3..5];
 *  3. lead: dt = (double)(now - timestamp) / tick_frequency + latency_s;  q_i = p_i + v_i * dt;  cam = world2camera . [q; 1], each row
 *     ((W0 q0 + W1 q1) + W2 q2) + W3 * 1.0;  h = height (RMCV_AIM_HEIGHT_FIXED) or rmcv_delta_height(cam, motor_angle, offset_y,
 *     angle_offset) (RMCV_AIM_HEIGHT_DELTA);  (pitch, yaw, t) = rmcv_solve_gea(cam, ...);  then lead_iterations times: t not finite: stop;
 *     else q = p + v * (dt + t), and cam, h and the solution again;  distance = rmcv_distance(cam);  RMCV_AIM_NO_SOLUTION when the final
 *     pitch or t is not finite.  A NaN state (a matched update with dt = 0 makes one) runs through and comes out NaN;
 *  4. pick: RMCV_AIM_PICK_WINDOW: the candidate with the greatest timestamp, lowest index on ties (the tracker's own window rule
 *     restricted to candidates); RMCV_AIM_PICK_NEAREST: the smallest distance, NaN counting as +infinity, lowest index on ties;
 *  5. record: the stream's rmcv_aim; `point` is cam of the last solution (the led target in the camera's frame, cm).  No candidate:
 *     track = identity = -1, lost_count = 0, status = RMCV_AIM_NO_TARGET, every double +0.0.
 * A stream with RMCV_TRACKER_OVF is aimed like any other, on the list as it stands.  The positions are in whatever frame the tracker's
 * observations came in; world2camera brings them to the camera frame rm::SolveGEA expects (a pipeline's RMCV_STAGE_POSE has
 * base2gripper = identity, so positions are in the gripper's frame and world2camera = rmcv_rigid_inverse(gripper2camera)).
 * Aiming reads the tracker's state and never writes it.  Every byte of every record equals tests/aim_ref.c. */
#define RMCV_AIM_NO_TARGET 1
#define RMCV_AIM_NO_SOLUTION 2
#define RMCV_AIM_HEIGHT_FIXED 0
#define RMCV_AIM_HEIGHT_DELTA 1
#define RMCV_AIM_SRC_FILTER 0
#define RMCV_AIM_SRC_MEASUREMENT 1
#define RMCV_AIM_PICK_WINDOW 0
#define RMCV_AIM_PICK_NEAREST 1
typedef struct {
    double  g, v0, height;       /* m/s^2, m/s, cm   (9.8, 15, 0: the project's defaults -- the reference gives none) */
    float   offset_x, offset_y;  /* cm  (0, 0: mobility.h:56,97) */
    double  angle_offset;        /* rad (0) */
    double  latency_s;           /* (0) */
    int32_t mode;                /* RMCV_COMPENSATE_NONE (mobility.h:97); RMCV_COMPENSATE_NI is refused */
    int32_t height_mode;         /* RMCV_AIM_HEIGHT_FIXED */
    int32_t source;              /* RMCV_AIM_SRC_FILTER */
    int32_t pick;                /* RMCV_AIM_PICK_WINDOW */
    int32_t lead_iterations;     /* 0 .. 4 (1) */
    int32_t max_lost;            /* (25) */
    int32_t overloads;           /* bit 0 as bit 0 of RMCV_OPT_OVERLOADS: the unqualified abs(double) of mobility.cpp:74,150 is int abs(int),
                                    the argument truncated toward zero (a NaN argument: 0); 0: fabs (0) */
    uint32_t identity_mask;      /* (0xFFFFFFFF) */
} rmcv_aim_config;               /* 80 bytes */
typedef struct { double world2camera[16]; double motor_angle; } rmcv_aim_input;   /* per stream, 136 bytes; (identity, 0) */
typedef struct {
    int32_t track, identity, lost_count, status;   /* index in the stream's current list; RMCV_AIM_* */
    double  pitch, yaw, flight_time, distance, point[3];
} rmcv_aim;                                        /* 72 bytes */
void rmcv_default_aim_config(rmcv_aim_config* c);
/* aiming on (cfg) or off (NULL: no aim kernel is launched; the records stay as they are).  Waits for the step in flight; allocates on first
 * use.  RMCV_ERR_BAD_ARG with a message: a number not finite, an enum out of range, mode == RMCV_COMPENSATE_NI, lead_iterations outside
 * 0..4, max_lost < 0. */
int  rmcv_tracker_set_aim(rmcv_tracker* trk, const rmcv_aim_config* cfg);
/* n_streams inputs, copied (NULL: the defaults).  Waits for the step in flight. */
int  rmcv_tracker_set_aim_inputs(rmcv_tracker* trk, const rmcv_aim_input* inputs);
/* device view of the inputs (n_streams rmcv_aim_input): the caller may write them on its own stream before a submit.  Owned by the tracker. */
int  rmcv_tracker_device_aim_inputs(rmcv_tracker* trk, void** d_inputs);
/* enqueue the aim step alone on `hip_stream` (NULL: the null stream), on the lists as they are; never synchronises.  RMCV_ERR_BAD_ARG when
 * aiming is off. */
int  rmcv_tracker_aim(rmcv_tracker* trk, int64_t now, void* hip_stream);
/* the first min(cap, n_streams) records; synchronous (the tracker's 5 s deadline).  Zeros until the first aim step. */
int  rmcv_tracker_get_aims(rmcv_tracker* trk, rmcv_aim* out, int cap);
/* device view of the records (n_streams rmcv_aim).  Owned by the tracker. */
int  rmcv_tracker_device_aims(rmcv_tracker* trk, void** d_aims);
/* seed or restore one stream's current list: n <= track_cap tracks (RMCV_ERR_CAPACITY beyond) and their side records ([n][4][2] floats;
 * NULL: zeros).  Synchronous; status and origin stay as they are. */
int  rmcv_tracker_put(rmcv_tracker* trk, int stream, const rmcv_track* tracks, int n, const float* last_vertices);
/* the aim step for ONE stream on the CPU (no device; the same source the kernel is compiled from): n <= RMCV_TRACKER_MAX_CAP tracks,
 * input NULL: the defaults.  RMCV_ERR_BAD_ARG: what rmcv_tracker_set_aim refuses, or tick_frequency not finite and positive. */
int  rmcv_aim_step_host(const rmcv_aim_config* cfg, double tick_frequency, const rmcv_track* tracks, int n, const rmcv_aim_input* input,
                        int64_t now, rmcv_aim* out);

/* ---- per-stream gimbal attitude: packet in, aim out, host only submits ------------------------------------------------
 * Every frame of the reference's process loop carries what the MCU link sent for it (serial_package, executable/main.cpp:24-28): the enemy
 * colour and the gimbal's rotation.  process_function turns the rotation into h_base2gripper (main.cpp:170) and puts every armour's
 * position into the base frame with it (main.cpp:189); the tracking thread filters those.  With attitude on, an ATTITUDE STEP (k_attitude,
 * one lane per stream) runs in front of a tracked batch and writes, per stream f, from the stream's rmcv_attitude or its 24-byte packet:
 *  1. with a packet (main.cpp:120-143): valid iff pkt[0] == 0x38 and pkt[23] == rmcv_crc8(pkt, 23).  A valid one sets attitude[f] -- yaw,
 *     pitch, roll the little-endian f32 at bytes 3, 11, 15, each ((double)deg * 3.141592653589793) / 180.0 -- and, where the tracker's camp
 *     table is on (rmcv_tracker_set_camps), camps[f] = (pkt[1] & 1) ? RMCV_CAMP_RED : RMCV_CAMP_BLUE.  A rejected one leaves both as they
 *     were (the reference's `continue`: the last good package stays in use) and adds one to packet_errors[f];
 *  2. B = rmcv_homogeneous(rmcv_euler_to_matrix(attitude[f]), 0) -> base2gripper[f] of the batch's context (skipped without pose tables,
 *     rmcv_pnp_load).  The matrices are the BATCH's: the table rmcv_batch_set_base2gripper writes is not touched and is in force again
 *     from the context's next binding of frames (or the next rmcv_batch_set_base2gripper) on;
 *  3. world2camera[f] = rmcv_rigid_inverse(B x gripper2camera), the 4x4 product's entries ((r0 c0 + r1 c1) + r2 c2) + r3 c3; motor_angle[f]
 *     stays (RMCV_ATT_MOTOR_KEEP) or becomes attitude[f].pitch (RMCV_ATT_MOTOR_PITCH);
 *  4. a valid packet with a non-finite angle runs through and comes out NaN (every NaN that leaves is the quiet NaN), as in the aim step.
 *     So does an angle of 3.37e9 rad (1.93e11 degrees) or more: the pinned sine and cosine reduce by a quadrant number held in an int, and
 *     where |angle * 2 / pi| >= 2^31 - 1 they return NaN on the host and on the device alike (pinned_math.h, "the conversion's edge");
 * The step is enqueued on the batch's pixel stream: in front of k_frame_keys / k_window_origins (the camps it may write are read there) and
 * behind an event wait for the tracker's previous step (the aim inputs it writes are read by that step's k_aim) -- with attitude on that
 * wait is made for whole-frame trackers (win_w == 0) too, which otherwise have none.  Nothing blocks: host_blocking_calls stays 0.
 * Every byte written equals tests/attitude_ref.c. */
typedef struct { double roll, pitch, yaw; } rmcv_attitude;          /* radians = rm::euler<double>{x, y, z}; 24 bytes */
#define RMCV_ATT_MOTOR_KEEP 0
#define RMCV_ATT_MOTOR_PITCH 1
typedef struct { double gripper2camera[16]; int32_t motor_angle_mode; int32_t reserved; } rmcv_attitude_config;   /* 136 bytes */
#define RMCV_SERIAL_PACKET_BYTES 24
/* host functions (no device; the source the kernel is compiled from).  R = (Rz(yaw) . Ry(pitch)) . Rx(roll), row-major, every entry
 * ((a0 b0 + a1 b1) + a2 b2) with pinned sin / cos (rm::euler<double>::to_matrix, include/core.h:66-84) */
int     rmcv_euler_to_matrix(const rmcv_attitude* a, double R[9]);
/* rm::utils::homogeneous (src/core.cpp:406-416): R and t in an identity 4x4 */
int     rmcv_homogeneous(const double R[9], const double t[3] /* NULL: zeros */, double H[16]);
/* rm::lookup_CRC (hardware/src/serialport.cpp:9-18): polynomial 0x31, MSB first, init 0; n <= 0 or data NULL: 0 */
uint8_t rmcv_crc8(const uint8_t* data, int n);
int     rmcv_serial_decode(const uint8_t pkt[24], int32_t* camp, rmcv_attitude* att);   /* 1 valid, 0 rejected (nothing written), <0 bad arg */
/* the inverse, for replay hosts and tests: header, bit 0 of byte 1 (camp RMCV_CAMP_RED: 1, RMCV_CAMP_BLUE: 0; anything else is
 * RMCV_ERR_BAD_ARG), the three floats, the CRC; every other byte 0 */
int     rmcv_serial_encode(int32_t camp, float yaw_deg, float pitch_deg, float roll_deg, uint8_t pkt[24]);
/* the attitude step for ONE stream on the CPU.  pkt, camp nullable (no packet; camp table off); base2gripper nullable (no pose tables).
 * RMCV_ERR_BAD_ARG: a null pointer elsewhere, or a config rmcv_tracker_set_attitude refuses */
int     rmcv_attitude_step_host(const rmcv_attitude_config* cfg, const uint8_t* pkt, rmcv_attitude* att, int32_t* camp,
                                int32_t* packet_errors, double base2gripper[16], rmcv_aim_input* input);
void rmcv_default_attitude_config(rmcv_attitude_config* c);          /* gripper2camera of rmcv_default_pnp_config, RMCV_ATT_MOTOR_KEEP */
/* attitude on (cfg) or off (NULL: no kernel is launched; the tables stay as they are).  Waits for the step in flight; allocates the
 * attitude tables (zero attitudes, zero packet_errors) and the aim tables on first use.  RMCV_ERR_BAD_ARG with a message: an entry of the
 * matrix not finite, motor_angle_mode out of range. */
int  rmcv_tracker_set_attitude(rmcv_tracker* trk, const rmcv_attitude_config* cfg);
/* n_streams attitudes, copied (NULL: zeros); packet_errors are left alone.  Waits for the step in flight. */
int  rmcv_tracker_set_attitudes(rmcv_tracker* trk, const rmcv_attitude* attitudes);
/* the first min(cap, n_streams) attitudes and packet_errors (either pointer may be NULL); synchronous.  Zeros before first use. */
int  rmcv_tracker_get_attitudes(rmcv_tracker* trk, rmcv_attitude* out, int32_t* packet_errors, int cap);
/* device view of the attitudes (n_streams rmcv_attitude): a device-side producer may write them on its own stream.  Owned by the tracker. */
int  rmcv_tracker_device_attitudes(rmcv_tracker* trk, void** d_attitudes);
/* the first min(cap, n_streams) aim inputs as the device holds them; synchronous.  The defaults before first use. */
int  rmcv_tracker_get_aim_inputs(rmcv_tracker* trk, rmcv_aim_input* out, int cap);
/* the first n_frames matrices of the table the bound batch's RMCV_STAGE_POSE reads (the attitude step's, or rmcv_batch_set_base2gripper's);
 * synchronous.  RMCV_ERR_BAD_ARG without rmcv_pnp_load; RMCV_ERR_CAPACITY beyond max_frames. */
int  rmcv_batch_get_base2gripper(rmcv_ctx* ctx, double* mats, int n_frames);
/* context path: enqueue the attitude step for the bound batch on `hip_stream` (NULL: the context's stream), in front of rmcv_batch_run.
 * d_packets: n_streams x 24 bytes in DEVICE memory, borrowed until the step has run, or NULL.  Never synchronises.  RMCV_ERR_BAD_ARG with
 * a message, before anything is enqueued: attitude off, no frames bound, n_frames != n_streams, a tracker on another device. */
int  rmcv_batch_attitude(rmcv_ctx* ctx, rmcv_tracker* trk, const void* d_packets, void* hip_stream);

/* ---- per-stream camera model and ballistics: a mixed fleet's batch ---------------------------------------------------
 * cammat, discof and h_gripper2camera (executable/main.cpp:8-19), the plate size handed to rm::solve_PnP (main.cpp:184) and the matrix
 * positions are placed with (main.cpp:189) belong to ONE physical camera on ONE robot, and so do the muzzle velocity and the offsets
 * rm::SolveGEA is called with.  A batch whose frame f is the next frame of stream f may take its streams from different robots: the camera
 * becomes a TABLE in the context, selected per frame on the device; the attitude step's hand-eye matrix and the aim step's config become
 * per-stream tables of the tracker.  With the tables off every entry point produces the bytes it produced before they existed.
 *
 * The rule from a raw index to the table entry used, the ONE function k_pnp runs (pixel_plan.h: frame_camera_eff):
 *     effective = ((uint32_t)idx < (uint32_t)n_cameras) ? idx : 0
 * so whatever a device-side producer writes, a frame reads an entry of the table.  Frame f's rvec, tvec and position are, byte for byte,
 * what the same batch gives with rmcv_pnp_load(cams[effective(idx[f])]).  rmcv_locate_armours (one frame) always uses camera 0. */
int  rmcv_frame_camera(int32_t idx, int32_t n_cameras);   /* the rule: host-side, no context, no device */
/* n_cameras configs, copied (1 .. limits.max_frames, else RMCV_ERR_BAD_ARG with a message); waits for the context's work first.  Entry 0
 * is what rmcv_pnp_load would have loaded; rmcv_pnp_load is "a table of one".  Either call switches per-frame selection off. */
int  rmcv_pnp_load_cameras(rmcv_ctx* ctx, const rmcv_pnp_config* cams, int n_cameras);
/* after the frames are bound: n_frames indices, host, copied.  A value outside 0 .. n_cameras - 1 is RMCV_ERR_BAD_ARG with a message and
 * nothing changes.  NULL: selection off, every frame uses camera 0.  A new binding of frames returns to off, as for camps and windows. */
int  rmcv_batch_set_frame_cameras(rmcv_ctx* ctx, const int32_t* idx);
/* ... n_frames int32 in DEVICE memory, BORROWED: read again by every run that includes RMCV_STAGE_POSE, on that run's stream.  Any value
 * (the rule above).  NULL: selection off. */
int  rmcv_batch_set_device_frame_cameras(rmcv_ctx* ctx, const void* d_idx);
/* the EFFECTIVE indices of the first min(cap, n_frames) frames in the last run with RMCV_STAGE_POSE since selection was set; 0 for every
 * frame without selection; synchronous */
int  rmcv_batch_get_frame_cameras(rmcv_ctx* ctx, int32_t* out, int cap);
/* the attitude step's hand-eye matrix per stream: n_streams x 16 doubles, host, copied; step 3 above then reads stream f's own matrix in
 * place of rmcv_attitude_config::gripper2camera (rmcv_batch_attitude and the tracked submits alike).  NULL: back to the config's one.
 * Waits for the step in flight.  RMCV_ERR_BAD_ARG with a message naming the stream: an entry not finite.  Keeping this table and the
 * contexts' camera table consistent is the caller's job, as it is for rmcv_pnp_config against rmcv_attitude_config. */
int  rmcv_tracker_set_stream_cameras(rmcv_tracker* trk, const double* gripper2camera);
/* the aim step's config per stream: n_streams rmcv_aim_config, host, copied; k_aim then reads stream f's own.  NULL: back to
 * rmcv_tracker_set_aim's one.  Waits for the step in flight.  RMCV_ERR_BAD_ARG with a message: aiming off; an entry rmcv_tracker_set_aim
 * would refuse (the message names the stream).  Every byte stream f's steps write equals rmcv_attitude_step_host / rmcv_aim_step_host
 * called with stream f's matrix or config. */
int  rmcv_tracker_set_aim_configs(rmcv_tracker* trk, const rmcv_aim_config* cfgs);

/* ---- pipelined batches: the process loop behind the ABI ------------------------------------------------------------------------
 * The reference's process_function is a `while (1)` that takes the newest camera frame, runs the three detection calls and hands
 * the armours on (executable/main.cpp:163-209).  Its batch form on one MI355X: `depth` batches in flight, each in a context of its
 * own; the HBM-bound pixel kernels of consecutive batches alternate over `pixel_streams` HIP streams (two launches overlap: each
 * hides the other's ramp and tail), the latency-bound per-frame kernels run on `sparse_streams` higher-priority streams; a batch's
 * two halves and the reuse of its context are chained by events, the armour lists are compacted frame-major on the device and (by
 * default) copied to pinned host memory behind that.  This is the schedule bench.py's figure is measured on -- owned by the library:
 * a C or C++ host gets it with three calls.
 *
 *     rmcv_pipeline_create(0, &limits, NULL, &pl);
 *     for (;;) { rmcv_pipeline_submit(pl, d_frames, n, w, h, stride, pitch, &params, RMCV_STAGE_ALL, &ticket);
 *                if (ticket >= depth) rmcv_pipeline_collect(pl, ticket - depth + 1, armours, cap, frame_offs, &n_total); }
 *
 * Single-owner like a context: calls on one pipeline must not overlap.  The frames handed to submit are borrowed until the ticket
 * is collected (or waited for).  HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read once
 * when the HIP runtime starts: the default schedule wants 8 or more (kernels of two batches that share a queue cannot overlap).
 * The library does NOT touch the process environment (round 4's load-time setenv is gone): a host that wants the pipelined schedule
 * calls rmcv_hw_queues_hint() before its first HIP call, or exports GPU_MAX_HW_QUEUES=12 itself; rmcv_pipeline_get_info reports
 * what the variable reads and what the schedule wants.
 *
 * rmcv_pipeline_submit NEVER BLOCKS the host (round 5): it allocates nothing (the ring's contexts hold everything a batch of the
 * limits' size needs from rmcv_pipeline_create on), synchronises nothing and copies nothing synchronously -- a change of geometry
 * (planes zeroed, frame order recomputed) and a slot's change of finishing stream are enqueued work and event waits on the GPU.
 * rmcv_pipeline_info::host_blocking_calls counts the exceptions: it stays 0. */
typedef struct rmcv_pipeline rmcv_pipeline;
typedef struct {            /* 0 in any field = the default; rmcv_default_pipeline_config fills them in */
    int32_t depth;          /* batches in flight = slots (records, tickets) = contexts in the ring (8)  */
    int32_t pixel_streams;  /*                                                                  (2)  */
    int32_t sparse_streams; /*                                                                  (4)  */
    int32_t armour_cap;     /* armours a batch's compacted list holds                (8 per frame)   */
    int32_t sparse_waves;   /* RMCV_OPT_SPARSE_WAVES of the ring's contexts   (4 if depth >= 3 else 8) */
    int32_t pixel_groups;   /* RMCV_OPT_PIXEL_GROUPS                          (2 if depth >= 2 else 3) */
    int32_t host_results;   /* 1: every list is copied to pinned host memory behind its compaction (collect then copies from there);
                             * 2: lists stay on the device until collected                      (1)  */
    int32_t dense_streams;  /* streams for a batch's frames beyond findContours' LDS tables (a lit window, hundreds of specks): WHILE a
                             * few frames per batch are that dense (1 .. max_frames / 8 in the batch that last left the slot; needs
                             * host_results = 1 and sparse_waves = 4), the per-frame launch leaves them to a second launch with 8
                              * wavefronts per frame that runs -- with the compaction behind it -- on one of these streams: the sparse
                             * stream goes on with the next batch instead of waiting for a 0.5-1 ms frame (one lit window per batch:
                             * 1.3 x the plain step time without, 1.01 x with).  Batches without such frames, and batches full of them,
                             * run as if this were off.  -1: off                                                              (4)  */
    int32_t hot_contexts;   /* WHILE the batches are calm -- no frame of the record that last came back went beyond findContours' LDS
                             * tables, no classifier / pose stage asked for -- the batches take turns at the first `hot_contexts`
                             * contexts of the ring (slot, record and ticket window stay `depth` deep) and run the wave-specialised pixel
                             * kernel (RMCV_OPT_PIXEL_SHAPE 1).  What a batch writes with ordinary stores and reads right back -- the
                             * 46 MB bit plane first of all -- then stays in the 256 MB Infinity Cache instead of going to HBM and
                             * back: 3-8 % on the plain stream.  A context's next batch waits for its last one's list, so dense
                             * batches (0.5-1 ms of sparse work) would stall the pixel stream: those run one context per slot, as
                             * with -1.  Needs host_results = 1 and depth >= 4.  0: DERIVED per geometry -- as many contexts as keep
                             * the batches' bit planes within 200 MB of the cache, 3 .. depth - 1 (4 at 256 x 1280x1024, 3 at
                             * 256 x 1920x1200); n: exactly n (3 .. depth - 1); -1: off                                       (0)  */
    int32_t _reserved;
} rmcv_pipeline_config;
typedef struct {
    int32_t depth, pixel_streams, sparse_streams, armour_cap, sparse_waves, pixel_groups, host_results, dense_streams;
    int32_t max_frames;
    int32_t hw_queues_env;     /* what GPU_MAX_HW_QUEUES reads in this process (0: unset) */
    int32_t hw_queues_wanted;  /* 1 + pixel_streams + sparse_streams + dense_streams (+ 1 with a communicator) */
    int32_t _pad;
    int64_t record_bytes;      /* a batch's record in HBM: [frame_offs: max_frames + 1 int32 | status: int32 | load: int32 = frames beyond the LDS tables
                                * (bits 0-19) + border points per frame / 16 (bits 20-31) | pad to 16 B | armours: armour_cap x 88 B] */
    int64_t armours_offset;    /* = the layout of rmcv_amd/dist.py, the payload of rmcv_gather */
    uint64_t submitted, collected;
    uint64_t dense_split;      /* batches whose dense frames were given a launch and a stream of their own (see dense_streams) */
    uint64_t hot_batches;      /* batches that ran in one of the hot contexts (see hot_contexts) */
    int32_t hot_contexts, _pad2;
    uint64_t latency_batches;  /* batches whose back half ran with the latency kernel (8 wavefronts per frame): the newest batch when a call waited
                                * for it -- wait / collect of it, drain -- before another submit (a burst's last batch; one batch at a time) */
    uint64_t host_blocking_calls; /* allocations, host-side synchronisations and blocking copies made inside rmcv_pipeline_submit since the
                                * pipeline was created: 0 (tests/test_gpu_pipeline.py asserts it over plain, dense and re-shaped streams) */
    int32_t wait_timeout_ms, _pad3; /* rmcv_pipeline_set_wait_timeout */
    double   max_submit_us;    /* host time of the longest single rmcv_pipeline_submit since creation / rmcv_pipeline_reset_stats, microseconds */
    uint64_t heavy_batches;    /* batches run in DENSE MODE: while the records that come back are heavy (more than an eighth of the frames beyond
                                * findContours' LDS tables, or >= 1 500 border points per frame; back below 1 200) the sparse stage runs its lean build
                                * (every frame on the mid tier, 61 KB of LDS instead of 80): dense streams 7-10 % faster */
    uint64_t held_back;        /* pixel launches held back behind a burst's first one (k_delay): only launches of the wave-specialised
                                * kernel on every CU, for a quarter of their expected time, 60 us at most, none below 100 us of launch */
} rmcv_pipeline_info;
/* GPU_MAX_HW_QUEUES=12 in the process environment unless the variable is set already; returns what it reads afterwards.  Effective
 * only BEFORE the process's first HIP call (the runtime reads the variable once); not thread-safe (setenv) -- call it first thing
 * in main.  12 = the default schedule's 2 + 4 + 4 streams + the null stream; more is harmful. */
int  rmcv_hw_queues_hint(void);
void rmcv_default_pipeline_config(rmcv_pipeline_config* c);
int  rmcv_pipeline_create(int device, const rmcv_limits* limits /* nullable */, const rmcv_pipeline_config* cfg /* nullable */, rmcv_pipeline** out);
void rmcv_pipeline_destroy(rmcv_pipeline* pl);   /* drains first */
const char* rmcv_pipeline_last_error(const rmcv_pipeline* pl);
int  rmcv_pipeline_get_info(const rmcv_pipeline* pl, rmcv_pipeline_info* out);
/* the context of ring slot `slot` (0 .. depth-1), for set-up that is per context -- rmcv_svm_load (RMCV_STAGE_IDENTITY),
 * rmcv_pnp_load (RMCV_STAGE_POSE), rmcv_ctx_set_option: do it for EVERY slot.  Owned by the pipeline. */
rmcv_ctx* rmcv_pipeline_context(rmcv_pipeline* pl, int slot);
/* the context a ticket's batch ran in, for the per-stage getters (binary image, contours, blobs, counts) on a ticket that has been
 * waited for.  The ticket's RECORD (rmcv_pipeline_collect / _record) lives until ticket + depth is submitted; its context's buffers
 * only until the context's next batch, which can be as early as ticket + hot_contexts (rmcv_pipeline_config): read them before
 * submitting that many more.  NULL for a ticket that is not live OR whose context a later batch has taken (rmcv_pipeline_last_error
 * says which). */
rmcv_ctx* rmcv_pipeline_context_of(rmcv_pipeline* pl, uint64_t ticket);
/* rmcv_pipeline_config::hot_contexts from the next submit on (3 .. depth - 1; 0 or -1: off).  Batches in flight are not touched. */
int  rmcv_pipeline_set_hot_contexts(rmcv_pipeline* pl, int n);
/* rmcv_pipeline_info::max_submit_us starts over (a diagnostic: bench.py reads it per timed region) */
int  rmcv_pipeline_reset_stats(rmcv_pipeline* pl);
/* the deadline of rmcv_pipeline_wait / _collect / _drain (and of the ring contexts' own waits), milliseconds; default 5000, 0: none.
 * A wait that runs out returns RMCV_ERR_TIMEOUT (the batch is still in flight; waiting again is allowed);
 * rmcv_pipeline_last_error names the enqueue made last. */
int  rmcv_pipeline_set_wait_timeout(rmcv_pipeline* pl, int ms);
/* enqueue one batch of n_frames frames that are resident in HBM (layout as rmcv_batch_set_device_frames); stages must include
 * RMCV_STAGE_BINARY.  Asynchronous; *ticket (0, 1, 2, ...) names the batch.  Without a hook, the batch's back half (sparse stage,
 * compaction) is enqueued by the NEXT call on the pipeline: another submit enqueues it as it always was; rmcv_pipeline_wait / _collect
 * of this very ticket, or _drain, know that nothing will run beside it and use the latency kernel (8 wavefronts per frame) -- the
 * last batch of a burst and a host that submits one batch at a time finish 0.03-0.08 ms earlier.  A submitted batch therefore
 * completes only once the pipeline is called again (any call that names it, the next submit, drain, destroy).  The slot's previous batch (ticket - depth) is
 * overwritten: collect it first. */
int  rmcv_pipeline_submit(rmcv_pipeline* pl, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch,
                          const rmcv_params* p, int stages, uint64_t* ticket);
/* the same with rm::FindLightBlobs as the blob stage (rmcv_batch_run_legacy) */
int  rmcv_pipeline_submit_legacy(rmcv_pipeline* pl, const void* d_frames, int n_frames, int w, int h, int stride, int64_t frame_pitch,
                                 const rmcv_params* p, const rmcv_legacy_params* lp, int stages, uint64_t* ticket);
/* a WINDOWED batch (see rmcv_batch_set_windows): d_origins = n_frames rmcv_point in DEVICE memory, borrowed like the frames and read on
 * the batch's stream in front of its pixel pass -- the host need never see them; nothing blocks (host_blocking_calls stays 0).  The
 * batch takes the k_binary shape and stays out of the hot-context rotation, as batches with RMCV_OPT_ENHANCE do; windowed and whole-frame
 * submits may alternate on one pipeline (each change of a context's geometry is enqueued work: planes zeroed, frame order recomputed).
 * The record is the usual one, armours in window coordinates; rmcv_pipeline_context_of(ticket) + rmcv_batch_get_windows give the
 * effective origins. */
int  rmcv_pipeline_submit_windows(rmcv_pipeline* pl, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride, int64_t frame_pitch,
                                  const void* d_origins, int win_w, int win_h, const rmcv_params* p, int stages, uint64_t* ticket);
/* a batch with PER-FRAME DETECTION KEYS (see rmcv_batch_set_frame_camps): rmcv_pipeline_submit (win_w == 0; d_origins ignored) or
 * rmcv_pipeline_submit_windows (win_w > 0) with d_camps = n_frames int32 and d_lower_bounds = n_frames int32 or NULL (the batch's
 * p->lower_bound) in DEVICE memory, borrowed like the frames and read on the batch's stream in front of its pixel pass; nothing blocks
 * (host_blocking_calls stays 0).  The batch takes the k_binary shape and stays out of the hot-context rotation, as windowed and enhanced
 * batches do; submits with and without keys may alternate on one pipeline.  Refused as rmcv_batch_set_frame_camps refuses. */
int  rmcv_pipeline_submit_camps(rmcv_pipeline* pl, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride, int64_t frame_pitch,
                                const void* d_camps, const void* d_lower_bounds /* nullable */, const void* d_origins /* nullable */, int win_w,
                                int win_h, const rmcv_params* p, int stages, uint64_t* ticket);
/* a TRACKED batch: frame f is the next frame of stream f of `trk` (device-resident tracker, above).  With the tracker's win_w > 0 this is
 * rmcv_pipeline_submit_windows whose origins are the tracker's requested origins; with win_w == 0 a whole-frame submit.  In both cases one
 * step of the tracker (`timestamp`: see rmcv_batch_track) is enqueued behind the batch's compaction on its finishing stream, and the NEXT
 * tracked submit on the same tracker waits on the GPU, by event, for that step in front of its k_window_origins: a strict closed loop --
 * batch k + 1 sees the origins of step k -- in which the host only submits.  (The pipeline enqueues a batch's back half on the next call:
 * that call enqueues back half, step and event before the next front half.)  rmcv_pipeline_wait / _collect / _drain of a tracked ticket
 * complete the step too.  Submits on different trackers, and untracked submits, are not ordered against it: two trackers interleave on one
 * pipeline and overlap as batches do.  Tracked batches stay out of the hot-context rotation.  Nothing blocks: host_blocking_calls stays 0.
 * RMCV_ERR_BAD_ARG, with a message and before anything is enqueued: n_frames != the tracker's n_streams, a frame size other than its
 * config's, stages without RMCV_STAGE_ARMOURS, a tracker on another device. */
int  rmcv_pipeline_submit_tracked(rmcv_pipeline* pl, rmcv_tracker* trk, const void* d_frames, int n_frames, int frame_w, int frame_h, int stride,
                                  int64_t frame_pitch, const rmcv_params* p, int stages, int64_t timestamp, uint64_t* ticket);
/* rmcv_pipeline_submit_tracked + this batch's serial packets: d_packets is n_frames x RMCV_SERIAL_PACKET_BYTES in DEVICE memory, borrowed
 * like the frames, or NULL.  On a tracker with attitude on (rmcv_tracker_set_attitude) the attitude step (above) is enqueued on the batch's
 * pixel stream, behind the event wait for the tracker's previous step and in front of k_frame_keys / k_window_origins;
 * rmcv_pipeline_submit_tracked on such a tracker is this call with d_packets == NULL.  Packet in, aim out, the host only submits.
 * RMCV_ERR_BAD_ARG, with a message and before anything is enqueued: what rmcv_pipeline_submit_tracked refuses; attitude off and d_packets
 * given. */
int  rmcv_pipeline_submit_tracked_serial(rmcv_pipeline* pl, rmcv_tracker* trk, const void* d_frames, int n_frames, int frame_w, int frame_h,
                                         int stride, int64_t frame_pitch, const void* d_packets, const rmcv_params* p, int stages,
                                         int64_t timestamp, uint64_t* ticket);
/* the frames' camera indices for every following submit, of any of the six calls, whose stages include RMCV_STAGE_POSE: a
 * stream's camera does not change from batch to batch.  d_idx: n_frames int32 in DEVICE memory, borrowed until replaced and until the
 * batches submitted with it are through; read on the batch's stream in front of k_pnp; any value (rmcv_frame_camera).  NULL: off.  The
 * cameras themselves are loaded into EVERY slot (rmcv_pipeline_context(k), rmcv_pnp_load_cameras).  Such a submit is refused with
 * RMCV_ERR_BAD_ARG and a message, before anything is enqueued: its n_frames differs from the table's; the ring's contexts do not all hold
 * the same n_cameras.  Nothing blocks: host_blocking_calls stays 0. */
int  rmcv_pipeline_set_frame_cameras(rmcv_pipeline* pl, const void* d_idx, int n_frames);
/* the frames' model indices for every following submit, of any of the six calls, whose stages include RMCV_STAGE_IDENTITY.
 * d_idx: n_frames int32 in DEVICE memory, borrowed until replaced and until the batches submitted with it are through; read on the batch's
 * stream in front of the classifier; any value (rmcv_frame_model).  NULL: off.  The models themselves are loaded into EVERY slot
 * (rmcv_pipeline_context(k), rmcv_svm_load_models).  Such a submit is refused with RMCV_ERR_BAD_ARG and a message, before anything is
 * enqueued: its n_frames differs from the table's; the ring's contexts do not all hold the same n_models.  Nothing blocks:
 * host_blocking_calls stays 0.  The device camps table of rmcv_pipeline_submit_camps may be the same buffer (see rmcv_svm_load_models). */
int  rmcv_pipeline_set_frame_models(rmcv_pipeline* pl, const void* d_idx, int n_frames);
/* block until the batch is through (its record complete in HBM and, with host_results, on the host) */
int  rmcv_pipeline_wait(rmcv_pipeline* pl, uint64_t ticket);
/* wait + hand the batch's armours over, frame-major, in submission order of the frames: frame_offs (nullable) has n_frames + 1
 * entries.  RMCV_ERR_CAPACITY: a frame exceeded a context limit, or the list exceeds armour_cap / cap (*n_total says what is
 * needed); RMCV_ERR_BAD_ARG: the ticket was never issued or its slot has been reused. */
int  rmcv_pipeline_collect(rmcv_pipeline* pl, uint64_t ticket, rmcv_armour* armours_out, int cap, int32_t* frame_offs, int32_t* n_total);
/* everything submitted so far is through */
int  rmcv_pipeline_drain(rmcv_pipeline* pl);
/* device view of a ticket's record and the stream it is produced on (work enqueued there runs behind the compaction) */
int  rmcv_pipeline_record(rmcv_pipeline* pl, uint64_t ticket, void** d_record, void** hip_stream);
/* Hook called by rmcv_pipeline_submit, on the submitting thread, right behind the enqueue of a batch's compaction: for a consumer
 * that lives on the device (a collective, a tracker kernel).  What the hook enqueues on `hip_stream` is ordered behind the record;
 * the record's next rewrite (ticket + depth) is ordered behind what the hook enqueued there.  A hook that moves the record on
 * ANOTHER stream returns an event through *done_event (a hipEvent_t it owns, recorded when the record has been read): the rewrite
 * then waits for it.  A non-zero return fails the submit. */
typedef int (*rmcv_pipeline_hook)(void* user, uint64_t ticket, void* d_record, int64_t record_bytes, void* hip_stream, void** done_event);
int  rmcv_pipeline_set_hook(rmcv_pipeline* pl, rmcv_pipeline_hook fn, void* user);
/* built-in hook for BASELINE config 4: every batch's record is gathered to `root` with rmcv_gather on `comm` (every rank submits the
 * same number of batches).  On the root, *d_recv of rmcv_pipeline_gathered is n_ranks x record_bytes in rank order, valid once the
 * ticket has been waited for, until ticket + depth is submitted. */
int  rmcv_pipeline_set_gather(rmcv_pipeline* pl, rmcv_comm* comm, int root);
int  rmcv_pipeline_gathered(rmcv_pipeline* pl, uint64_t ticket, void** d_recv, int64_t* bytes);

/* ---- the operator's view: the debug image of the reference's loop, rendered on the device -------------------------
 * executable/main.cpp:200-207 builds a debug image from `binary` -- cvtColor(GRAY2BGR), rm::debug::draw_lightblobs(positive, negative),
 * rm::debug::draw_armours(armours) (src/debug.cpp:43-93) -- and its debug thread (:90-100) shows it resized to 1024 x 768.  For a frame f of
 * a batch whose run included RMCV_STAGE_ARMOURS and a view size (vw, vh):
 *     V(f) = resize( draw_armours( draw_lightblobs( GRAY2BGR(binary_f) ) ), (vw, vh), INTER_LINEAR ),   8UC3, BGR
 * every byte equal to the CPU restatement rmcv_debug_view_host of those calls (OpenCV 4.8.0 as recalled: SURVEY.md A.10), with one stated
 * deviation: cv::putText (debug.cpp:53-57) is not rendered BY THESE ENTRY POINTS -- the label pass over the finished view draws it (see "view
 * labels" below: rmcv_batch_view_labels, rmcv_pipeline_set_view_labels); its data (identity, position, vertices[0]) also comes from the getters.
 * A segment with an endpoint that is not finite or of magnitude >= 2^30 is skipped.  In a windowed batch the view is the window's.  The view
 * is written from the frame's bit plane and its result tables: it is the same with and without RMCV_STAGE_NO_IMAGE.
 * Colours (BGR): a positive blob (0, 255, 0) if its target is RMCV_CAMP_RED, (0, 0, 255) otherwise; negatives, armours' vertices and icons
 * (0, 255, 255); later draws overwrite earlier ones. */
#define RMCV_VIEW_BLOBS 1     /* the positive light blobs                         */
#define RMCV_VIEW_NEGATIVES 2 /* the negative contours                            */
#define RMCV_VIEW_ARMOURS 4   /* every armour's vertices and icon quadrilaterals  */
#define RMCV_VIEW_ALL 7       /* the reference                                    */
/* the views of n frames of the batch bound, frames[k] -> d_out + k * out_pitch (DEVICE memory of the caller's, rows out_stride >= 3 vw bytes
 * apart, views out_pitch >= out_stride (vh - 1) + 3 vw apart).  Asynchronous: enqueued on hip_stream (NULL: the context's) behind the run;
 * renders what the tables hold and reports no frame status.  RMCV_ERR_BAD_ARG, with a message, before anything is enqueued: n < 1 or beyond
 * the batch; a frame index out of range or repeated; vw / vh < 1 or beyond the context's max_width / max_height; a stride or pitch too small;
 * unknown flags; a batch whose last run lacked the stages the flags need (RMCV_STAGE_BINARY; _CONTOURS and _BLOBS for blobs and negatives;
 * _ARMOURS for armours). */
int rmcv_batch_debug_views(rmcv_ctx* ctx, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch,
                           void* hip_stream);
/* one frame's view to HOST memory; waits with the context's deadline.  Also RMCV_ERR_BAD_ARG: the frame carries an RMCV_FRAME_OVF_* status
 * (its tables are not the frame's lists). */
int rmcv_batch_get_debug_view(rmcv_ctx* ctx, int frame, int vw, int vh, int flags, uint8_t* out, int out_stride);
/* stage-wise: host lists through the same two kernels, buffers of its own (nothing bound to the context moves).  binary: h rows of
 * `stride >= w` bytes, 0 / 255 (any other non-zero byte counts as 255); neg_pts / neg_offs: the negative contours as CSR, n_neg + 1
 * offsets; w, h, vw, vh within the context's max_width / max_height. */
int rmcv_debug_view(rmcv_ctx* ctx, const uint8_t* binary, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs,
                    const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags,
                    int vw, int vh, uint8_t* out, int out_stride);
/* the same arguments, host-side (no context, no device, any size): the sequential restatement -- a BGR canvas drawn in the reference's
 * call order, every blob in its own colour, then resized */
int rmcv_debug_view_host(const uint8_t* binary, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
                         const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh,
                         uint8_t* out, int out_stride);
/* a pipeline's views: from the next submit on, every batch's frames[0 .. n) are rendered behind its sparse stage into the slot's own view
 * buffer (allocated HERE, one per ring slot: this call blocks, no submit does).  n == 0: off -- a submit then enqueues exactly what it did
 * before.  RMCV_ERR_BAD_ARG as rmcv_batch_debug_views; a later submit whose n_frames does not reach every index, or whose stages lack what
 * the flags need, is refused before anything is enqueued. */
int rmcv_pipeline_set_views(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int flags);
/* the views of a ticket's batch: n views of vh rows, *stride bytes between rows, *pitch between views, in device memory; complete once the
 * ticket has been waited for, valid as long as the ticket's record (until ticket + depth is submitted).  RMCV_ERR_BAD_ARG: the ticket was
 * never issued, its slot has been reused, or it was submitted without views. */
int rmcv_pipeline_views(rmcv_pipeline* pl, uint64_t ticket, void** d_views, int32_t* stride, int64_t* pitch, int32_t* n);

/* ---- the source view: the camera frame with the loop's overlays, rendered on the device ------------------------------
 * The operator's view shows what the detector kept; executable/svm/labeler.cpp:108-111 copies the CAMERA FRAME and draws the armours and
 * light blobs on it -- the picture a person labelling icons, checking an exposure or judging a threshold looks at.  For a frame f of a
 * batch, flags in 0 .. RMCV_VIEW_ALL and a view size (vw, vh):
 *     S(f) = resize( draw_armours( draw_lightblobs( SRC(f) ) ), (vw, vh), INTER_LINEAR ),   8UC3, BGR
 * everything as for V(f) above -- the order of the draws, colours, clipping, the skipped segments, the three resize modes, no text -- but
 * the canvas: SRC(f), the BGR image the frame's results are defined on:
 *     BGR frames                                          the frame
 *     a Bayer RMCV_OPT_INPUT_FORMAT, in any layout        D(T(r)): rmcv_demosaic / rmcv_demosaic_raw of the frame, D's border clamp included
 *     RMCV_OPT_ENHANCE                                    E(f): every frame byte through the frame's own table, the one the run built
 *                                                         (overlay colours are drawn afterwards and do not go through it)
 *     windows                                             the crop at the frame's effective origin, win_w x win_h, in window coordinates
 * A set overlay pixel replaces the source pixel.  Flags 0 is the plain resized frame, a thumbnail.  Every byte equals the CPU restatement
 * rmcv_source_view_host of SRC(f) and the frame's lists.  The view is the same with and without RMCV_STAGE_NO_IMAGE.  There is no flag bit
 * for it: the entry points above keep refusing flags > RMCV_VIEW_ALL. */
/* rmcv_batch_debug_views' arguments, RMCV_ERR_BAD_ARG list and stage rule.  Asynchronous: enqueued on hip_stream (NULL: the context's)
 * behind the run.  The kernels read the frames: BORROWED device frames (rmcv_batch_set_device_frames) must stay valid, and unchanged, until
 * the views have finished on that stream. */
int rmcv_batch_source_views(rmcv_ctx* ctx, const int32_t* frames, int n, int vw, int vh, int flags, void* d_out, int out_stride, int64_t out_pitch,
                            void* hip_stream);
/* one frame's source view to HOST memory; waits with the context's deadline.  Also RMCV_ERR_BAD_ARG: the frame carries an RMCV_FRAME_OVF_*
 * status (its tables are not the frame's lists). */
int rmcv_batch_get_source_view(rmcv_ctx* ctx, int frame, int vw, int vh, int flags, uint8_t* out, int out_stride);
/* stage-wise: a host BGR image (h rows of `stride >= 3 w` bytes) and host lists (as rmcv_debug_view's) through the same kernels, buffers of
 * its own (nothing bound to the context moves); w, h, vw, vh within the context's max_width / max_height. */
int rmcv_source_view(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs,
                     const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags,
                     int vw, int vh, uint8_t* out, int out_stride);
/* the same arguments, host-side (no context, no device, any size): the sequential restatement -- the image copied to a BGR canvas, drawn in
 * the reference's call order, then resized */
int rmcv_source_view_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_lightblob* blobs, int n_blobs, const rmcv_point* neg_pts,
                          const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours, int flags, int vw, int vh,
                          uint8_t* out, int out_stride);
/* a pipeline's source views: rmcv_pipeline_set_views' semantics (allocates HERE, no submit blocks, n == 0: off).  A pipeline renders ONE kind
 * of view at a time: the later of the two setters wins, and rmcv_pipeline_views returns whichever kind was rendered for the ticket. */
int rmcv_pipeline_set_source_views(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int flags);

/* ---- view labels: armour labels and tracker targets over finished views, rendered on the device ------------------------
 * rm::debug::draw_armours writes a text line at every armour's vertices[0] (src/debug.cpp:53-57):
 *     to_string(identity) + ": " + to_string(x) + ", " + to_string(y) + ", " + to_string(z)
 * The label pass draws it over views either kind above has FINISHED (BGR, vw x vh, device memory), and for a tracked run every target the
 * tracker holds: its quadrilateral and the same line followed by ", " + to_string(lost_count).  Every byte equals the CPU restatement
 * rmcv_view_labels_host.  Stated deviations from the reference:
 *   - the text is drawn IN VIEW SPACE, behind the resize, with an integer scale 1 .. 8 -- the reference writes it on the full frame, then the
 *     contours, then resizes; a label must stay legible in a thumbnail;
 *   - the font is this library's own 5 x 7 bitmap glyphs (rmcv_view_glyph), not FONT_HERSHEY_SIMPLEX;
 *   - to_string(double) is "%f" for finite |v| < 1e15 -- six decimals, round-half-even on the exact binary value, the sign bit printed also
 *     for -0.0 and for negatives that round to zero --; a NaN prints "nan" whatever its sign (glibc: "-nan"); a finite |v| >= 1e15 prints
 *     "big" / "-big" (the reference: up to 309 digits); +-inf print "inf" / "-inf";
 *   - the tracker's targets are not drawn by the reference at all.
 * The line.  An armour's: identity from the run's RMCV_STAGE_IDENTITY, else -1; position from its RMCV_STAGE_POSE, else (0, 0, 0) -- the
 * tracker's observations' defaults.  A track's: rmcv_track::identity; state_post[0 .. 2] if `initialized`, else `position` (the aim step's
 * source rule); rmcv_track::lost_count.
 * Placement.  (w, h) is the geometry the frame's tables are in (a windowed batch: the window's).  An anchor vertex is rounded as
 * cv::Point(Point2f) does (cvRound, half to even) to (px, py); view anchor ax = floor(px vw / w), ay = floor(py vh / h) (a true floor).  With
 * scale s, a set bit of character k at glyph column c (0 .. 4, left to right) and row r (0 .. 6, top to bottom) fills the s x s block at
 * x = ax + (6 k + c) s, y = ay - (7 - r) s: the text's bottom-left sits at the anchor, as putText's origin does.  Every pixel is clipped to the
 * view; only set bits write (no background box).  A vertex that is not finite or of magnitude >= 2^30 is not drawable: a line whose anchor
 * is not is skipped, and so is a quadrilateral with such a vertex.
 * A track's quadrilateral: the side record's four vertices (frame coordinates), each rounded, moved by the frame's effective window origin
 * ((0, 0) without windows) and mapped by the two floors, joined j -> j + 1 (closed) through the views' line iterator and clip with the view
 * as the canvas; its line's anchor is the mapped vertex 0.
 * Colours (BGR): armours' lines (0, 255, 255), the reference's; tracks' quadrilaterals and lines (255, 0, 255).  Everything of the tracks is
 * drawn first, then the armours' lines. */
#define RMCV_LABEL_MAX_CHARS 112 /* >= the longest line: 11 + 2 + 3 x 23 + 2 x 2 + 2 + 11 = 99 characters */
#define RMCV_LABEL_ARMOURS 1
#define RMCV_LABEL_TRACKS 2
/* host-side (no context, no device).  The three text functions write a terminated string into out[0 .. cap) and return its length;
 * RMCV_ERR_CAPACITY when cap cannot hold it and the terminator (out is terminated within cap, its contents otherwise unspecified);
 * RMCV_ERR_BAD_ARG for a null pointer or cap < 1.  rmcv_format_f6 is to_string(double) as stated above. */
int rmcv_format_f6(double v, char* out, int cap);
int rmcv_label_text(int32_t identity, const double position[3], char* out, int cap); /* position NULL: (0, 0, 0) */
int rmcv_track_label_text(const rmcv_track* t, char* out, int cap);
/* a glyph: 7 row bytes, top to bottom, 5 bits each, the LEFT column in bit 4.  The set is 0-9 - . : , space n a i f b g (21 glyphs; space
 * is empty); RMCV_ERR_BAD_ARG for any other character. */
int rmcv_view_glyph(int ch, uint8_t rows[7]);
/* the sequential restatement, drawing in place: view is vh rows of `stride >= 3 vw` bytes; armours in the geometry's coordinates with
 * identities (NULL: -1) and positions (n_armours x 3 doubles; NULL: zeros); tracks (NULL: none) with last_vertices [n_tracks][4][2] in
 * frame coordinates (rmcv_tracker_get's) and the effective window origin (x_eff, y_eff) they are moved by.  RMCV_ERR_BAD_ARG: a null
 * view or list, sizes < 1, a stride too small, scale outside 1 .. 8. */
int rmcv_view_labels_host(uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours, const int32_t* identities,
                          const double* positions, int n_armours, const rmcv_track* tracks, const float* last_vertices, int n_tracks, int x_eff, int y_eff);
/* stage-wise: the same arguments through the kernel, on a HOST view returned in place, buffers of its own (nothing bound to the context
 * moves); vw, vh within the context's max_width / max_height. */
int rmcv_view_labels(rmcv_ctx* ctx, uint8_t* view, int vw, int vh, int stride, int w, int h, int scale, const rmcv_armour* armours,
                     const int32_t* identities, const double* positions, int n_armours, const rmcv_track* tracks, const float* last_vertices,
                     int n_tracks, int x_eff, int y_eff);
/* the armours' lines of frames[k] of the batch bound over view k at d_views + k * pitch (DEVICE memory, rows `stride` bytes apart): the views
 * rmcv_batch_debug_views / rmcv_batch_source_views wrote for the same frames and size.  Asynchronous: enqueued on hip_stream (NULL: the
 * context's) behind the run; nothing is allocated (but, once in a context's life, the views' frame list where no view call has run yet).
 * RMCV_ERR_BAD_ARG, with a message, before anything is enqueued: everything rmcv_batch_debug_views refuses about frames, n, sizes, stride and
 * pitch; scale outside 1 .. 8; a last run without RMCV_STAGE_ARMOURS. */
int rmcv_batch_view_labels(rmcv_ctx* ctx, const int32_t* frames, int n, int vw, int vh, int scale, void* d_views, int stride, int64_t pitch,
                           void* hip_stream);
/* the tracks of stream frames[k] (frame f of the batch is stream f) over view k: behind the run and behind the tracker's step in flight,
 * whichever stream that ran on; the tracker's next step waits for it.  Also RMCV_ERR_BAD_ARG: everything rmcv_batch_track refuses about
 * the tracker and the batch. */
int rmcv_batch_view_tracks(rmcv_ctx* ctx, rmcv_tracker* trk, const int32_t* frames, int n, int vw, int vh, int scale, void* d_views, int stride,
                           int64_t pitch, void* hip_stream);
/* a pipeline's labels: from the next submit on, `what` (RMCV_LABEL_* bits) is drawn at `scale` over the views of every batch, whichever kind
 * the pipeline renders (rmcv_pipeline_set_views / _set_source_views), in front of the batch's completion; RMCV_LABEL_TRACKS behind the
 * tracker step of the same submit.  what == 0: off -- a submit then enqueues exactly what it did before.  No submit blocks
 * (host_blocking_calls stays 0).  RMCV_ERR_BAD_ARG: unknown bits, scale outside 1 .. 8, no views set (turning the views off turns the labels
 * off).  A later submit without a tracker while RMCV_LABEL_TRACKS is set, or whose stages lack RMCV_STAGE_ARMOURS, is refused before
 * anything is enqueued. */
int rmcv_pipeline_set_view_labels(rmcv_pipeline* pl, int what, int scale);
/* launches of the label kernel (k_view_text) by this process so far: a submit with the labels off adds none */
int64_t rmcv_view_text_launches(void);

/* ---- the labeler's screen: icons at any size and the combined sheet, rendered on the device ------------------------------
 * executable/svm/labeler.cpp:93-106 rectifies every armour's icon with rm::affine_correction(frame, tmp, armour.icon, {80, 80}) and lays the
 * icons side by side; :113-119 puts the frame with its overlays, the binary image and that strip into one canvas.
 * The icon.  rm::affine_correction (src/imgproc.cpp:9-35) at an output size (ow, oh), 1 .. RMCV_ICON_SIDE_MAX each: the vertices clamped in
 * place to the image, their integer bounding box, getAffineTransform of ([1], [2], [0]) onto the box's corners, warpAffine INTER_LINEAR /
 * BORDER_CONSTANT 0 of the box, resize INTER_LINEAR to (ow, oh) -- the exact 2:1 case as the 2 x 2 box average -- all in OpenCV's fixed
 * point.  At 20 x 20 it is the row rmcv_batch_get_icons hands out.  A degenerate box gives zeros.
 * The strip.  For a frame f, a side and a cap: `side` rows of cap * side pixels (8UC3, BGR); the icon of armour j < min(n_armours, cap) at
 * side x side in columns [j side, (j + 1) side); every other byte zero (the labeler's Mat::zeros; the uninitialised tail of its strip is not
 * mirrored).  The icon is computed on SRC(f), the image the frame's results are defined on (the source view's: the frame, its demosaic, the
 * frame through its gamma table, its window).  The armour table is only read: the strip is the same with and without RMCV_STAGE_IDENTITY
 * (the clamp that stage writes back is idempotent).  Every byte equals rmcv_icon_strip_host of SRC(f) and the frame's armours.
 * The sheet.  labeler.cpp:113-119 at view size, one canvas of 2 vw x (vh + side) pixels: S(f) with `flags` in [0, vw) x [0, vh); the plain
 * binary as BGR -- V(f) with flags 0 -- in [vw, 2 vw) x [0, vh); the strip with cap = min(floor(2 vw / side), max_armours) in rows
 * [vh, vh + side), the rest of those rows zero.  Stated deviations: the strip is square; the views keep their draw order (blobs, then armours;
 * the labeler draws the armours first); no text under the icons; no window, no keyboard. */
#define RMCV_ICON_SIDE_MAX 256
#define RMCV_ICON_STRIP_CAP_MAX 1024 /* slots of a host strip (a context's: its max_armours) */
/* host-side (no context, no device): rm::affine_correction(bgr, out, icon, {ow, oh}) on an image of h rows of `stride >= 3 w` bytes.  icon is
 * clamped in place (imgproc.cpp:11-15); *degenerate (nullable) is set to 1 when the box is, and `out` (oh rows of out_stride >= 3 ow bytes)
 * is then zero-filled.  RMCV_ERR_BAD_ARG: a null buffer; w or h < 1; stride < 3 w; ow or oh outside 1 .. 256; out_stride < 3 ow. */
int rmcv_affine_correction_host(const uint8_t* bgr, int w, int h, int stride, float icon[4][2], int ow, int oh, uint8_t* out, int out_stride,
                                int32_t* degenerate);
/* stage-wise: a host image and host armours through the kernel, buffers of its own (nothing bound to the context moves); w, h within the
 * context's max_width / max_height, n and cap within its max_armours.  out: `side` rows of out_stride >= 3 cap side bytes, of which
 * 3 cap side are written. */
int rmcv_icon_strip(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, const rmcv_armour* armours, int n, int side, int cap, uint8_t* out,
                    int out_stride);
/* the same on the CPU (icon_host.h); no context; cap 1 .. RMCV_ICON_STRIP_CAP_MAX */
int rmcv_icon_strip_host(const uint8_t* bgr, int w, int h, int stride, const rmcv_armour* armours, int n, int side, int cap, uint8_t* out,
                         int out_stride);
/* chosen frames of the batch run last: strip k (of frame frames[k]) at d_out + k * out_pitch (DEVICE memory), `side` rows of out_stride >=
 * 3 cap side bytes; d_counts (device, may be NULL): int32 per strip, the icons rendered, min(n_armours, cap).  Asynchronous: enqueued on
 * hip_stream (NULL: the context's) behind the run; the kernel reads the frames, as the source view's do.  RMCV_ERR_BAD_ARG, with a message,
 * before anything is enqueued: everything rmcv_batch_source_views refuses about frames and n; side outside 1 .. 256; cap outside
 * 1 .. max_armours; out_stride < 3 cap side; out_pitch < out_stride (side - 1) + 3 cap side for n > 1; a null output; nothing bound; a last
 * run without RMCV_STAGE_ARMOURS.  The call renders what the tables hold. */
int rmcv_batch_icon_strips(rmcv_ctx* ctx, const int32_t* frames, int n, int side, int cap, void* d_out, int out_stride, int64_t out_pitch,
                           int32_t* d_counts, void* hip_stream);
/* one frame's strip to HOST memory, *n_icons (nullable) the icons rendered; waits with the context's deadline.  Also RMCV_ERR_BAD_ARG: the
 * frame carries an RMCV_FRAME_OVF_* status. */
int rmcv_batch_get_icon_strip(rmcv_ctx* ctx, int frame, int side, int cap, uint8_t* out, int out_stride, int32_t* n_icons);
/* host-side: the sheet's extent, 2 vw x (vh + side).  RMCV_ERR_BAD_ARG: vw or vh < 1, side outside 1 .. 256 or > 2 vw, null outputs. */
int rmcv_sheet_size(int vw, int vh, int side, int32_t* sheet_w, int32_t* sheet_h);
/* sheet k (of frame frames[k]) at d_out + k * out_pitch (DEVICE memory), vh + side rows of out_stride >= 6 vw bytes.  The two panes are the
 * view launches aimed at sub-rectangles of the sheet: no copy pass.  Asynchronous, behind the run.  RMCV_ERR_BAD_ARG, before anything is
 * enqueued: what rmcv_batch_source_views and rmcv_batch_debug_views refuse; a last run without RMCV_STAGE_BINARY, what the flags need, or
 * RMCV_STAGE_ARMOURS; side outside 1 .. 256 or > 2 vw; out_stride < 6 vw; out_pitch < out_stride (vh + side - 1) + 6 vw for n > 1. */
int rmcv_batch_labeler_sheets(rmcv_ctx* ctx, const int32_t* frames, int n, int vw, int vh, int side, int flags, void* d_out, int out_stride,
                              int64_t out_pitch, void* hip_stream);
/* one frame's sheet to HOST memory; also RMCV_ERR_BAD_ARG: the frame carries an RMCV_FRAME_OVF_* status */
int rmcv_batch_get_labeler_sheet(rmcv_ctx* ctx, int frame, int vw, int vh, int side, int flags, uint8_t* out, int out_stride);
/* the same on the CPU: rmcv_source_view_host's image and lists plus the binary image (h rows of binary_stride >= w bytes); the strip holds
 * min(floor(2 vw / side), RMCV_ICON_STRIP_CAP_MAX) slots */
int rmcv_labeler_sheet_host(const uint8_t* bgr, int w, int h, int stride, const uint8_t* binary, int binary_stride, const rmcv_lightblob* blobs,
                            int n_blobs, const rmcv_point* neg_pts, const int32_t* neg_offs, int n_neg, const rmcv_armour* armours, int n_armours,
                            int vw, int vh, int side, int flags, uint8_t* out, int out_stride);
/* a pipeline's sheets: rmcv_pipeline_set_source_views' semantics (allocates HERE, no submit blocks, n == 0: off).  A third kind of view: the
 * latest of the three setters wins, rmcv_pipeline_views then returns sheets (n of vh + side rows, stride 6 vw), and with
 * rmcv_pipeline_set_view_labels on the label pass draws over the left pane.  With sheets off a submit enqueues exactly what it did before. */
int rmcv_pipeline_set_sheets(rmcv_pipeline* pl, const int32_t* frames, int n, int vw, int vh, int side, int flags);

/* ---- the session recorder: rm::debug::logger (include/debug.h:13-29, src/debug.cpp:9-41) for frames resident in HBM ----
 * The reference records every frame the detector saw, losslessly (FFV1), with a `data` record per frame.  Here chosen frames of every batch
 * are packed losslessly ON THE DEVICE into a ring of the last `slots` batches, together with what is needed to run the batch again; the
 * ring is downloaded, saved, loaded and replayed bit for bit.  deviation: the packed format is this library's (below), not FFV1 / AVI.
 *
 * The packed form of a plane of h rows of w_bytes bytes with a byte lag of 1 .. 4 (the distance to the previous sample of the same kind:
 * 3 for BGR, 2 for an 8-bit Bayer mosaic, 4 for Bayer in 2-byte samples, 1 otherwise), S = ceil(w_bytes / 256) segments of 256 bytes a row
 * (the last one extended with virtual bytes of raw value 0 and residual 0 that are never read):
 *   per segment: b_raw = the bit length of its greatest byte; b_pred = the bit length of its greatest z, where for byte i of the row
 *   r = (v[i] - (i >= lag ? v[i - lag] : 0)) mod 256 and z = ((s << 1) ^ (s >> 7)) & 0xFF with s = r as int8; raw mode with b = b_raw if
 *   b_raw <= b_pred, predicted mode with b = b_pred otherwise; header byte b | mode_predicted << 4; payload 32 b bytes: for j < b
 *   (outermost), k < 4: one little-endian u64 whose bit L is bit j of the coded value (v or z) of the segment's byte 4 L + k
 *   a frame: h S header bytes (row-major), zeros to a multiple of 8 | h + 1 u32 offsets of the rows' first segments from the start of the
 *   payload area (entry h: its size), zeros to a multiple of 8 | the payloads in segment order
 * rmcv_pack_bound: the size with b = 8 everywhere.  An all-zero plane packs to the header and the table alone. */
int64_t rmcv_pack_bound(int w_bytes, int h);
/* host-side (no device).  pack: *size = the packed size; RMCV_ERR_CAPACITY when cap is smaller (*size then says what is needed, or the
 * bound where that is not known yet).  unpack: RMCV_ERR_BAD_ARG for a buffer whose header, row table or size do not agree with w_bytes, h
 * and len -- it never reads outside packed[0 .. len) -- and bytes beyond w_bytes of a destination row are left alone. */
int rmcv_pack_host(const uint8_t* src, int w_bytes, int h, int64_t stride, int lag, uint8_t* out, int64_t cap, int64_t* size);
int rmcv_unpack_host(const uint8_t* packed, int64_t len, int w_bytes, int h, int lag, uint8_t* dst, int64_t stride);
/* device-side, asynchronous on hip_stream, nothing allocated: n frames (rows `stride` >= w_bytes apart, frames `pitch` apart) -> n packed
 * frames out_pitch >= rmcv_pack_bound apart (d_out and out_pitch multiples of 8), their sizes in d_sizes[n] (int64, device).  n <= 65535. */
int rmcv_pack_frames(int device, const void* d_frames, int n, int w_bytes, int h, int stride, int64_t pitch, int lag, void* d_out,
                     int64_t out_pitch, int64_t* d_sizes, void* hip_stream);
/* the inverse: packed frames in_pitch apart -> frames.  A packed frame that points outside its in_pitch bytes is left unfinished. */
int rmcv_unpack_frames(int device, const void* d_packed, int n, int w_bytes, int h, int64_t in_pitch, int lag, void* d_frames, int stride,
                       int64_t pitch, void* hip_stream);

#define RMCV_RECORDER_MAX_FRAMES 64
typedef struct rmcv_recorder rmcv_recorder;
typedef struct rmcv_session rmcv_session;
typedef struct rmcv_recorder_config {
    int32_t slots;       /* batches the ring holds                                (default 8)          */
    int32_t max_frames;  /* chosen frames of a batch, <= RMCV_RECORDER_MAX_FRAMES (default 8)          */
    int32_t max_w_bytes; /* bytes of a row                                        (default 3 * 1280)   */
    int32_t max_h;       /*                                                       (default 1024)       */
    int32_t user_bytes;  /* capacity of the user blob                             (default 256)        */
    int32_t track_cap;   /* tracks a loop record keeps per chosen frame, 1 .. RMCV_TRACKER_MAX_CAP; 0: no loop records (default 0) */
} rmcv_recorder_config;
/* what the host knows of a recorded batch at its submit, plus what the device reported of it */
typedef struct rmcv_record_entry {
    uint64_t ticket;       /* the pipeline's ticket; a stand-alone record: == sequence */
    uint64_t sequence;     /* batches recorded before this one; the slot is sequence mod slots */
    int64_t timestamp;     /* a tracked submit's */
    int32_t n_frames;      /* frames recorded */
    int32_t batch_frames;  /* frames of the batch they were chosen from */
    int32_t w, h;          /* pixels of a frame (a stand-alone record: w = w_bytes) */
    int32_t w_bytes, stride; /* bytes of a row as recorded; bytes between the rows of the frames as submitted */
    int32_t lag, input_format, sample_bits, valid_bit, orient, stages;
    int32_t win_w, win_h;  /* a windowed batch's window (0: whole frames) */
    int32_t has_keys;      /* keys[] holds the batch's effective per-frame detection keys (rmcv_batch_get_frame_keys), camps[] the raw camps */
    int32_t has_origins;   /* origins[] holds the batch's effective window origins (rmcv_batch_get_windows) */
    int32_t user_bytes;
    int32_t loop_bytes;    /* bytes of ONE loop record of this entry (rmcv_loop_bound of the recorder's track_cap); 0: the batch has none */
    rmcv_params params;
    int32_t frames[RMCV_RECORDER_MAX_FRAMES];   /* indices into the batch */
    int64_t sizes[RMCV_RECORDER_MAX_FRAMES];    /* packed sizes */
    int32_t keys[RMCV_RECORDER_MAX_FRAMES][4];
    int32_t camps[RMCV_RECORDER_MAX_FRAMES];    /* with has_keys: the frames' raw camps (what blobs' targets and the pairing compare against) */
    rmcv_point origins[RMCV_RECORDER_MAX_FRAMES];
} rmcv_record_entry;
void rmcv_default_recorder_config(rmcv_recorder_config* c);
/* allocates the ring (slots x max_frames areas of rmcv_pack_bound(max_w_bytes, max_h) bytes, and the small tables); 0 in a field = default */
int rmcv_recorder_create(int device, const rmcv_recorder_config* cfg, rmcv_recorder** out);
void rmcv_recorder_destroy(rmcv_recorder* rec);
const char* rmcv_recorder_last_error(const rmcv_recorder* rec);
/* the user blob of the NEXT batch recorded (and every one after it, until set again): the `data` of logger::write */
int rmcv_recorder_set_user(rmcv_recorder* rec, const void* data, int bytes);
/* stand-alone: pack frames[0 .. n) (indices; NULL: 0 .. n - 1) of device frames into the next slot, asynchronously on hip_stream; the
 * frames must stay as they are until the stream has passed.  Frozen: RMCV_OK, nothing recorded. */
int rmcv_recorder_record(rmcv_recorder* rec, const void* d_frames, int w_bytes, int h, int stride, int64_t pitch, int lag, const int32_t* frames,
                         int n, void* hip_stream);
/* while frozen nothing is recorded and nothing is overwritten */
int rmcv_recorder_freeze(rmcv_recorder* rec);
int rmcv_recorder_resume(rmcv_recorder* rec);
/* readers: each waits for the packing of what it reads, with a 5 s deadline (RMCV_ERR_TIMEOUT).  i = 0 is the oldest batch held.
 * user_out (nullable): the first min(user_cap, entry->user_bytes) bytes of the blob.  frame: the packed bytes only (*size of them). */
int rmcv_recorder_count(rmcv_recorder* rec, int32_t* n);
int rmcv_recorder_entry(rmcv_recorder* rec, int i, rmcv_record_entry* entry, void* user_out, int user_cap);
int rmcv_recorder_frame(rmcv_recorder* rec, int i, int k, void* out, int64_t cap, int64_t* size);
int rmcv_recorder_device_frame(rmcv_recorder* rec, int i, int k, void** d_packed, int64_t* size);
/* the ring as a session file (little-endian, magic, version), oldest batch first; an existing file is replaced */
int rmcv_recorder_save(rmcv_recorder* rec, const char* path);
/* one host-packed batch behind what a session file holds (created when missing): what rm::debug::logger::write does.  No device. */
int rmcv_session_append(const char* path, const rmcv_record_entry* entry, const void* user, const uint8_t* const* packed);
/* a session file, host-side (no device): every length is checked against the file's size; RMCV_ERR_BAD_ARG for a truncated or
 * inconsistent file */
int rmcv_session_open(const char* path, rmcv_session** out);
int rmcv_session_count(const rmcv_session* s, int32_t* n);
int rmcv_session_entry(const rmcv_session* s, int i, rmcv_record_entry* entry, void* user_out, int user_cap);
int rmcv_session_frame(const rmcv_session* s, int i, int k, void* out, int64_t cap, int64_t* size);
void rmcv_session_close(rmcv_session* s);
/* a pipeline's recorder: from the next submit of any form on, frames[0 .. n) of every batch are packed into `rec` behind the batch's pixel
 * kernel, off the pixel streams, so that rmcv_pipeline_wait(ticket) implies the entry is complete.  This call drains; no submit blocks
 * (rmcv_pipeline_info::host_blocking_calls stays 0).  n == 0 (or rec NULL): off -- a submit then enqueues exactly what it did before.
 * RMCV_ERR_BAD_ARG: an index repeated, negative or beyond the pipeline's max_frames; n beyond the recorder's max_frames; another device.  A
 * later submit whose n_frames does not reach every index, or whose rows or height are beyond the recorder's, is refused before anything
 * is enqueued. */
int rmcv_pipeline_set_recorder(rmcv_pipeline* pl, rmcv_recorder* rec, const int32_t* frames, int n);

/* ---- the recorder for the closed loop: loop records, tracked replay, device-side triggers --------------------------------
 * A recorder created with track_cap > 0 keeps, for every chosen frame k of every TRACKED submit (rmcv_pipeline_submit_tracked[_serial]), a
 * LOOP RECORD: the state of stream frames[k] right behind the batch's tracker step and aim step, written on the device by one launch
 * (k_loop_record, one workgroup per chosen frame) on the stream that ran those steps, in front of the tracker's event and of the batch's
 * completion -- rmcv_pipeline_wait(ticket) covers it.  A loop record is a rmcv_loop_state followed by n_tracks x { rmcv_track, float[8] }
 * (the side record: rmcv_tracker_get's last_vertices), in an area of rmcv_loop_bound(track_cap) bytes whose tail is zero.  Untracked
 * submits, stand-alone records and recorders with track_cap == 0 have none (rmcv_record_entry::loop_bytes == 0), and record exactly what
 * they did before.
 * The step of a batch is enqueued by the NEXT call on the pipeline (see rmcv_pipeline_submit): until then the readers of the recorder
 * (rmcv_recorder_count / _entry / _frame / _loop / _save) answer RMCV_ERR_BAD_ARG for that newest batch, with a message -- wait for its
 * ticket, or drain, first.  They never return a half-written record: each waits, 5 s deadline, for the packing AND the loop launch. */
#define RMCV_LOOP_TRUNCATED 1  /* rmcv_loop_state::flags: n_tracking exceeded the recorder's track_cap; the first track_cap tracks are kept */
typedef struct rmcv_loop_state {
    int32_t stream;              /* index of the stream = of the frame in its batch */
    int32_t n_tracking, status;  /* rmcv_tracker_counts' */
    int32_t n_armours;           /* the frame's armours the step observed */
    rmcv_point origin_next;      /* the requested origin the step left: the next batch's request (rmcv_tracker_get's origin) */
    rmcv_point origin_eff;       /* the effective origin this batch was read at (rmcv_batch_get_windows); (0, 0): whole frames */
    int32_t frame_status;        /* the frame's RMCV_FRAME_* word */
    int32_t has_camps;           /* bit 0: camp is the tracker's (rmcv_tracker_set_camps); bit 1: lower_bound too */
    int32_t camp, lower_bound;   /* raw, as the tracker's tables held them behind the step */
    int32_t has_key;             /* key[] holds the frame's effective detection key (the batch ran with per-frame keys) */
    int32_t key[4];              /* rmcv_batch_get_frame_keys' */
    int32_t has_cameras;         /* cam_eff is the effective index of a camera table (rmcv_pipeline_set_frame_cameras); else 0 */
    int32_t cam_eff;
    int32_t has_aim;             /* aiming was on: aim is this step's record */
    int32_t has_attitude;        /* attitude was on: attitude, packet_errors, attitude_config, gripper2camera are this batch's */
    int32_t has_packet;          /* packet[] holds the 24 bytes the attitude step of this batch read */
    int32_t packet_errors;
    int32_t n_tracks;            /* tracks stored behind this struct: min(n_tracking, track_cap of the recorder) */
    int32_t flags;               /* RMCV_LOOP_* */
    uint32_t fired;              /* RMCV_TRIG_* this record raised against its predecessor, BEFORE the trigger mask; 0 without one */
    int32_t has_prev;            /* a predecessor was compared */
    int32_t trig_frame_status_mask; /* the rule's inputs beside the two records, as the recorder's trigger config had them at the launch: */
    double  trig_aim_jump_deg;      /* with them fired can be recomputed from a file alone (+inf and 0 while triggers are off) */
    int64_t timestamp;           /* the step's */
    uint64_t sequence;           /* the recorder's, of the batch */
    rmcv_aim aim;
    rmcv_aim_input aim_input;    /* what the aim step read (behind this batch's attitude step) */
    rmcv_attitude attitude;
    uint8_t packet[24];
    rmcv_tracker_config tracker_config;    /* the setup the step ran under: a record is self-contained */
    rmcv_aim_config aim_config;            /* the stream's effective one (global or per-stream); zero without has_aim */
    rmcv_attitude_config attitude_config;  /* zero without has_attitude */
    double gripper2camera[16];             /* the stream's effective one (the config's or rmcv_tracker_set_stream_cameras'); zero without has_attitude */
} rmcv_loop_state;
/* bytes of one loop area: sizeof(rmcv_loop_state) + track_cap x (sizeof(rmcv_track) + 32); track_cap 0 .. RMCV_TRACKER_MAX_CAP, else -1 */
int64_t rmcv_loop_bound(int track_cap);

/* THE TRIGGER RULE, a pure function of two loop records of one stream in consecutive batches and the config (device_loop.h: loop_trigger,
 * compiled for host and device from one source).  had_target(r) := !(r.aim.status & RMCV_AIM_NO_TARGET); solved(r) := had_target(r) &&
 * !(r.aim.status & RMCV_AIM_NO_SOLUTION).
 *   RMCV_TRIG_NO_ARMOURS     prev.n_armours > 0 && cur.n_armours == 0
 *   RMCV_TRIG_TRACK_DROPPED  cur.n_tracking < prev.n_tracking
 *   RMCV_TRIG_TRACKER_OVF    (cur.status & RMCV_TRACKER_OVF) && !(prev.status & RMCV_TRACKER_OVF)
 *   RMCV_TRIG_FRAME_STATUS   (cur.frame_status & cfg.frame_status_mask & ~prev.frame_status) != 0
 *   only with prev.has_aim && cur.has_aim:
 *   RMCV_TRIG_TARGET_LOST    had_target(prev) && (cur.aim.status & RMCV_AIM_NO_TARGET)
 *   RMCV_TRIG_TARGET_SWITCH  had_target(prev) && had_target(cur) && cur.aim.identity != prev.aim.identity
 *   RMCV_TRIG_NO_SOLUTION    (cur.aim.status & RMCV_AIM_NO_SOLUTION) && !(prev.aim.status & RMCV_AIM_NO_SOLUTION)
 *   RMCV_TRIG_AIM_JUMP       solved(prev) && solved(cur) && (fabs(cur.aim.yaw - prev.aim.yaw) > cfg.aim_jump_deg ||
 *                            fabs(cur.aim.pitch - prev.aim.pitch) > cfg.aim_jump_deg)   -- a NaN difference compares false
 *   only with prev.has_attitude && cur.has_attitude:
 *   RMCV_TRIG_PACKET_ERROR   cur.packet_errors > prev.packet_errors
 * The device evaluates it for a record only against the record of the SAME chosen frame in the recorder's previous slot, and only when
 * that slot holds the immediately preceding sequence, of the same tracker, with the same chosen frames, recorded with loop records, and
 * no rmcv_recorder_resume lies between; otherwise nothing is compared, fired == 0 and has_prev == 0. */
#define RMCV_TRIG_NO_ARMOURS 1
#define RMCV_TRIG_TRACK_DROPPED 2
#define RMCV_TRIG_TRACKER_OVF 4
#define RMCV_TRIG_FRAME_STATUS 8
#define RMCV_TRIG_TARGET_LOST 16
#define RMCV_TRIG_TARGET_SWITCH 32
#define RMCV_TRIG_NO_SOLUTION 64
#define RMCV_TRIG_AIM_JUMP 128
#define RMCV_TRIG_PACKET_ERROR 256
#define RMCV_TRIG_ALL 511
typedef struct rmcv_trigger_config {
    uint32_t mask;              /* RMCV_TRIG_* that take the latch; 0: none */
    int32_t post_batches;       /* batches still recorded once the host has noticed the latch, >= 0 */
    int32_t frame_status_mask;  /* RMCV_FRAME_* bits RMCV_TRIG_FRAME_STATUS looks at */
    int32_t reserved;
    double aim_jump_deg;        /* RMCV_TRIG_AIM_JUMP's bound, in the unit of rmcv_aim::yaw / ::pitch; not NaN, >= 0 (+inf: never) */
} rmcv_trigger_config;
typedef struct rmcv_trigger_info {
    int32_t fired;              /* the latch is taken (as the host sees it now) */
    uint32_t mask;              /* fired & mask of the record that took it */
    uint64_t sequence;          /* the recorder sequence of its batch */
    int32_t k, stream;          /* the chosen frame's index in the entry, and its stream */
    int32_t noticed;            /* a submit has seen the latch */
    int32_t batches_since;      /* batches recorded since then */
} rmcv_trigger_info;
/* the rule on the host (no device).  prev / cur: loop records (only their fixed parts are read).  RMCV_ERR_BAD_ARG: a null argument. */
int rmcv_loop_trigger_host(const void* prev, const void* cur, const rmcv_trigger_config* cfg, uint32_t* fired);
/* THE LATCH.  A record with (fired & mask) != 0 takes the recorder's latch with one atomic compare-and-swap on a device word -- the first
 * wins -- and the winner writes {mask fired, sequence, k, stream} to device memory and to a mapped pinned host copy.  Every submit that
 * records reads that host copy on entry (a plain load: no HIP call, no wait); once it sees the latch, post_batches more batches are
 * recorded, STARTING WITH THE ONE BEING ENQUEUED, and the recorder is then frozen exactly as rmcv_recorder_freeze leaves it.
 * rmcv_recorder_resume clears the latch and re-arms it (synchronous: it waits for the recorder's launches in flight).
 * SIZING.  The step of the batch with sequence s, and with it the launch that may take the latch, is enqueued by the next call on the
 * pipeline, and is complete once its ticket t has been waited for or collected.  A caller keeps the pipeline's contract -- ticket t is
 * collected (or waited for) before ticket t + depth is submitted -- so the submit of sequence s + depth at the latest sees the latch, and
 * the last batch recorded is at most s + depth + post_batches - 1: a ring of
 *     slots >= depth + post_batches
 * still holds the triggering batch when the recorder freezes.  rmcv_pipeline_set_recorder, and every submit, refuse a recorder whose
 * triggers are armed on a smaller ring.  (A host that waits for every ticket before the next submit notices at s + 1 and holds exactly
 * post_batches batches behind s.)
 * cfg NULL: triggers off.  RMCV_ERR_BAD_ARG with a message: post_batches < 0, aim_jump_deg NaN or negative, mask beyond RMCV_TRIG_ALL, a
 * non-zero mask on a recorder with track_cap == 0. */
int rmcv_recorder_set_trigger(rmcv_recorder* rec, const rmcv_trigger_config* cfg);
int rmcv_recorder_trigger(rmcv_recorder* rec, rmcv_trigger_info* info);
/* frame k's loop record of held batch i: *size = rmcv_loop_bound(track_cap) bytes (the tail behind n_tracks tracks is zero).
 * RMCV_ERR_BAD_ARG: the batch has none; RMCV_ERR_CAPACITY: cap is smaller (*size says what is needed). */
int rmcv_recorder_loop(rmcv_recorder* rec, int i, int k, void* out, int64_t cap, int64_t* size);
int rmcv_session_loop(const rmcv_session* s, int i, int k, void* out, int64_t cap, int64_t* size);
/* rmcv_session_append for an entry with loop records: loops[k] = entry->loop_bytes bytes, written behind the packed frames.  The reader
 * checks loop_bytes against rmcv_loop_bound, and every record's n_tracks against loop_bytes, before it reads anything else of them. */
int rmcv_session_append_loop(const char* path, const rmcv_record_entry* entry, const void* user, const uint8_t* const* packed,
                             const uint8_t* const* loops);
/* RESTORING A TRACKER for a replay.  rmcv_tracker_restore sets stream `stream` of `trk` to what a loop record holds: list, side records,
 * count, status, requested origin (origin_next), camp and lower bound (with has_camps; the tracker's per-stream camps are switched on as
 * the record says), aim record and aim input (with has_aim), attitude and packet_errors (with has_attitude).  Synchronous.  The setup is
 * the caller's: the *_from_loop extractors hand it out (n_streams is the recorded tracker's).  RMCV_ERR_BAD_ARG with a message: a
 * truncated record (RMCV_LOOP_TRUNCATED), n_tracks outside 0 .. the tracker's track_cap or != n_tracking, has_aim / has_attitude on a
 * tracker whose aiming / attitude is off.  The extractors refuse a truncated record or an n_tracks outside 0 .. RMCV_TRACKER_MAX_CAP;
 * *has == 0: the part was off (the output is zero). */
int rmcv_tracker_restore(rmcv_tracker* trk, int stream, const void* loop_record);
int rmcv_tracker_config_from_loop(const void* loop_record, rmcv_tracker_config* out);
int rmcv_tracker_aim_config_from_loop(const void* loop_record, rmcv_aim_config* out, int32_t* has);
int rmcv_tracker_attitude_config_from_loop(const void* loop_record, rmcv_attitude_config* out, double gripper2camera[16], int32_t* has);

/* ---- dataset harvest: the labeler's job (executable/svm/labeler.cpp) on the device ---------------------------------
 * A dataset is `capacity_rows` icon rows (u8 [1200], as rmcv_batch_get_icons hands them out) and their metadata in device memory.  Any
 * batch whose last run included RMCV_STAGE_ARMOURS appends its armours' rows to it, with one label per frame (= per stream of a
 * labelling session) and no host round trip; no model is needed, and RMCV_STAGE_IDENTITY only for RMCV_HARVEST_MISSES.  The rule:
 *   - frame f contributes nothing when labels[f] == RMCV_HARVEST_SKIP or its status word carries an RMCV_FRAME_OVF_* bit;
 *   - otherwise its candidates are armours 0 .. min(n[f], max_armours) - 1 in the order of rmcv_batch_get_armours;
 *   - RMCV_HARVEST_MISSES keeps a candidate only when its identity != labels[f]; without the flag every candidate is kept;
 *   - kept rows are numbered frame-major, then armour-major; kept row k of the call goes to slot count + k;
 *   - a row whose slot is >= capacity is dropped: count = min(count + kept, capacity), dropped += max(0, count + kept - capacity).
 * Appends to one dataset land in the order of the calls, whatever streams they are enqueued on: each waits, on the device, for the
 * event of the one before.  The armour table is never written. */
#define RMCV_HARVEST_SKIP INT32_MIN /* a label: the frame contributes nothing */
#define RMCV_HARVEST_MISSES 1       /* a flag: keep only the armours the loaded model does not give the frame's label */
typedef struct rmcv_harvest_meta { /* 64 bytes per row */
    uint64_t tag;          /* the pipeline's ticket, or the caller's tag on a bare context */
    int32_t  frame, armour, label;
    int32_t  identity;     /* INT32_MIN when the run had no identity stage */
    int32_t  win_x, win_y; /* the frame's effective window origin; 0, 0 without windows */
    float    icon[4][2];   /* the icon quadrilateral as clamped by imgproc.cpp:11-15 (window coordinates in a windowed batch) */
} rmcv_harvest_meta;
typedef struct rmcv_harvest_item { int32_t frame, armour, slot; } rmcv_harvest_item;
typedef struct rmcv_dataset rmcv_dataset;
/* on the context's device; the context outlives the dataset (its deadline is the dataset's).  RMCV_ERR_BAD_ARG: capacity_rows < 1 */
int  rmcv_dataset_create(rmcv_ctx* ctx, int capacity_rows, rmcv_dataset** out);
void rmcv_dataset_destroy(rmcv_dataset* ds); /* waits for its last append */
int  rmcv_dataset_clear(rmcv_dataset* ds);   /* waits for its last append; count = dropped = 0 (and the novelty state: near, pushed, rings) */
const char* rmcv_dataset_last_error(const rmcv_dataset* ds);
/* waits for the last append with the context's deadline (RMCV_ERR_TIMEOUT); either pointer may be NULL */
int  rmcv_dataset_count(rmcv_dataset* ds, int32_t* rows, int64_t* dropped);
/* rows first .. first + n - 1 to host memory: rows_out u8 [n][1200], meta_out [n] (either may be NULL).  RMCV_ERR_BAD_ARG beyond count. */
int  rmcv_dataset_get(rmcv_dataset* ds, int first, int n, uint8_t* rows_out, rmcv_harvest_meta* meta_out);
/* zero-copy views: u8 [capacity][1200], rmcv_harvest_meta [capacity], and the int32 count (device memory).  Never synchronises: order a
 * reader behind the appending stream. */
int  rmcv_dataset_device(rmcv_dataset* ds, void** d_rows, void** d_meta, void** d_count);
/* append the bound batch's armours, behind its last run on `hip_stream` (NULL: the context's).  labels: n_frames int32, host, copied.
 * Asynchronous.  RMCV_ERR_BAD_ARG, with a message, before anything is enqueued: no frames bound; the last run lacked RMCV_STAGE_ARMOURS;
 * RMCV_HARVEST_MISSES without RMCV_STAGE_IDENTITY in the last run; unknown flags; a dataset of another device. */
int  rmcv_batch_harvest(rmcv_ctx* ctx, rmcv_dataset* ds, const int32_t* labels, int flags, uint64_t tag, void* hip_stream);
/* the same with the labels in DEVICE memory (n_frames int32), borrowed until the append has run */
int  rmcv_batch_harvest_device(rmcv_ctx* ctx, rmcv_dataset* ds, const void* d_labels, int flags, uint64_t tag, void* hip_stream);
/* the rule on the host (no context, no device).  identity [n_frames][max_armours]: may be NULL without RMCV_HARVEST_MISSES.  items_out:
 * the (frame, armour, slot) of every row that gets a slot, `cap` entries (RMCV_ERR_CAPACITY beyond; *n_items says what is needed);
 * *count_out, *dropped_out: the counters behind the call (dropped_in + what this call drops). */
int  rmcv_harvest_plan_host(const int32_t* n_armours, const int32_t* status, const int32_t* labels, const int32_t* identity, int n_frames,
                            int max_armours, int flags, int32_t count, int32_t capacity, int64_t dropped_in, rmcv_harvest_item* items_out, int cap,
                            int32_t* n_items, int32_t* count_out, int64_t* dropped_out);
/* every following submit appends its batch behind its sparse stage (with RMCV_STAGE_IDENTITY: behind the classifier); tag = the ticket.
 * labels: n_labels int32, host, copied.  ds NULL: off -- a submit then enqueues exactly what it did before.  The call itself may drain
 * the pipeline; no submit blocks (rmcv_pipeline_info::host_blocking_calls stays 0).  RMCV_ERR_BAD_ARG, with a message: what
 * rmcv_batch_harvest refuses; n_labels outside 1 .. max_frames; and, before anything is enqueued, a later submit whose batch has more
 * frames than the label table, lacks RMCV_STAGE_ARMOURS, or lacks RMCV_STAGE_IDENTITY under RMCV_HARVEST_MISSES.  Detach (ds NULL) before
 * destroying the dataset. */
int  rmcv_pipeline_set_harvest(rmcv_pipeline* pl, rmcv_dataset* ds, const int32_t* labels, int n_labels, int flags);
/* rmcv_svm_train on rows of the dataset, in place: rows = n int32 slot indices (host), or NULL = slots 0 .. n - 1; the responses are the
 * rows' labels.  The rows are gathered on the device and only the responses (4 bytes per row) come to the host; every output is bit-identical
 * to rmcv_svm_train on the same rows obtained through rmcv_dataset_get.  RMCV_ERR_BAD_ARG with a message: an index outside 0 .. count - 1,
 * n < 1 or beyond RMCV_SVM_MAX_SAMPLES, a dataset of another device, and everything rmcv_svm_train refuses. */
int  rmcv_svm_train_dataset(rmcv_ctx* ctx, rmcv_dataset* ds, const int32_t* rows, int n, const int32_t* perm, const rmcv_svm_train_params* params,
                            float* weights_out, double* rho_out, int32_t* labels_out, int32_t* n_class_out, rmcv_svm_train_report* report);
/* rmcv_svm_predict on rows of the dataset, in place (the validation pass of optimizer.cpp:27-40 without moving rows) */
int  rmcv_svm_predict_dataset(rmcv_ctx* ctx, rmcv_dataset* ds, const int32_t* rows, int n, int32_t* identity_out);

/* ---- novelty: a dataset that skips near-duplicates of the icons it kept last from the same stream -------------------
 * Consecutive frames of a stream show the same plate from almost the same pose; a dataset with novelty on remembers, per stream (= frame
 * index of every append), the last `ring_rows` rows it kept and does not keep a candidate whose sum of absolute byte differences to one
 * of them is <= max_sad.  The rule, in full (rmcv_amd/csrc/device_novelty.h is its one source for host and device):
 *   - the candidates of an append are exactly the rows it would keep with novelty off, taken frame by frame in armour order;
 *   - d = min of rmcv_icon_sad(row, r) over the rows r the frame's ring holds at that moment, rows pushed by earlier candidates of the same
 *     frame in the same append included; an empty ring gives no d and the candidate is kept;
 *   - d <= max_sad: the candidate is near -- not kept, near += 1; otherwise it is kept and pushed to the ring (the row pushed as number k
 *     lies at position k % ring_rows), whether or not the dataset has a slot left for it;
 *   - kept rows are numbered, placed, dropped and described exactly as with novelty off.
 * Novelty is a property of the dataset, not a flag: every append to it (rmcv_batch_harvest*, a pipeline's, rmcv_dataset_append_rows) is
 * filtered.  With ring_rows == 0 (the default) an append enqueues exactly what it did before. */
#define RMCV_ICON_SAD_MAX 306000  /* 1200 * 255 */
#define RMCV_HARVEST_RING_MAX 8
int32_t rmcv_icon_sad(const uint8_t* a, const uint8_t* b); /* host; two rows of 1200 bytes */
/* waits for the last append; allocates the rings on first use; sets ring_rows and max_sad and empties every ring (pushed = 0, every
 * position zero; `near` is kept).  ring_rows 0: off.  RMCV_ERR_BAD_ARG with a message: ring_rows outside 0 .. RMCV_HARVEST_RING_MAX,
 * max_sad outside 0 .. RMCV_ICON_SAD_MAX.  With a pipeline appending to the dataset, call it when every submitted ticket has been waited
 * for (the newest batch's append is enqueued by the call that waits for it), as rmcv_dataset_clear. */
int  rmcv_dataset_set_novelty(rmcv_dataset* ds, int ring_rows, int32_t max_sad);
/* waits like rmcv_dataset_count; any pointer may be NULL.  rmcv_dataset_clear additionally zeroes near, every pushed and every ring. */
int  rmcv_dataset_novelty(rmcv_dataset* ds, int* ring_rows, int32_t* max_sad, int64_t* near);
/* the state as it lies: rows_out u8 [n_streams][ring_rows][1200] (positions not yet written read as zero), pushed_out int64 [n_streams];
 * either may be NULL.  RMCV_ERR_BAD_ARG: streams outside 0 .. the creating context's max_frames - 1. */
int  rmcv_dataset_get_rings(rmcv_dataset* ds, int first_stream, int n_streams, uint8_t* rows_out, int64_t* pushed_out);
/* append rows the caller already has (icons of an earlier session, seeded rows): the same rule, in the same order as any other append, on
 * the creating context's stream.  rows u8 [sum n_rows][1200], stream-major; stream s gives n_rows[s] candidates in order, none when
 * labels[s] == RMCV_HARVEST_SKIP (its rows are stepped over).  Metadata: frame = s, armour = the index within the stream, label = labels[s],
 * identity = INT32_MIN, window origin 0, icon quadrilateral zeros.  Waits for the dataset's last append, then copies the host tables before it
 * returns; the append itself is asynchronous.  RMCV_ERR_BAD_ARG with a message, before anything is enqueued: a null pointer, n_streams
 * outside 1 .. the creating context's max_frames, an n_rows[s] outside 0 .. its max_armours. */
int  rmcv_dataset_append_rows(rmcv_dataset* ds, const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, uint64_t tag);
/* the rule on the host (no context, no device) over rows the caller has, laid out as for rmcv_dataset_append_rows.  rings u8
 * [n_streams][ring_rows][1200] and pushed int64 [n_streams]: in and out (NULL is allowed with ring_rows == 0); keep_out u8 [sum n_rows]: 1
 * kept, 0 near or skipped; min_sad_out (nullable) int32 [sum n_rows]: each candidate's d, INT32_MAX where the ring was empty, the stream
 * skipped or ring_rows == 0; *near_out (nullable): the near candidates of this call.  RMCV_ERR_BAD_ARG: null tables, n_streams < 0, a negative
 * n_rows[s], arguments rmcv_dataset_set_novelty refuses. */
int  rmcv_harvest_novel_host(const uint8_t* rows, const int32_t* n_rows, const int32_t* labels, int n_streams, int ring_rows, int32_t max_sad,
                             uint8_t* rings, int64_t* pushed, uint8_t* keep_out, int32_t* min_sad_out, int64_t* near_out);

/* ---- calibration capture: sub-pixel corner refinement ------------------------------------------------------------------
 * The pixel step of executable/calibration/hand_eye.cpp (:121, cornerSubPix(gray, corners, {8, 8}, {-1, -1}, {EPS + COUNT, 40, 0.001})) on
 * frames resident on the device.  The rule is the library's own pinned statement of cv::cornerSubPix, rmcv_amd/csrc/device_corner.h: one
 * source for the host form below and the kernel, which agree bit for bit.  Gray of a BGR pixel is (1868 B + 9617 G + 4899 R + 8192) >> 14.
 * A corner is two floats (x, y), pixel centres at integers, in the coordinates of SRC(f), the BGR image a frame's results are defined on
 * (a windowed batch: window coordinates).  The coarse guess is the caller's.  One status word per corner: */
#define RMCV_CORNER_ITERS_MASK 0xFF        /* bits 0-7: iterations run */
#define RMCV_CORNER_DET_ZERO   (1 << 8)    /* the window's gradient matrix was singular: the iteration stopped where it was */
#define RMCV_CORNER_LEFT_IMAGE (1 << 9)    /* the iterate left [0, w) x [0, h): the iteration stopped there */
#define RMCV_CORNER_REVERTED   (1 << 10)   /* the result lay more than (win_x, win_y) from the input: the input is returned */
#define RMCV_CORNER_CONVERGED  (1 << 11)   /* the last step's squared length was <= eps * eps */
#define RMCV_CORNER_BAD_INPUT  (1 << 12)   /* a non-finite input corner: left untouched, 0 iterations */
#define RMCV_CORNER_WIN_MAX 15             /* win_x, win_y: 1 .. 15 (the window is (2 win_x + 1) x (2 win_y + 1)) */
#define RMCV_CORNER_ITERS_MAX 100          /* max_iters: 1 .. 100 */
#define RMCV_CORNER_PER_FRAME_MAX 1024     /* corners per frame: 1 .. 1024 */
/* host, no context.  mask_out: (2 win_y + 1) rows of (2 win_x + 1) floats, the window's weights; zero zone (zero_x, zero_y): (-1, -1) none,
 * 0 <= zero_x < win_x && 0 <= zero_y < win_y zeroes the middle (2 zero_x + 1) x (2 zero_y + 1); anything else is RMCV_ERR_BAD_ARG (OpenCV
 * ignores it). */
int  rmcv_corner_mask(int win_x, int win_y, int zero_x, int zero_y, float* mask_out);
/* host, no context: gray_out[y * gray_stride + x] of a BGR image (stride >= 3 w, gray_stride >= w) */
int  rmcv_gray_host(const uint8_t* bgr, int w, int h, int stride, uint8_t* gray_out, int gray_stride);
/* host, no context: the sequential statement of the rule.  corners: n x 2 floats, refined in place; status_out (nullable): n words.
 * RMCV_ERR_BAD_ARG: a null buffer, w or h < 1, stride < 3 w, n < 0, win / zero zone / max_iters / eps (finite, >= 0) outside their limits. */
int  rmcv_corner_subpix_host(const uint8_t* bgr, int w, int h, int stride, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y,
                             int max_iters, double eps, int32_t* status_out);
/* stage-wise: the same through the kernel, on a host image and host corners, with device buffers of its own (nothing bound to the context
 * moves).  n: 1 .. RMCV_CORNER_PER_FRAME_MAX; w, h within the context's max_width / max_height.  Waits with the context's deadline. */
int  rmcv_corner_subpix(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, float* corners, int n, int win_x, int win_y, int zero_x,
                        int zero_y, int max_iters, double eps, int32_t* status_out);
/* the corners of n chosen frames of the batch bound, refined in place in the caller's device table: d_corners float [n][per_frame][2], chosen
 * frame k's corners in row k; d_counts (nullable) int32 [n]: row k holds d_counts[k] corners (clamped to 0 .. per_frame), entries beyond are not
 * touched; d_status (nullable) int32 [n][per_frame].  SRC(f) is read as rmcv_batch_source_views reads it: all five kinds of source, a windowed
 * batch at its effective origin, RMCV_OPT_ENHANCE through the frame's table -- for those two the call goes behind the run that made them (a
 * last run with RMCV_STAGE_BINARY).  Asynchronous: enqueued on hip_stream (NULL: the context's), ordered behind the context's earlier work;
 * borrowed frames must stay valid until it has finished.  RMCV_ERR_BAD_ARG with a message, before anything is enqueued: what
 * rmcv_batch_source_views refuses about frames and n; no frames bound; a null d_corners; per_frame outside 1 .. RMCV_CORNER_PER_FRAME_MAX;
 * win, zero zone, max_iters or eps outside their limits. */
int  rmcv_batch_refine_corners(rmcv_ctx* ctx, const int32_t* frames, int n, void* d_corners, int per_frame, const void* d_counts, int win_x,
                               int win_y, int zero_x, int zero_y, int max_iters, double eps, void* d_status, void* hip_stream);
/* one frame of the batch bound, host corners (n x 2 floats) in and out, status_out nullable: the batch call on a table of the context's own,
 * then a wait with the context's deadline */
int  rmcv_batch_get_refined_corners(rmcv_ctx* ctx, int frame, float* corners, int n, int win_x, int win_y, int zero_x, int zero_y, int max_iters,
                                    double eps, int32_t* status_out);

/* ---- calibration capture: the chessboard detector -------------------------------------------------------------------------
 * The step in front of the refinement in executable/calibration/hand_eye.cpp (:119, findChessboardCorners): the inner corners of a
 * cols x rows pattern, coarse (whole pixels), in the order and the coordinates rmcv_batch_refine_corners takes.  OpenCV's detector is not
 * restated: the rule is the library's own, in integer arithmetic throughout, written at the head of rmcv_amd/csrc/device_chess.h -- a ChESS
 * response, non-maximum suppression, a graph of mutually accepted neighbours whose edges run along square borders, a breadth-first labelling
 * -- one source for the host form below and the kernels, which agree byte for byte.  One status word per frame: */
#define RMCV_CHESS_COUNT_MASK 0x7FF        /* bits 0-10: candidates found, saturating */
#define RMCV_CHESS_FOUND      (1 << 11)    /* a board: cols * rows corners were written */
#define RMCV_CHESS_OVERFLOW   (1 << 12)    /* more than RMCV_CHESS_CAND_MAX candidates: no board, no candidate list */
#define RMCV_CHESS_NO_GRID    (1 << 13)    /* no component of the neighbour graph labels as a cols x rows grid */
#define RMCV_CHESS_CAND_MAX 1024
typedef struct rmcv_chess_params {
    int32_t threshold;  /* >= 0: a candidate's response exceeds it */
    int32_t contrast;   /* 0 .. 255: gray levels the two sides of an edge differ by, at least */
    int32_t nms;        /* 1 .. 7: a candidate is the maximum of its (2 nms + 1)^2 neighbourhood */
    int32_t dist_min;   /* 1 <= dist_min <= dist_max <= 1023: the distance of neighbouring corners, pixels */
    int32_t dist_max;
} rmcv_chess_params;
/* threshold 1000, contrast 10, nms 3, dist 6 .. 255: the values the rule was prototyped with on drawn boards, not tuned on footage */
void rmcv_chess_defaults(rmcv_chess_params* p);
/* host, no context: the sequential statement of the rule.  cols, rows: 2 .. 32 with cols * rows <= RMCV_CORNER_PER_FRAME_MAX; params: null =
 * the defaults.  corners_out: cols * rows x 2 floats, row-major (j * cols + i), written when a board is found (untouched otherwise);
 * status_out (nullable): the status word; cand_out (nullable): RMCV_CHESS_CAND_MAX x 3 int32, the candidates (x, y, R) in row-major order of
 * the image, *cand_n_out (nullable) rows written.  RMCV_ERR_BAD_ARG: a null image or corner table, w or h outside 1 .. 32767, stride < 3 w,
 * the pattern or a parameter outside its limits. */
int  rmcv_find_chessboard_host(const uint8_t* bgr, int w, int h, int stride, int cols, int rows, const rmcv_chess_params* params, float* corners_out,
                               int32_t* status_out, int32_t* cand_out, int32_t* cand_n_out);
/* stage-wise: the same through the kernels, on a host image, with device buffers of its own (nothing bound to the context moves).  w, h
 * within the context's max_width / max_height.  Waits with the context's deadline. */
int  rmcv_find_chessboard(rmcv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, int cols, int rows, const rmcv_chess_params* params,
                          float* corners_out, int32_t* status_out, int32_t* cand_out, int32_t* cand_n_out);
/* the boards of n chosen frames of the batch bound, into the caller's device tables: d_corners float [n][per_frame][2], chosen frame k's
 * corners at the head of row k; d_counts int32 [n]: cols * rows for a frame with a board, 0 for one without (whose corner row is not touched);
 * d_status (nullable) int32 [n].  The tables have the layout rmcv_batch_refine_corners reads: the two calls chain on the device.  SRC(f) is
 * read as rmcv_batch_refine_corners reads it, under the same condition for windowed and enhanced batches.  Asynchronous: enqueued on
 * hip_stream (NULL: the context's), ordered behind the context's earlier work.  RMCV_ERR_BAD_ARG with a message, before anything is
 * enqueued: what rmcv_batch_source_views refuses about frames and n; no frames bound; a null d_corners or d_counts; the pattern or a
 * parameter outside its limits; per_frame outside cols * rows .. RMCV_CORNER_PER_FRAME_MAX. */
int  rmcv_batch_find_chessboards(rmcv_ctx* ctx, const int32_t* frames, int n, int cols, int rows, const rmcv_chess_params* params, void* d_corners,
                                 int per_frame, void* d_counts, void* d_status, void* hip_stream);
/* one frame of the batch bound, host outputs as rmcv_find_chessboard_host's: the batch call on tables of the context's own, then a wait with
 * the context's deadline */
int  rmcv_batch_get_chessboard(rmcv_ctx* ctx, int frame, int cols, int rows, const rmcv_chess_params* params, float* corners_out, int32_t* status_out,
                               int32_t* cand_out, int32_t* cand_n_out);

/* ---- calibration solve: camera matrix and distortion from boards ------------------------------------------------------------
 * The first solver of executable/calibration/hand_eye.cpp (:128-131, calibrateCamera) on the tables rmcv_batch_find_chessboards and
 * rmcv_batch_refine_corners leave on the device: a capture is three asynchronous calls (find, refine, solve) and its result goes into
 * rmcv_pnp_load_cameras.  OpenCV's solver is not restated: the rule is the library's own, written at the head of
 * rmcv_amd/csrc/device_calib.h -- a homography per view (Hartley, DLT, a pinned cyclic Jacobi), intrinsics from the vanishing points, poses
 * as unit quaternions, Levenberg-Marquardt with per-view elimination, every sum in a pinned order -- one source for the host form below and
 * the kernels, which agree bit for bit.  calibrateHandEye is the next section.  One status word per camera: */
#define RMCV_CALIB_CONVERGED      (1 << 0)   /* an accepted step had |step|^2 <= eps^2 |parameters|^2 */
#define RMCV_CALIB_MAX_ITERS      (1 << 1)   /* max_iters trials were made */
#define RMCV_CALIB_STALLED        (1 << 2)   /* the damping passed 1e12 without an accepted step */
#define RMCV_CALIB_TOO_FEW_VIEWS  (1 << 3)   /* fewer than 3 used views: nothing but status, views_used and iters (0) is written */
#define RMCV_CALIB_BAD_INIT       (1 << 4)   /* the initial focal lengths or the initial cost are not finite and positive: likewise */
#define RMCV_CALIB_TOO_MANY_VIEWS (1 << 5)   /* more than RMCV_CALIB_VIEWS_PER_CAMERA_MAX used views: likewise */
#define RMCV_CALIB_VIEWS_MAX 4096
#define RMCV_CALIB_VIEWS_PER_CAMERA_MAX 256
#define RMCV_CALIB_CAMERAS_MAX 64
/* bits of fix_mask: the parameter keeps its initial value */
#define RMCV_CALIB_FIX_FX (1 << 0)
#define RMCV_CALIB_FIX_FY (1 << 1)
#define RMCV_CALIB_FIX_CX (1 << 2)
#define RMCV_CALIB_FIX_CY (1 << 3)
#define RMCV_CALIB_FIX_K1 (1 << 4)
#define RMCV_CALIB_FIX_K2 (1 << 5)
#define RMCV_CALIB_FIX_P1 (1 << 6)
#define RMCV_CALIB_FIX_P2 (1 << 7)
#define RMCV_CALIB_FIX_K3 (1 << 8)
typedef struct rmcv_calib_params {
    int32_t max_iters;  /* 1 .. 100: trials, accepted or not */
    int32_t fix_mask;   /* 0 .. 511 */
    double  eps;        /* finite, >= 0 */
} rmcv_calib_params;
/* max_iters 30, eps DBL_EPSILON (calibrateCamera's default criteria), fix_mask 0 */
void rmcv_calib_defaults(rmcv_calib_params* p);
typedef struct rmcv_calib_guess {  /* a camera's starting point, laid out as rmcv_pnp_config's head; camera_matrix[0] == 0: none for this camera */
    double camera_matrix[9];
    double dist[5];
} rmcv_calib_guess;
typedef struct rmcv_calib_result {
    double  camera_matrix[9];  /* as rmcv_pnp_config's */
    double  dist[5];           /* k1 k2 p1 p2 k3 */
    double  rms, rms_init;     /* sqrt(cost / points): what calibrateCamera returns, and the same at the starting point */
    int32_t views_used, iters, status, reserved;
} rmcv_calib_result;
typedef struct rmcv_calib_view {
    double  rvec[3], tvec[3];  /* board to camera, as calibrateCamera's rvecs / tvecs */
    double  q[4];              /* the same rotation as the unit quaternion (w, x, y, z) the solver carries */
    double  rms;
    int32_t used, reserved;    /* used = 1 is written for a used view of a solved camera; no other row is touched */
} rmcv_calib_view;
/* host, no context, one camera: the sequential statement of the rule.  corners float [n_views][per_frame][2], counts int32 [n_views]; a view
 * is used iff its count is cols * rows and its corners are finite.  params: null = the defaults; guess: nullable.  result: one;
 * views_out: n_views rows.  RMCV_ERR_BAD_ARG: a null table; n_views outside 1 .. RMCV_CALIB_VIEWS_MAX; cols * rows outside
 * 4 .. RMCV_CORNER_PER_FRAME_MAX or a side < 1; per_frame outside cols * rows .. RMCV_CORNER_PER_FRAME_MAX; square not finite and > 0; w or h < 1;
 * a parameter outside its limits; a guess that is not finite or has a focal length <= 0. */
int  rmcv_calibrate_camera_host(const float* corners, int per_frame, const int32_t* counts, int n_views, int cols, int rows, double square, int w, int h,
                                const rmcv_calib_params* params, const rmcv_calib_guess* guess, rmcv_calib_result* result, rmcv_calib_view* views_out);
/* a fleet in one call, on device tables: d_corners / d_counts as rmcv_batch_find_chessboards and rmcv_batch_refine_corners leave them;
 * d_view_camera (nullable: camera 0) int32 [n_views], any value (rmcv_batch_set_device_frame_cameras' rule); guesses: a HOST table of
 * n_cameras, nullable, copied; d_results rmcv_calib_result [n_cameras], d_views rmcv_calib_view [n_views].  Asynchronous: enqueued on
 * hip_stream (NULL: the context's), ordered behind the context's earlier work.  RMCV_ERR_BAD_ARG with a message, before anything is
 * enqueued: what the host form refuses; n_cameras outside 1 .. RMCV_CALIB_CAMERAS_MAX. */
int  rmcv_calibrate_cameras(rmcv_ctx* ctx, const void* d_corners, int per_frame, const void* d_counts, int n_views, const void* d_view_camera, int n_cameras,
                            int cols, int rows, double square, int w, int h, const rmcv_calib_params* params, const rmcv_calib_guess* guesses, void* d_results,
                            void* d_views, void* hip_stream);
/* stage-wise: one camera, host tables through the same kernels, with device buffers of its own.  Waits with the context's deadline. */
int  rmcv_calibrate_camera(rmcv_ctx* ctx, const float* corners, int per_frame, const int32_t* counts, int n_views, int cols, int rows, double square, int w,
                           int h, const rmcv_calib_params* params, const rmcv_calib_guess* guess, rmcv_calib_result* result, rmcv_calib_view* views_out);
/* camera_matrix and dist of a result into cfg; gripper2camera and the square are left alone.  RMCV_ERR_BAD_ARG: null, or a result without a
 * solution (none of CONVERGED, MAX_ITERS, STALLED) */
int  rmcv_calib_to_pnp_config(const rmcv_calib_result* result, rmcv_pnp_config* cfg);

/* ---- calibration solve: the gimbal-to-camera transform ----------------------------------------------------------------------
 * The second solver of executable/calibration/hand_eye.cpp (:140-155, calibrateHandEye) and the check loop behind it (:157-180), on the view
 * table rmcv_calibrate_cameras leaves on the device and a table of gimbal attitudes (rmcv_tracker_device_attitudes' layout): the fourth
 * asynchronous call of a camera's setup.  Its result is the h_gripper2camera of executable/main.cpp:14-19 and goes into
 * rmcv_pnp_config::gripper2camera, rmcv_attitude_config::gripper2camera and rmcv_tracker_set_stream_cameras.  OpenCV's solver is not
 * restated: the rule is the library's own, written at the head of rmcv_amd/csrc/device_handeye.h -- the closed form of Horaud and Dornaika
 * over all pairs of used views, every sum in a pinned order -- one source for the host form below and the kernel, which agree bit for bit.
 * One status word per camera: */
#define RMCV_HANDEYE_OK              (1 << 0)   /* rotation and translation solved */
#define RMCV_HANDEYE_T_UNOBSERVABLE  (1 << 1)   /* a pivot of the translation's 3 x 3 was not finite and > 0: t = 0, the rotation is reported */
#define RMCV_HANDEYE_TOO_FEW_VIEWS   (1 << 2)   /* fewer than 3 used views, or no pair left: nothing but status and the four counts is written */
#define RMCV_HANDEYE_TOO_MANY_VIEWS  (1 << 3)   /* more than RMCV_CALIB_VIEWS_PER_CAMERA_MAX used views: likewise */
typedef struct rmcv_handeye_params {
    double  min_w;        /* finite, in [0, 1): a pair whose relative rotation has a scalar part below it is skipped */
    int32_t reserved[2];
} rmcv_handeye_params;
/* min_w 0.5: relative turns over 120 degrees are skipped */
void rmcv_handeye_defaults(rmcv_handeye_params* p);
typedef struct rmcv_handeye_result {
    double  cam2gripper[16];   /* row-major 4x4 [R t; 0 1]: the h_gripper2camera hand_eye.cpp:165-167 assembles, rmcv_pnp_config::gripper2camera */
    double  q[4], t[3];        /* its rotation as the unit quaternion (w, x, y, z), w >= 0, and its translation (the views' tvec units) */
    double  eig[4];            /* the eigenvalues of the rotation's 4 x 4, ascending: eig[1] near eig[0] says the rotation is not determined */
    double  pivots[3];         /* the Cholesky pivots of the translation's 3 x 3; behind a failed one: 0 */
    double  rot_rms, trans_rms;   /* rms residuals of the rotation (quaternion units) and the translation equations over the pairs used */
    double  world_mean[3];     /* the mean of the board's origin in the base frame over the used views (the check loop, hand_eye.cpp:157-180) */
    double  world_rms;         /* the rms distance of those origins from their mean */
    int32_t views_used, pairs_used, pairs_skipped, sweeps;
    int32_t status, reserved[3];
} rmcv_handeye_result;         /* 320 bytes */
typedef struct rmcv_handeye_view {
    double  world[3];          /* the board's origin in the base frame as this view has it */
    int32_t used, reserved;    /* used = 1 is written for a used view of a solved camera; no other row is touched */
} rmcv_handeye_view;
/* host, no context, one camera: the sequential statement of the rule.  views rmcv_calib_view [n_views] as rmcv_calibrate_camera* leaves them
 * (q and tvec are read, and used); attitudes rmcv_attitude [n_views], radians; gripper_t double [n_views][3], null: zeros (hand_eye.cpp:150).
 * A view is used iff its used == 1 and every double read for it is finite.  params: null = the defaults.  result: one; views_out: n_views
 * rows.  RMCV_ERR_BAD_ARG: a null table; n_views outside 1 .. RMCV_CALIB_VIEWS_MAX; min_w not finite or outside [0, 1). */
int  rmcv_calibrate_hand_eye_host(const rmcv_calib_view* views, const rmcv_attitude* attitudes, const double* gripper_t, int n_views,
                                  const rmcv_handeye_params* params, rmcv_handeye_result* result, rmcv_handeye_view* views_out);
/* a fleet in one call, on device tables: d_views as rmcv_calibrate_cameras leaves them, d_attitudes as rmcv_tracker_device_attitudes,
 * d_gripper_t nullable, d_view_camera (nullable: camera 0) int32 [n_views], any value (rmcv_calibrate_cameras' rule); d_results
 * rmcv_handeye_result [n_cameras], d_views_out rmcv_handeye_view [n_views].  Asynchronous: enqueued on hip_stream (NULL: the context's),
 * ordered behind the context's earlier work; nothing is allocated.  RMCV_ERR_BAD_ARG with a message, before anything is enqueued: what the
 * host form refuses; n_cameras outside 1 .. RMCV_CALIB_CAMERAS_MAX. */
int  rmcv_calibrate_hand_eyes(rmcv_ctx* ctx, const void* d_views, const void* d_attitudes, const void* d_gripper_t, int n_views, const void* d_view_camera,
                              int n_cameras, const rmcv_handeye_params* params, void* d_results, void* d_views_out, void* hip_stream);
/* stage-wise: one camera, host tables through the same kernel, with device buffers of its own.  Waits with the context's deadline. */
int  rmcv_calibrate_hand_eye(rmcv_ctx* ctx, const rmcv_calib_view* views, const rmcv_attitude* attitudes, const double* gripper_t, int n_views,
                             const rmcv_handeye_params* params, rmcv_handeye_result* result, rmcv_handeye_view* views_out);
/* cam2gripper of a result into cfg->gripper2camera; nothing else of cfg is written.  RMCV_ERR_BAD_ARG: null; a result without a rotation
 * (neither OK nor T_UNOBSERVABLE); one with T_UNOBSERVABLE unless allow_rotation_only != 0 */
int  rmcv_handeye_to_pnp_config(const rmcv_handeye_result* result, rmcv_pnp_config* cfg, int allow_rotation_only);
int  rmcv_handeye_to_attitude_config(const rmcv_handeye_result* result, rmcv_attitude_config* cfg, int allow_rotation_only);

/* ---- device memory for hosts without HIP headers (tools/pipeline_bench.c): frames resident in HBM ------------------------------- */
int  rmcv_device_alloc(int device, int64_t bytes, void** d_ptr);
void rmcv_device_free(int device, void* d_ptr);
int  rmcv_device_upload(int device, void* d_dst, const void* h_src, int64_t bytes);   /* synchronous */
int  rmcv_device_download(int device, void* h_dst, const void* d_src, int64_t bytes); /* synchronous */

/* ---- synthetic stream: host generator, integer-only, bit-reproducible --- */
int      rmcv_synth_frame(uint8_t* bgr, int w, int h, int stride, uint64_t frame_index, int camp, int variant);
uint64_t rmcv_synth_checksum(const uint8_t* bgr, int w, int h, int stride);

#ifdef __cplusplus
}
#endif
#endif /* RMCV_ABI_H */
