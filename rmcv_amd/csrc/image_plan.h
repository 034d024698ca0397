// image_plan.h -- what a context knows about its 0/255 byte image (Bufs::binary) and how a pixel launch may use it.  A pure function of
// plain values, without HIP types, so that a host compiler alone can check it (tests/test_image_plan.py).
//
// The invariant: Bufs::imgmask describes the CONTENTS of Bufs::binary -- bit k of imgmask[f * h + y] clear means the 64
// bytes of word k of row y of frame f are zero.  It holds in IMAGE_TRACKED, for the first `frames` frames of w x h images, and only
// k_binary_ws maintains it.  A launch that finds it in force stores only the words that are or were non-zero ("delta"); any other
// launch stores every byte ("full").
#pragma once

namespace rmcv {

enum ImageTrack { IMAGE_UNKNOWN = 0, IMAGE_TRACKED };
struct ImageState {
    ImageTrack track;
    int w, h;   // IMAGE_TRACKED: the geometry the mask and the image are laid out for
    int frames; // ... and how many frames of them the mask describes
};
constexpr ImageState IMAGE_STATE_UNKNOWN = {IMAGE_UNKNOWN, 0, 0, 0};

// IMAGE_KERNEL_WS: k_binary_ws, every chunk of the batch.  IMAGE_KERNEL_OTHER: anything else that writes the image when it is wanted
// (k_binary in any mode, k_binary_enh, k_binary_win, k_binary_bayer, the per-frame chain, a caller's own image).
enum ImageKernel { IMAGE_KERNEL_WS = 0, IMAGE_KERNEL_OTHER };
struct ImageLaunch {
    ImageKernel kernel;
    bool image; // the byte image is wanted (no RMCV_STAGE_NO_IMAGE)
    int w, h, ww, frames;
};
enum ImageMode { IMAGE_FULL = 0, IMAGE_DELTA };
struct ImageStep { ImageMode mode; ImageState next; };

// mode: how the launch stores the image (meaningful for k_binary_ws alone); next: the state once the launch has been enqueued (ok) or
// has failed to be (an error leaves nothing known).
inline ImageStep image_step(const ImageState& st, const ImageLaunch& l, bool ok)
{
    ImageStep r = {IMAGE_FULL, st};
    if (!l.image) { // neither the image nor the mask is touched
        if (!ok) r.next = IMAGE_STATE_UNKNOWN;
        return r;
    }
    const bool same = st.track == IMAGE_TRACKED && st.w == l.w && st.h == l.h;
    if (l.kernel == IMAGE_KERNEL_WS && same && l.frames <= st.frames && l.ww <= 32) r.mode = IMAGE_DELTA;
    if (!ok || l.kernel != IMAGE_KERNEL_WS) {
        r.next = IMAGE_STATE_UNKNOWN;
        return r;
    }
    // (a batch with fewer frames than the mask covers leaves the rest of it valid: it still describes the buffer)
    r.next = {IMAGE_TRACKED, l.w, l.h, same && st.frames > l.frames ? st.frames : l.frames};
    return r;
}

// ---- the bit plane beside the image: plane word k of row y is zero exactly when image word k is, so in a delta launch the
// image's mask says which plane words to store as well -- as long as plane, row masks, image and image mask of the context all come from
// the SAME launches.  A pixel launch without the image (RMCV_STAGE_NO_IMAGE) writes plane and row masks alone and breaks that.
// sync: the leading frames whose plane and row masks were last written by a launch that wrote their image and its mask too (0: none).
struct PlaneStep { bool delta; int next; };
// mode: image_step's for this launch.  delta: k_binary_ws stores only the plane words that are or were non-zero, no pad words, and only the
// row masks that changed; next: `sync` once the launch has been enqueued (ok) or has failed to be.
inline PlaneStep plane_step(int sync, ImageMode mode, const ImageLaunch& l, bool ok)
{
    PlaneStep r = {false, 0};
    if (!l.image || l.kernel != IMAGE_KERNEL_WS) return r; // the plane is rewritten without the image, or the image's state is lost anyway
    r.delta = mode == IMAGE_DELTA && l.frames <= sync;
    // (a delta launch with fewer frames leaves the rest in sync: neither their planes nor their images are touched)
    if (ok) r.next = r.delta ? sync : l.frames;
    return r;
}

} // namespace rmcv
