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

} // namespace rmcv
