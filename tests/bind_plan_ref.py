"""The batch context's host decisions as rmcv_host.hip made them before bind_plan.h, statement by statement, in Python: what
tests/test_bind_plan.py holds the header against.  Line numbers are those of rmcv_amd/csrc/rmcv_host.hip at the commit before the header
("Ellipse fit: device tests for every branch of its scalar tails and sums"); pixel_refusal is pixel_plan.h's, which those lines call."""
OK, BAD_ARG = 0, -1
STAGE_BINARY, STAGE_CONTOURS, STAGE_BLOBS, STAGE_ARMOURS, STAGE_IDENTITY, STAGE_POSE, STAGE_NO_IMAGE = 1, 2, 4, 8, 16, 32, 64
STAGE_MAX = 15 | STAGE_IDENTITY | STAGE_POSE | STAGE_NO_IMAGE
FRAME_OVF_BLOBS, FRAME_OVF_ARMOURS, FRAME_HULL = 4, 8, 32
INT_MAX = 2**31 - 1

LEGACY_BAYER = "the legacy matcher votes camps from BGR means: not for Bayer frames (RMCV_OPT_INPUT_FORMAT)"
LEGACY_ENH = "the legacy matcher votes camps from BGR means: not with RMCV_OPT_ENHANCE"
LEGACY_CAMPS = "the legacy matcher votes a camp per blob from BGR means: not with per-frame camps (rmcv_batch_set_frame_camps)"
CAMPS_BAYER = "per-frame camps with a Bayer input format (RMCV_OPT_INPUT_FORMAT): the mosaic kernel takes one camp per run; not supported"
CAMPS_ENH = "per-frame camps with RMCV_OPT_ENHANCE: the threshold table folds one lower bound per run; not supported"
WIN_BAYER = "windows with a Bayer input format (RMCV_OPT_INPUT_FORMAT): crop-then-demosaic has other border semantics; not supported"
WIN_ENH = "windows with RMCV_OPT_ENHANCE: the mean of a crop is not the frame's; not supported"
ENH_BAYER = "RMCV_OPT_ENHANCE with a Bayer input format: the mean of a demosaiced frame is not a function of the mosaic's sums"
LAYOUT_BITS = "a BGR frame with RMCV_OPT_INPUT_SAMPLE_BITS = 16: the option is for Bayer frames (RMCV_OPT_INPUT_FORMAT)"
LAYOUT_ORIENT = "a BGR frame with RMCV_OPT_INPUT_ORIENT set: the option is for Bayer frames (RMCV_OPT_INPUT_FORMAT)"
EVEN = "16-bit samples (RMCV_OPT_INPUT_SAMPLE_BITS): stride and frame_pitch are bytes and must be even"
WIN_SMALL = "window size out of range: win_w and win_h must be at least 1"
WIN_FRAMES = "window size out of range: larger than the frames"
WIN_LIMITS = "window size out of range: larger than the context's limits"


def pixel_refusal(fmt, enh, windows, keys, legacy):
    """pixel_plan.h, pixel_refusal"""
    if legacy:
        if fmt:
            return LEGACY_BAYER
        if enh:
            return LEGACY_ENH
        if keys:
            return LEGACY_CAMPS
    if keys:
        if fmt:
            return CAMPS_BAYER
        if enh:
            return CAMPS_ENH
    if windows:
        if fmt:
            return WIN_BAYER
        if enh:
            return WIN_ENH
    if fmt and enh:
        return ENH_BAYER
    return None


def pixel_bytes(fmt, bits):
    """rmcv_ctx.h, ctx_pixel_bytes"""
    return bits // 8 if fmt else 3


def check_layout(fmt, bits, orient):
    """lines 389-395"""
    if fmt != 0:
        return None
    if bits != 8:
        return LAYOUT_BITS
    if orient != 0:
        return LAYOUT_ORIENT
    return None


def check_windows(max_w, max_h, fw, fh, fmt, enh, win_w, win_h):
    """lines 408-415"""
    why = pixel_refusal(fmt, enh, True, False, False)
    if why:
        return why
    if win_w < 1 or win_h < 1:
        return WIN_SMALL
    if win_w > fw or win_h > fh:
        return WIN_FRAMES
    if win_w > max_w or win_h > max_h:
        return WIN_LIMITS
    return None


def set_geom_refusal(lim, opt, n, w, h, stride, pitch, win_w, win_h):
    """lines 427-435: (code, message); lim = (max_frames, max_width, max_height), opt = (format, bits, valid_bit, orient, enhance)"""
    fmt, bits, _, orient, enh = opt
    why = None
    bpp = pixel_bytes(fmt, bits)
    if n < 1 or n > lim[0]:
        why = "n_frames out of range"
    elif w < 1 or h < 1 or w > lim[1] or h > lim[2]:
        why = "frame size out of range"
    elif check_layout(fmt, bits, orient):
        why = check_layout(fmt, bits, orient)
    elif fmt and (w < 3 or h < 3):
        why = "a Bayer frame needs w >= 3 and h >= 3"
    elif stride < bpp * w or pitch < stride * (h - 1) + bpp * w:
        why = "bad stride/pitch"
    elif bpp == 2 and ((stride & 1) or (pitch & 1)):
        why = EVEN
    elif pixel_refusal(fmt, enh, False, False, False):
        why = pixel_refusal(fmt, enh, False, False, False)
    elif win_w > 0:
        why = check_windows(lim[1], lim[2], w, h, fmt, enh, win_w, win_h)
    return (BAD_ARG, why) if why else (OK, None)


def extent(w, h):
    """set_extent, lines 461-465: (w, h, ww, prow, plane_pitch)"""
    ww = (w + 63) // 64
    return w, h, ww, ww + 2, (h + 2) * (ww + 2)


def set_geom_fields(opt, gains, n, w, h, stride, pitch, win_w, win_h):
    """lines 438-454 and set_extent's fields: what the binding leaves in Geom, as the test program prints it"""
    fmt, bits, valid, orient, enh = opt
    sample_bytes = bits // 8 if fmt else 1
    win = 1 if win_w > 0 else 0
    return (enh, gains[0], gains[1], fmt, sample_bytes, valid if sample_bytes == 2 else 0, orient if fmt else 0, n, stride, pitch, w, h, win, 0) + \
        extent(win_w if win else w, win_h if win else h)


def extent_change(geom_w, geom_h, order_n, order_h, w, h, n):
    """line 466: (planes_change, order_change)"""
    return geom_w != w or geom_h != h, order_n != n or order_h != h


def upload(bpp, w, h, stride, pitch):
    """rmcv_batch_upload, lines 607-612 and 618: (refusal, device stride, device pitch, one copy); bpp 3 is a BGR frame (input_format 0)"""
    rowb = bpp * w
    why = None
    if bpp != 3 and (stride < rowb or pitch < stride * (h - 1) + rowb):
        why = "bad stride/pitch"
    elif bpp == 2 and ((stride & 1) or (pitch & 1)):
        why = EVEN
    dstride = (rowb + 15) & ~15
    dpitch = dstride * h
    return why, dstride, dpitch, stride == dstride and pitch == dpitch


def check_params(have_params, morph, stages, have_svm, have_pnp):
    """lines 573-577"""
    if not have_params:
        return "null params"
    if morph < 0 or morph > 2:
        return "bad morph"
    if stages <= 0 or stages > STAGE_MAX:
        return "bad stage mask"
    if (stages & STAGE_IDENTITY) and not have_svm:
        return "RMCV_STAGE_IDENTITY needs rmcv_svm_load first"
    if (stages & STAGE_POSE) and not have_pnp:
        return "RMCV_STAGE_POSE needs rmcv_pnp_load first"
    return None


def run_ladder(stages, timed, legacy, fmt, enh, win, keys):
    """run_stages, lines 520-564: the launches in the order they are enqueued, as (name, arguments...) tuples; the refusal first"""
    out = []
    why = pixel_refusal(fmt, enh, False, keys != 0, True) if legacy else None   # 520
    if not (stages & STAGE_CONTOURS):                                            # 529-533
        own = ((FRAME_OVF_BLOBS | FRAME_HULL) if stages & STAGE_BLOBS else 0) | (FRAME_OVF_ARMOURS if stages & STAGE_ARMOURS else 0)
        if own:
            out.append(("status_clear", own))
    one_sparse = (not timed) and (not legacy) and bool(stages & STAGE_CONTOURS) and bool(stages & STAGE_BLOBS)   # 537
    if stages & STAGE_BINARY:                                                    # 538-548
        if enh:
            out.append(("enhance_tables",))
        if win:
            out.append(("window_origins",))
        if keys:
            out.append(("frame_keys",))
        out.append(("binary", int(not (stages & STAGE_NO_IMAGE))))
    identity_fused = one_sparse and bool(stages & STAGE_ARMOURS) and bool(stages & STAGE_IDENTITY) and fmt == 0 and not enh and not win   # 552
    if one_sparse:                                                               # 553-554
        out.append(("sparse", int(bool(stages & STAGE_ARMOURS)), int(identity_fused)))
    elif stages & STAGE_CONTOURS:
        out.append(("contours",))
    fused = bool(stages & STAGE_BLOBS) and bool(stages & STAGE_ARMOURS)          # 556
    if one_sparse:                                                               # 557-560
        pass
    elif legacy and (stages & STAGE_BLOBS):
        out.append(("match", int(fused)))
    elif fused:
        out.append(("blobs_armours",))
    elif stages & STAGE_BLOBS:
        out.append(("blobs",))
    if not one_sparse and not fused and (stages & STAGE_ARMOURS):                # 562
        out.append(("armours",))
    if (stages & STAGE_IDENTITY) and not identity_fused:                         # 563
        out.append(("classify",))
    if stages & STAGE_POSE:                                                      # 564
        out.append(("pnp",))
    return why, out


def next_last_stages(last, stages):
    """line 566"""
    return stages if stages & STAGE_BINARY else last | stages


# rmcv_ctx_set_option, lines 707-785: option -> the condition on `value` of its `if`
OPTIONS = {
    1: lambda v: v == 4 or v == 8,              # RMCV_OPT_SPARSE_WAVES, 707
    4: lambda v: v == 0 or v == 1,              # RMCV_OPT_RUN_AHEAD, 711
    3: lambda v: 0 <= v <= 3,                   # RMCV_OPT_FRAME_UPLOAD, 715
    18: lambda v: v >= 0,                       # RMCV_OPT_TEST_SLOW_US, 720
    11: lambda v: v == 0 or v == 1,             # RMCV_OPT_PIXEL_HALO_NT, 724
    1001: lambda v: v == 0 or v == 1,           # the hidden option, 728
    14: lambda v: v == 0 or v == 1,             # RMCV_OPT_PIXEL_SHAPE, 732
    13: lambda v: 0 <= v <= 3,                  # RMCV_OPT_OVERLOADS, 736
    7: lambda v: v == 0 or v == 1,              # RMCV_OPT_DENSE_DEFER, 741
    5: lambda v: 0 <= v <= 2,                   # RMCV_OPT_CONTOUR_TIER, 745
    17: lambda v: 0 <= v <= 2,                  # RMCV_OPT_IMAGE_EXPORT, 749
    15: lambda v: v >= 0,                       # RMCV_OPT_WAIT_TIMEOUT_MS, 754
    16: lambda v: 0 <= v <= 10000000,           # RMCV_OPT_TEST_DELAY_US, 758
    19: lambda v: 0 <= v <= 4,                  # RMCV_OPT_INPUT_FORMAT (RMCV_INPUT_BGR .. RMCV_BAYER_BG), 762
    20: lambda v: v == 8 or v == 16,            # RMCV_OPT_INPUT_SAMPLE_BITS, 766
    21: lambda v: 0 <= v <= 4,                  # RMCV_OPT_INPUT_VALID_BIT, 770
    22: lambda v: 0 <= v <= 3,                  # RMCV_OPT_INPUT_ORIENT (MIRROR | FLIP), 774
    23: lambda v: v == 0 or v == 1,             # RMCV_OPT_ENHANCE, 778
    2: lambda v: 1 <= v <= 8,                   # RMCV_OPT_PIXEL_GROUPS, 782
}
# the ends of every option's accepted values (the header's table, checked against the conditions above by the test): option -> (lowest, highest)
OPTION_ENDS = {1: (4, 8), 4: (0, 1), 3: (0, 3), 18: (0, INT_MAX), 11: (0, 1), 1001: (0, 1), 14: (0, 1), 13: (0, 3), 7: (0, 1), 5: (0, 2), 17: (0, 2),
               15: (0, INT_MAX), 16: (0, 10000000), 19: (0, 4), 20: (8, 16), 21: (0, 4), 22: (0, 3), 23: (0, 1), 2: (1, 8)}
