"""What rmcv_amd/csrc/frame_source.h's two fillers were before they were written once: the Python restatement of the two batch fillers
(corner_job_source of k_corner.hip; launch_source_view(g, b, ...) of k_view_source.hip with the view_job of rmcv_views.hip) and of the three
hand fills of one uploaded image (rmcv_corner_subpix, rmcv_find_chessboard, rmcv_source_view).  A filler is a dict of the fields it set; a
pointer is its offset from the base it was taken from, None for null.  merge() is the one FrameSource they add up to: where two of them set a
field they must have agreed, a field none of them set is zero or null (every job was zero-initialised)."""

SOURCE_BGR, SOURCE_BGR_WIN, SOURCE_MOSAIC, SOURCE_MOSAIC_RAW, SOURCE_BGR_LUT = range(5)
BAYER_RG, BAYER_GB, BAYER_GR, BAYER_BG = 1, 2, 3, 4
ORIENT_MIRROR, ORIENT_FLIP = 1, 2
LAY_S16, LAY_MIRROR, LAY_FLIP, LAY_VBIT_SHIFT = 1, 2, 4, 4

FIELDS = ("kind", "src", "src_end", "stride", "frame_pitch", "w", "h", "rx", "ry", "lay", "lut", "win_eff")
POINTERS = ("src", "src_end", "lut", "win_eff")
GEOM = ("input_format", "sample_bytes", "valid_bit", "orient", "enhance", "win", "n_frames", "w", "h", "frame_w", "frame_h", "stride", "frame_pitch")


def source_kind(g):
    if g["input_format"]:
        return SOURCE_MOSAIC if g["sample_bytes"] == 1 and g["orient"] == 0 else SOURCE_MOSAIC_RAW
    return SOURCE_BGR_LUT if g["enhance"] else SOURCE_BGR_WIN if g["win"] else SOURCE_BGR


def raw_layout(sample_bits, valid_bit, orient):
    return ((LAY_S16 | valid_bit << LAY_VBIT_SHIFT) if sample_bits == 16 else 0) | (LAY_MIRROR if orient & ORIENT_MIRROR else 0) | (LAY_FLIP if orient & ORIENT_FLIP else 0)


def raw_rx(pattern, lay, w):
    rx = 1 if pattern in (BAYER_GR, BAYER_BG) else 0
    return (w - 1 - rx) & 1 if lay & LAY_MIRROR else rx


def raw_ry(pattern, lay, h):
    ry = 1 if pattern in (BAYER_GB, BAYER_BG) else 0
    return (h - 1 - ry) & 1 if lay & LAY_FLIP else ry


def mosaic_fields(g):
    if not g["input_format"]:
        return dict(rx=0, ry=0, lay=0)
    lay = raw_layout(8 * g["sample_bytes"], g["valid_bit"], g["orient"])
    return dict(lay=lay, rx=raw_rx(g["input_format"], lay, g["w"]), ry=raw_ry(g["input_format"], lay, g["h"]))


def tables(kind):
    return dict(lut=0 if kind == SOURCE_BGR_LUT else None, win_eff=0 if kind == SOURCE_BGR_WIN else None)


def corner_job_source(g):
    kind = source_kind(g)
    return dict(kind=kind, src=0, stride=g["stride"], frame_pitch=g["frame_pitch"], w=g["w"], h=g["h"], **mosaic_fields(g), **tables(kind))


def launch_source_view(g):
    kind = source_kind(g)
    pixel_bytes = g["sample_bytes"] if g["input_format"] else 3
    end = (g["n_frames"] - 1) * g["frame_pitch"] + (g["frame_h"] - 1) * g["stride"] + pixel_bytes * g["frame_w"]
    return dict(kind=kind, src=0, src_end=end, stride=g["stride"], frame_pitch=g["frame_pitch"], w=g["w"], h=g["h"],  # (w, h: view_job's)
                **mosaic_fields(g), **tables(kind))


def stagewise_corner(w, h, dstride):  # rmcv_corner_subpix, and word for word rmcv_find_chessboard
    return dict(kind=SOURCE_BGR, src=0, stride=dstride, frame_pitch=dstride * h, w=w, h=h)


def stagewise_source_view(w, h, dstride):
    return dict(kind=SOURCE_BGR, src=0, src_end=dstride * (h - 1) + 3 * w, stride=dstride, frame_pitch=dstride * h, w=w, h=h)  # (w, h: the view job's)


def merge(*fills):
    out = {}
    for fill in fills:
        for k, v in fill.items():
            assert out.setdefault(k, v) == v, "the parent's fillers disagreed on " + k
    return {k: out.get(k, None if k in POINTERS else 0) for k in FIELDS}


def of_batch(g):
    return merge(corner_job_source(g), launch_source_view(g))


def packed(w, h, dstride):
    return merge(stagewise_corner(w, h, dstride), stagewise_corner(w, h, dstride), stagewise_source_view(w, h, dstride))
