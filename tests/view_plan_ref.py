"""A Python restatement of the refusals that take a frame list, as they stood at the commit BEFORE csrc/view_plan.h (4e5548f), statement by
statement, for tests/test_view_plan.py.  Each function names the lines it restates.  A case is a dict of plain values; frames is a list of
ints or None (a null pointer); pointers are truth values."""

# include/rmcv_abi.h
STAGE_BINARY, STAGE_CONTOURS, STAGE_BLOBS, STAGE_ARMOURS, STAGE_ALL = 1, 2, 4, 8, 15
VIEW_BLOBS, VIEW_NEGATIVES, VIEW_ARMOURS, VIEW_ALL = 1, 2, 4, 7
ICON_SIDE_MAX, CORNER_WIN_MAX, CORNER_ITERS_MAX, CORNER_PER_FRAME_MAX = 256, 15, 100, 1024
# csrc/source_view_plan.h: SourceKind
SOURCE_BGR, SOURCE_BGR_WIN, SOURCE_MOSAIC, SOURCE_MOSAIC_RAW, SOURCE_BGR_LUT = range(5)
DBL_MAX = 1.79769313486231570815e308

OK, NONE, TOO_MANY, OUTSIDE, REPEATED = range(5)


def frame_list_fault(frames, n, n_frames):
    """the rule itself, as every copy below has it: the count, then the entries in list order, an entry outside the batch in front of its
    being a repeat"""
    if frames is None or n < 1:
        return NONE
    if n > n_frames:
        return TOO_MANY
    for k in range(n):
        if frames[k] < 0 or frames[k] >= n_frames:
            return OUTSIDE
        if frames[k] in frames[:k]:
            return REPEATED
    return OK


def view_stages_needed(flags):
    """csrc/rmcv_internal.h:288-292"""
    need = STAGE_BINARY
    if flags & (VIEW_BLOBS | VIEW_NEGATIVES):
        need |= STAGE_CONTOURS | STAGE_BLOBS
    if flags & VIEW_ARMOURS:
        need |= STAGE_CONTOURS | STAGE_BLOBS | STAGE_ARMOURS
    return need


def debug_views(c):
    """csrc/rmcv_host.hip:1368-1385, ctx_view_check, with its std::vector of frames seen (need: its view_stages_needed(flags) of line 1382)"""
    frames, n, n_frames, vw, vh = c["frames"], c["n"], c["n_frames"], c["vw"], c["vh"]
    if frames is None or n < 1:
        return "debug views: no frames chosen"
    if n > n_frames:
        return "debug views: more views than the batch has frames"
    if c["flags"] < 0 or c["flags"] > VIEW_ALL:
        return "debug views: unknown view flags"
    if vw < 1 or vh < 1 or vw > c["max_width"] or vh > c["max_height"]:
        return "debug views: the view size must be 1 .. max_width x 1 .. max_height"
    if c["out_stride"] < 3 * vw:
        return "debug views: out_stride < 3 vw"
    if n > 1 and c["out_pitch"] < c["out_stride"] * (vh - 1) + 3 * vw:
        return "debug views: out_pitch < out_stride (vh - 1) + 3 vw"
    seen = [0] * n_frames
    for k in range(n):
        if frames[k] < 0 or frames[k] >= n_frames:
            return "debug views: a frame index is outside the batch"
        if seen[frames[k]]:
            return "debug views: a frame index is repeated"
        seen[frames[k]] = 1
    if (c["stages"] & c["need"]) != c["need"]:
        return "debug views: the batch's run lacked a stage the view flags need"
    return None


def source_views(c):
    """csrc/source_view_plan.h:38-54, source_views_refusal"""
    frames, n, n_frames, vw, vh = c["frames"], c["n"], c["n_frames"], c["vw"], c["vh"]
    if frames is None or n < 1:
        return "source views: no frames chosen"
    if n > n_frames:
        return "source views: more views than the batch has frames"
    if c["flags"] < 0 or c["flags"] > VIEW_ALL:
        return "source views: unknown view flags"
    if vw < 1 or vh < 1 or vw > c["max_width"] or vh > c["max_height"]:
        return "source views: the view size must be 1 .. max_width x 1 .. max_height"
    if c["out_stride"] < 3 * vw:
        return "source views: out_stride < 3 vw"
    if n > 1 and c["out_pitch"] < c["out_stride"] * (vh - 1) + 3 * vw:
        return "source views: out_pitch < out_stride (vh - 1) + 3 vw"
    for k in range(n):
        if frames[k] < 0 or frames[k] >= n_frames:
            return "source views: a frame index is outside the batch"
        for q in range(k):
            if frames[q] == frames[k]:
                return "source views: a frame index is repeated"
    if (c["stages"] & c["need"]) != c["need"]:
        return "source views: the batch's run lacked a stage the view flags need"
    return None


def icon_strips(c):
    """csrc/icon_strip_plan.h:41-56, icon_strips_refusal"""
    frames, n, n_frames, side, cap = c["frames"], c["n"], c["n_frames"], c["side"], c["cap"]
    if frames is None or n < 1:
        return "icon strips: no frames chosen"
    if n > n_frames:
        return "icon strips: more strips than the batch has frames"
    if side < 1 or side > ICON_SIDE_MAX:
        return "icon strips: side must be 1 .. 256"
    if cap < 1 or cap > c["max_armours"]:
        return "icon strips: cap must be 1 .. max_armours"
    if c["out_stride"] < 3 * cap * side:
        return "icon strips: out_stride < 3 cap side"
    if n > 1 and c["out_pitch"] < c["out_stride"] * (side - 1) + 3 * cap * side:
        return "icon strips: out_pitch < out_stride (side - 1) + 3 cap side"
    for k in range(n):
        if frames[k] < 0 or frames[k] >= n_frames:
            return "icon strips: a frame index is outside the batch"
        for q in range(k):
            if frames[q] == frames[k]:
                return "icon strips: a frame index is repeated"
    if not c["stages"] & STAGE_ARMOURS:
        return "icon strips: the batch's run lacked RMCV_STAGE_ARMOURS"
    return None


def _borrowed_list(c):
    """corner_plan.h:43 and chess_plan.h:50: source_views_refusal(frames, n, n_frames, ~0, 0, 1, 1, 1, 1, 0, 3, 3)"""
    return source_views(dict(frames=c["frames"], n=c["n"], n_frames=c["n_frames"], stages=-1, need=0, vw=1, vh=1, max_width=1, max_height=1, flags=0,
                             out_stride=3, out_pitch=3))


def corner_params(c):
    """csrc/corner_plan.h:15-23, corner_params_refusal"""
    wx, wy, zx, zy = c["win_x"], c["win_y"], c["zero_x"], c["zero_y"]
    if wx < 1 or wy < 1 or wx > CORNER_WIN_MAX or wy > CORNER_WIN_MAX:
        return "corners: win_x and win_y must be 1 .. 15"
    if not (zx == -1 and zy == -1) and not (0 <= zx < wx and 0 <= zy < wy):
        return "corners: the zero zone must be (-1, -1) or 0 <= zero_x < win_x and 0 <= zero_y < win_y"
    if c["max_iters"] < 1 or c["max_iters"] > CORNER_ITERS_MAX:
        return "corners: max_iters must be 1 .. 100"
    if not c["eps"] >= 0.0 or not c["eps"] <= DBL_MAX:
        return "corners: eps must be finite and >= 0"
    return None


def corners(c):
    """csrc/corner_plan.h:40-49, corners_refusal"""
    why = _borrowed_list(c)
    if why:
        return why
    if not c["d_corners"]:
        return "corners: null corner table"
    if c["per_frame"] < 1 or c["per_frame"] > CORNER_PER_FRAME_MAX:
        return "corners: per_frame must be 1 .. 1024"
    why = corner_params(c)
    if why:
        return why
    if c["kind"] in (SOURCE_BGR_WIN, SOURCE_BGR_LUT) and not c["stages"] & STAGE_BINARY:
        return "corners: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)"
    return None


def chess_params(c):
    """csrc/chess_plan.h:22-30, chess_params_refusal"""
    if c["cols"] < 2 or c["rows"] < 2 or c["cols"] > 32 or c["rows"] > 32:
        return "chessboard: cols and rows must be 2 .. 32"
    if c["threshold"] < 0:
        return "chessboard: threshold must be >= 0"
    if c["contrast"] < 0 or c["contrast"] > 255:
        return "chessboard: contrast must be 0 .. 255"
    if c["nms"] < 1 or c["nms"] > 7:
        return "chessboard: nms must be 1 .. 7"
    if c["dist_min"] < 1 or c["dist_min"] > c["dist_max"] or c["dist_max"] > 1023:
        return "chessboard: 1 <= dist_min <= dist_max <= 1023"
    return None


def chessboards(c):
    """csrc/chess_plan.h:47-56, chessboards_refusal"""
    why = _borrowed_list(c)
    if why:
        return why
    if not c["d_corners"] or not c["d_counts"]:
        return "chessboard: null corner or count table"
    why = chess_params(c)
    if why:
        return why
    if c["per_frame"] < c["cols"] * c["rows"] or c["per_frame"] > CORNER_PER_FRAME_MAX:
        return "chessboard: per_frame must be cols * rows .. 1024"
    if c["kind"] in (SOURCE_BGR_WIN, SOURCE_BGR_LUT) and not c["stages"] & STAGE_BINARY:
        return "chessboard: a windowed or enhanced batch is read behind a run with RMCV_STAGE_BINARY (its origins / tables)"
    return None
