"""The pipeline's decisions as rmcv_pipeline.hip made them before batch_plan.h, statement by statement, in Python: what
tests/test_batch_plan.py holds the header against, and what tests/test_gpu_pipeline.py predicts a deterministic schedule with.  Line
numbers are those of rmcv_amd/csrc/rmcv_pipeline.hip at the commit before the header ("Per-stream camera table and ballistics ...")."""
BAD_ARG = -1
STAGE_BINARY, STAGE_CONTOURS, STAGE_BLOBS, STAGE_ARMOURS, STAGE_IDENTITY, STAGE_POSE = 1, 2, 4, 8, 16, 32
STANDARD, LEAN, SPLIT_FIRST, SPLIT_SECOND, SPLIT_BOTH = 0, 1, 2, 3, 4  # sparse_plan.h: SparseForm
ARMOUR_BYTES = 88
CONFIG_FIELDS = ("depth", "pixel_streams", "sparse_streams", "armour_cap", "sparse_waves", "pixel_groups", "host_results", "dense_streams", "hot_contexts")
DEFAULTS = dict(zip(CONFIG_FIELDS, (8, 2, 4, 0, 4, 2, 1, 4, 0)))  # rmcv_default_pipeline_config, lines 175-189


def config(cfg):
    """rmcv_pipeline_create, lines 227-257: (rc, resolved config, hot_cfg); cfg: a dict of CONFIG_FIELDS or None.  A refused config resolves nothing."""
    d = dict(DEFAULTS)
    if cfg is not None:
        for k in ("depth", "pixel_streams", "sparse_streams", "armour_cap", "host_results"):
            if cfg[k] > 0:
                d[k] = cfg[k]
        d["sparse_waves"] = cfg["sparse_waves"] if cfg["sparse_waves"] > 0 else (4 if d["depth"] >= 3 else 8)
        d["pixel_groups"] = cfg["pixel_groups"] if cfg["pixel_groups"] > 0 else (2 if d["depth"] >= 2 else 3)
        for k in ("dense_streams", "hot_contexts"):
            if cfg[k] != 0:
                d[k] = cfg[k]
    if d["dense_streams"] < 0 or d["sparse_waves"] != 4 or d["host_results"] != 1:
        d["dense_streams"] = 0
    if d["depth"] > 64 or d["pixel_streams"] > 16 or d["sparse_streams"] > 16 or d["dense_streams"] > 16 or d["host_results"] > 2:
        return BAD_ARG, None, None
    for k in ("pixel_streams", "sparse_streams", "dense_streams"):
        d[k] = min(d[k], d["depth"])
    hot_given = cfg["hot_contexts"] if cfg is not None else 0
    if hot_given > 0 and (hot_given < 3 or hot_given >= d["depth"]):
        d["hot_contexts"] = -1
    if d["depth"] < 4 or d["host_results"] != 1 or d["sparse_waves"] != 4:
        d["hot_contexts"] = -1
    hot_cfg = -1 if d["hot_contexts"] < 0 else (hot_given if hot_given > 0 else 0)
    if d["hot_contexts"] < 0:
        d["hot_contexts"] = 0
    return 0, d, hot_cfg


def layout(max_frames, armour_cap):
    """lines 275-277, and the words lines 514 / 618 (max_frames + 2) and 553 / 888 (max_frames + 1) read: (cap, head, record, status, report)"""
    cap = armour_cap if armour_cap > 0 else 8 * max_frames
    head = ((max_frames + 3) * 4 + 15) // 16 * 16
    return cap, head, head + cap * ARMOUR_BYTES, max_frames + 1, max_frames + 2


def hot_for(hot_cfg, depth, n_frames, w, h):
    """lines 422-430"""
    if hot_cfg != 0:
        return hot_cfg if hot_cfg > 0 else 0
    plane = n_frames * (h + 2) * ((w + 63) // 64 + 2) * 8
    return min(max((200 << 20) // (plane if plane > 0 else 1), 3), depth - 1)


def hot_contexts_refusal(n, depth, host_results, sparse_waves):
    """rmcv_pipeline_set_hot_contexts for n > 0, lines 403-404"""
    if n < 3 or n >= depth:
        return "hot_contexts: 3 .. depth - 1, or 0 / -1 for off"
    if host_results != 1 or sparse_waves != 4:
        return "hot_contexts needs host_results = 1 and sparse_waves = 4"
    return None


def report_word(dense, points_per_frame):
    """k_detect.hip:242-243, the encoder: frames beyond the LDS tables | floor(mean border points per frame / 16), capped, << 20"""
    return (dense & 0xFFFFF) | (min(points_per_frame // 16, 4095) << 20)


def report(word):
    """lines 618-619 (and 514): (dense, points)"""
    return word & 0xFFFFF, (word >> 20) * 16


def mood(word, slot_lean, slot_frames):
    """lines 621-622: (heavy, calm)"""
    dense, points = report(word)
    heavy = points >= 1200 if slot_lean else (dense * 8 > slot_frames or points >= 1500)
    return heavy, dense == 0 and not heavy


def split_now(word, slot_frames):
    """lines 514-515"""
    dense = word & 0xFFFFF
    return dense > 0 and dense * 8 <= slot_frames


def front(hot, calm, heavy, host_results, sparse_waves, stages, legacy, ws_variant, tracked, hot_seq, k):
    """lines 628-629, 637-638: (fast, heavy, j); lines 667-668 then set plan.pixel_ws = fast and, if heavy, plan.form = SPARSE_LEAN"""
    heavy = bool(heavy and host_results == 1 and sparse_waves == 4 and not legacy and not (stages & (STAGE_IDENTITY | STAGE_POSE)) and
                 (stages & STAGE_CONTOURS) and (stages & STAGE_BLOBS))
    fast = bool(hot and calm and not legacy and not (stages & STAGE_POSE) and not (stages & STAGE_IDENTITY) and ws_variant and not tracked)
    return fast, heavy, (hot_seq % hot if fast else k)


def back(latency, sparse_waves, legacy, form, plan_waves, split_now_, n_dense, sparse, k):
    """lines 499-505, 518-520, 531-540: (w8, split, waves of the launches, form of the first or only launch, form of a split batch's second,
    the dense stream the list is finished on or -1 for B)"""
    heavy = form == LEAN
    w8 = bool(latency and sparse_waves == 4 and not legacy and not heavy)
    split = bool(not w8 and not heavy and split_now_ and n_dense > 0 and not legacy and (sparse & STAGE_CONTOURS) and (sparse & STAGE_BLOBS))
    return w8, split, (8 if w8 else plan_waves), (SPLIT_FIRST if split else form), (SPLIT_SECOND if split else None), (k % n_dense if split else -1)


def place(t, depth, pixel_streams, sparse_streams):
    """lines 610, 669: (slot, pixel stream, sparse stream)"""
    return t % depth, t % pixel_streams, (t % depth) % sparse_streams


def hold_back(fast, t, was_cold, prev_live, prev_done, ws_full, n_frames, w, h):
    """lines 700-716: (cold, hold_us); prev_live: slot_ticket[s_] == t, prev_done: its hipEventQuery, ws_full: pixel_ws_full"""
    cold, hold = False, 0
    if fast:
        cold = t == 0
        if t > 0:
            cold = prev_live and prev_done
        if not cold and was_cold and prev_live and ws_full:
            launch_us = n_frames * 4.0 * w * h / 5.5e6
            hold = 0 if launch_us < 100.0 else int(launch_us / 4.0 if launch_us / 4.0 < 60.0 else 60.0)
    return cold, hold


def tracked_refusal(tracker_device, device, n_streams, frame_w, frame_h, n_frames, w, h, stages, packets, attitude_on):
    """lines 598-605: the message, or None"""
    if tracker_device != device:
        return "rmcv_pipeline_submit_tracked: the tracker lives on another device than the pipeline"
    if n_frames != n_streams:
        return "rmcv_pipeline_submit_tracked: n_frames differs from the tracker's n_streams (frame f is the next frame of stream f)"
    if w != frame_w or h != frame_h:
        return "rmcv_pipeline_submit_tracked: the frame size differs from the tracker's config"
    if not (stages & STAGE_ARMOURS):
        return "rmcv_pipeline_submit_tracked: the stages have no RMCV_STAGE_ARMOURS: nothing to track"
    if packets and not attitude_on:
        return "rmcv_pipeline_submit_tracked_serial: packets given and the tracker's attitude is off (rmcv_tracker_set_attitude)"
    return None


def cameras_refusal(n_frames, cam_frames, tables_agree):
    """lines 648-658: the message, or None"""
    if n_frames != cam_frames:
        return "the batch has %d frames, the pipeline's camera table %d (rmcv_pipeline_set_frame_cameras)" % (n_frames, cam_frames)
    if not tables_agree:
        return "n_cameras differs between the pipeline's contexts: load the same cameras into EVERY slot (rmcv_pipeline_context, rmcv_pnp_load_cameras)"
    return None
