"""rmcv_pipeline_* (include/rmcv_abi.h): the pipelined batch schedule, owned by the library.

The reference's process loop (executable/main.cpp:163-209) takes a frame, detects, hands the armours on.  Its batch form keeps
`depth` batches in flight on one GPU -- pixel kernels of consecutive batches alternating over two streams, the per-frame kernels on
four higher-priority streams, everything chained by events inside librmcv_hip.so.  This module is the thin ctypes face of the three
calls (submit / collect / drain) plus the hook through which a device-side consumer -- the multi-GPU gather -- rides along.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import ARMOUR, STAGE_ALL, Limits, PipelineConfig, PipelineInfo, RmcvError, default_params, lib, ptr
from .api import Context


class Pipeline:
    def __init__(self, device=0, depth=0, pixel_streams=0, sparse_streams=0, armour_cap=0, sparse_waves=0, pixel_groups=0,
                 host_results=0, dense_streams=0, hot_contexts=0, input_format=0, sample_bits=8, valid_bit=0, mirror=False, flip=False, enhance=None,
                 **limits):
        lim = Limits()
        lib().rmcv_default_limits(C.byref(lim))
        for k, v in limits.items():
            setattr(lim, k, v)
        self.limits = lim
        cfg = PipelineConfig(depth, pixel_streams, sparse_streams, armour_cap, sparse_waves, pixel_groups, host_results, dense_streams, hot_contexts, 0)
        h = C.c_void_p()
        rc = lib().rmcv_pipeline_create(int(device), C.byref(lim), C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RmcvError(rc, "rmcv_pipeline_create failed (no GPU? this library has no CPU path)")
        self._h, self._lib, self.device = h, lib(), device
        self.info = self.get_info()
        self.depth = self.info.depth
        self._hook = None              # keeps the ctypes callback alive
        self._keep = {}                # slot -> the frames object of the batch in flight there
        self._n = {}                   # slot -> frames of the batch that lives there
        self._shape = {}               # slot -> (n, h, w) of what that batch's getters return (the window's for a windowed batch)
        self._ticket = C.c_uint64(0)
        self._params = default_params()
        self.contexts = [Context.borrowed(self._lib.rmcv_pipeline_context(self._h, k), lim, device) for k in range(self.depth)]
        self.input_format = int(input_format)
        if self.input_format:  # RMCV_OPT_INPUT_FORMAT on every slot: each batch reads its own context's option
            for c in self.contexts:
                c.set_input_format(self.input_format)
        self.sample_bits = int(sample_bits)
        if self.sample_bits != 8 or valid_bit or mirror or flip:  # the frame as the sensor delivers it, on every slot likewise
            for c in self.contexts:
                c.set_input_layout(sample_bits, valid_bit, mirror, flip)
        if enhance:  # RMCV_OPT_ENHANCE on every slot: True, or the gains (max, min)
            self.set_enhance(True, *(enhance if isinstance(enhance, (tuple, list)) else ()))

    def set_enhance(self, on=True, max_gain=None, min_gain=None):
        """RMCV_OPT_ENHANCE (and the gains) on every slot's context, from the next submit on: batches are read through their frames'
        rm::AutoEnhance tables and stay out of the hot rotation"""
        for c in self.contexts:
            c.set_enhance(on, max_gain, min_gain)

    def close(self):
        if getattr(self, "_h", None):
            for c in self.contexts:
                c.close()
            self._lib.rmcv_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RmcvError(rc, self._lib.rmcv_pipeline_last_error(self._h).decode())

    def get_info(self):
        o = PipelineInfo()
        self._chk(self._lib.rmcv_pipeline_get_info(self._h, C.byref(o)))
        return o

    def set_frame_models(self, d_idx, n=0, keepalive=None):
        """the frames' model indices for every following submit with STAGE_IDENTITY (rmcv_pipeline_set_frame_models): d_idx a device pointer
        to n int32, borrowed until replaced (keepalive= is held for that long); None: off.  Load the models into every slot first:
        `for c in pipeline.contexts: c.svm_load_models(models)`.  The device camps table of submit_camps may be the same buffer."""
        self._models_ref = keepalive if d_idx else None
        self._chk(self._lib.rmcv_pipeline_set_frame_models(self._h, C.c_void_p(int(d_idx)) if d_idx else None, int(n)))

    def set_frame_cameras(self, d_idx, n=0, keepalive=None):
        """the frames' camera indices for every following submit with STAGE_POSE (rmcv_pipeline_set_frame_cameras): d_idx a device pointer
        to n int32, borrowed until replaced (keepalive= is held for that long); None: off.  Load the cameras into every slot first:
        `for c in pipeline.contexts: c.pnp_load_cameras(cfgs)`."""
        self._cams_ref = keepalive if d_idx else None
        self._chk(self._lib.rmcv_pipeline_set_frame_cameras(self._h, C.c_void_p(int(d_idx)) if d_idx else None, int(n)))

    # ------------------------------------------------------------------ the three calls
    def submit(self, data_ptr, n, h, w, params=None, stages=STAGE_ALL, stride=None, frame_pitch=None, keepalive=None, legacy=None, windows=None, tracker=None, timestamp=0, camps=None, packets=None):
        """enqueue one batch of frames resident in HBM (data_ptr: e.g. torch_tensor.data_ptr()); returns the ticket.
        windows = (d_origins_ptr, win_w, win_h): a windowed batch -- d_origins_ptr a device pointer to n (x, y) int32 pairs (e.g. an
        int32 (n, 2) torch tensor's data_ptr(); keep it alive like the frames), results in window coordinates (Context.set_windows).
        tracker = a rmcv_amd.Tracker (+ timestamp): a tracked batch (rmcv_pipeline_submit_tracked) -- windowed at the tracker's own origins
        when its win_w > 0, whole frames otherwise; one step of the tracker runs behind the batch, and the next tracked submit on that
        tracker reads the origins it wrote: the closed loop with the host only submitting
        camps = (d_camps_ptr, d_lower_bounds_ptr or None): per-frame detection keys (rmcv_pipeline_submit_camps) -- device pointers to n
        int32 each (keep them alive like the frames); composes with windows=.  A tracker with set_camps brings its own.
        packets = device pointer to n x 24 bytes: the tracked batch's serial packets (rmcv_pipeline_submit_tracked_serial; keep them alive like
        the frames) for a tracker with set_attitude -- the attitude step runs in front of the batch: packet in, aim out, the host only submits"""
        if params is not None:
            self._params = params
        stride = stride or (w * self.sample_bits // 8 if self.input_format else 3 * w)
        frame_pitch = frame_pitch or stride * h
        if tracker is not None:
            assert legacy is None and windows is None and camps is None, "a tracked batch takes its windows and camps from the tracker"
            if packets is not None:
                rc = self._lib.rmcv_pipeline_submit_tracked_serial(self._h, tracker._h, data_ptr, n, w, h, stride, frame_pitch, int(packets),
                                                                   C.addressof(self._params), int(stages), int(timestamp), C.addressof(self._ticket))
            else:
                rc = self._lib.rmcv_pipeline_submit_tracked(self._h, tracker._h, data_ptr, n, w, h, stride, frame_pitch, C.addressof(self._params), int(stages),
                                                            int(timestamp), C.addressof(self._ticket))
            if tracker.config.win_w > 0:
                windows = (0, tracker.config.win_w, tracker.config.win_h)   # (the shape of what the getters return)
        elif packets is not None:
            raise ValueError("packets= belongs to a tracked batch (tracker=)")
        elif camps is not None:
            assert legacy is None, "the legacy matcher votes a camp per blob: no per-frame camps"
            d_camps, d_lbs = camps
            d_origins, win_w, win_h = windows if windows is not None else (0, 0, 0)
            rc = self._lib.rmcv_pipeline_submit_camps(self._h, data_ptr, n, w, h, stride, frame_pitch, int(d_camps), None if d_lbs is None else int(d_lbs),
                                                      int(d_origins) or None, int(win_w), int(win_h), C.addressof(self._params), int(stages), C.addressof(self._ticket))
        elif windows is not None:
            assert legacy is None, "the legacy matcher has no windowed submit"
            d_origins, win_w, win_h = windows
            rc = self._lib.rmcv_pipeline_submit_windows(self._h, data_ptr, n, w, h, stride, frame_pitch, int(d_origins), int(win_w), int(win_h),
                                                        C.addressof(self._params), int(stages), C.addressof(self._ticket))
        elif legacy is not None:
            rc = self._lib.rmcv_pipeline_submit_legacy(self._h, data_ptr, n, w, h, stride, frame_pitch, C.addressof(self._params), C.addressof(legacy),
                                                       int(stages), C.addressof(self._ticket))
        else:
            rc = self._lib.rmcv_pipeline_submit(self._h, data_ptr, n, w, h, stride, frame_pitch, C.addressof(self._params), int(stages),
                                                C.addressof(self._ticket))
        if rc != 0:
            self._chk(rc)
        t = self._ticket.value
        self._keep[t % self.depth] = (keepalive, tracker)
        self._n[t % self.depth] = n
        self.shape = (n, h, w) if windows is None else (n, int(windows[2]), int(windows[1]))
        self._shape[t % self.depth] = self.shape     # (windowed and whole-frame batches may alternate: context_of hands out the ticket's)
        for c in self.contexts:
            c.shape = self.shape
        return t

    def wait(self, ticket):
        self._chk(self._lib.rmcv_pipeline_wait(self._h, int(ticket)))

    def collect(self, ticket, cap=None):
        """(ARMOUR[total], frame_offs int32[n + 1]) of the batch, frame-major"""
        cap = cap or self.info.armour_cap
        out = np.empty(cap, ARMOUR)
        offs = np.empty(self.limits.max_frames + 1, np.int32)
        tot = C.c_int32(0)
        self._chk(self._lib.rmcv_pipeline_collect(self._h, int(ticket), ptr(out), cap, ptr(offs), C.addressof(tot)))
        n = self._n[int(ticket) % self.depth]
        return out[:tot.value].copy(), offs[:n + 1].copy()

    # ------------------------------------------------------------------ the operator's debug views
    def set_views(self, frames, size=(1024, 768), flags=abi.VIEW_ALL, source=False):
        """from the next submit on, every batch renders the debug images of `frames` (indices into the batch) at size = (vw, vh) behind its
        sparse stage, into its slot's own buffer (rmcv_pipeline_set_views: allocates and drains HERE; no submit blocks).  frames empty or
        None: off.  source: the source views instead (rmcv_pipeline_set_source_views: the frame under the overlays, not the
        binary); a pipeline renders one kind at a time, the one set last."""
        fr = np.ascontiguousarray(frames if frames is not None else [], np.int32).reshape(-1)
        setter = self._lib.rmcv_pipeline_set_source_views if source else self._lib.rmcv_pipeline_set_views
        self._chk(setter(self._h, ptr(fr) if len(fr) else None, len(fr), int(size[0]), int(size[1]), int(flags)))

    def set_sheets(self, frames, size=(640, 512), side=80, flags=abi.VIEW_ALL):
        """from the next submit on, every batch renders the labeler's sheets of `frames` at view size = (vw, vh) with icons of
        side x side: views() then returns [n, vh + side, 2 vw, 3] (rmcv_pipeline_set_sheets: allocates and drains HERE; no submit blocks).
        A third kind of view: the one set last wins.  frames empty or None: off."""
        fr = np.ascontiguousarray(frames if frames is not None else [], np.int32).reshape(-1)
        self._chk(self._lib.rmcv_pipeline_set_sheets(self._h, ptr(fr) if len(fr) else None, len(fr), int(size[0]), int(size[1]), int(side), int(flags)))

    def set_view_labels(self, what, scale=1):
        """from the next submit on, the label pass over every batch's views, whichever kind is set: what = abi.LABEL_ARMOURS
        (the armours' lines) | abi.LABEL_TRACKS (the tracker's targets, behind the tracker step of the same tracked submit) at an integer
        `scale` 1 .. 8 (rmcv_pipeline_set_view_labels: drains HERE; no submit blocks).  what 0: off.  Refused while no views are set."""
        self._chk(self._lib.rmcv_pipeline_set_view_labels(self._h, int(what), int(scale)))

    def views(self, ticket):
        """the views of a ticket's batch as a torch uint8 tensor [n, vh, vw, 3] OVER the slot's device buffer (no copy): complete once the
        ticket has been waited for, valid until ticket + depth is submitted"""
        import torch
        d, stride, pitch, n = C.c_void_p(), C.c_int32(0), C.c_int64(0), C.c_int32(0)
        self._chk(self._lib.rmcv_pipeline_views(self._h, int(ticket), C.addressof(d), C.addressof(stride), C.addressof(pitch), C.addressof(n)))
        vw = stride.value // 3
        vh = pitch.value // stride.value

        class _Span:  # what torch needs to see device memory it does not own
            __cuda_array_interface__ = {"shape": (n.value, vh, vw, 3), "typestr": "|u1", "data": (d.value, False), "version": 2, "strides": None}
        return torch.as_tensor(_Span(), device="cuda:%d" % self.device)

    # ------------------------------------------------------------------ the session recorder
    def set_recorder(self, rec, frames):
        """from the next submit of any form on, every batch packs `frames` (indices into the batch) losslessly into the Recorder `rec`,
        behind its pixel kernel and off the pixel streams: wait(ticket) implies the entry is complete (rmcv_pipeline_set_recorder: drains
        HERE; no submit blocks).  rec None or frames empty: off."""
        fr = np.ascontiguousarray(frames if frames is not None and rec is not None else [], np.int32).reshape(-1)
        self._chk(self._lib.rmcv_pipeline_set_recorder(self._h, rec._h if rec is not None else None, ptr(fr) if len(fr) else None, len(fr)))
        self._recorder = rec if len(fr) else None   # (kept alive as long as batches go into it)

    def set_harvest(self, ds, labels=None, flags=0):
        """from the next submit of any form on, every batch appends its armours' icon rows to the DeviceDataset `ds` behind its sparse stage
        (behind the classifier with STAGE_IDENTITY), tagged with its ticket, in ticket order (rmcv_pipeline_set_harvest: drains HERE; no
        submit blocks).  labels: one int per frame of the batches to come (HARVEST_SKIP: none of that frame).  ds None: off -- detach
        before closing the dataset."""
        lb = np.ascontiguousarray(labels if labels is not None and ds is not None else [], np.int32).reshape(-1)
        self._chk(self._lib.rmcv_pipeline_set_harvest(self._h, ds._h if ds is not None else None, ptr(lb) if len(lb) else None, len(lb), int(flags)))
        self._harvest = ds   # (kept alive as long as batches go into it)

    def set_hot_contexts(self, n):
        """rmcv_pipeline_config::hot_contexts from the next submit on (0: off)"""
        self._chk(self._lib.rmcv_pipeline_set_hot_contexts(self._h, int(n)))

    def set_wait_timeout(self, ms):
        """deadline of wait / collect / drain in milliseconds (0: none); a wait that runs out raises RmcvError(ERR_TIMEOUT)"""
        self._chk(self._lib.rmcv_pipeline_set_wait_timeout(self._h, int(ms)))

    def drain(self):
        self._chk(self._lib.rmcv_pipeline_drain(self._h))

    def context_of(self, ticket):
        """the Context view of the slot a (waited-for) ticket lives in: per-stage getters (binary, contours, blobs, counts)"""
        h = self._lib.rmcv_pipeline_context_of(self._h, int(ticket))
        if not h:
            raise RmcvError(abi.ERR_BAD_ARG, "ticket %d: %s" % (ticket, self._lib.rmcv_pipeline_last_error(self._h).decode()))
        for c in self.contexts:
            if c._h.value == h:
                c.shape = self._shape.get(int(ticket) % self.depth, c.shape)
                return c
        raise RmcvError(abi.ERR_BAD_ARG, "unknown context")

    def record(self, ticket):
        """(device pointer of the ticket's record, hipStream_t it is produced on) as ints"""
        d, s = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.rmcv_pipeline_record(self._h, int(ticket), C.addressof(d), C.addressof(s)))
        return d.value, s.value or 0

    # ------------------------------------------------------------------ device-side consumers
    def set_hook(self, fn):
        """fn(ticket, d_record: int, record_bytes: int, hip_stream: int) -> None | a hipEvent_t (int) recorded when the record has been
        read on another stream; called on the submitting thread right behind the enqueue of every batch's compaction"""
        if fn is None:
            self._chk(self._lib.rmcv_pipeline_set_hook(self._h, None, None))
            self._hook = None
            return

        def tramp(_user, ticket, d_record, record_bytes, hip_stream, done_event):
            try:
                ev = fn(int(ticket), int(d_record or 0), int(record_bytes), int(hip_stream or 0))
                if ev:
                    done_event[0] = ev
                return 0
            except Exception:                                    # noqa: BLE001 -- never unwind through the C frame
                import traceback
                traceback.print_exc()
                return abi.ERR_HIP
        self._hook = abi.PIPELINE_HOOK(tramp)
        self._chk(self._lib.rmcv_pipeline_set_hook(self._h, self._hook, None))

    def set_gather(self, comm_handle, root=0):
        """built-in hook: rmcv_gather of every batch's record on an rmcv_comm (rmcv_amd.dist.AbiGather._h)"""
        self._chk(self._lib.rmcv_pipeline_set_gather(self._h, comm_handle, int(root)))

    def gathered(self, ticket):
        """root: (device pointer of n_ranks x record_bytes, bytes); others: (None, bytes)"""
        d, b = C.c_void_p(), C.c_int64(0)
        self._chk(self._lib.rmcv_pipeline_gathered(self._h, int(ticket), C.addressof(d), C.addressof(b)))
        return d.value, b.value
