"""The session recorder (include/rmcv_abi.h: rmcv_recorder_*, rmcv_session_*, rmcv_pack_*): the reference's
rm::debug::logger for frames that are resident in HBM.

    rec = Recorder(device=0, slots=8, max_frames=2, max_w_bytes=3 * 1280, max_h=1024)
    pipeline.set_recorder(rec, [0, 3])          # every batch packs its frames 0 and 3, losslessly, on the device
    rec.set_user(b"what logger::write calls data")
    ...                                         # submit / collect as ever
    rec.freeze(); rec.save("missed_target.rmcv")
    armours = Session("missed_target.rmcv").replay(fresh_pipeline)

pack / unpack / pack_bound are the host forms of the packed format (no device).

The closed loop (tracked submits): Recorder(track_cap=16) also keeps a LOOP RECORD per chosen frame -- the stream's tracks, aim, attitude
and setup behind the batch's step -- rec.set_trigger(TRIG_TARGET_SWITCH | TRIG_AIM_JUMP, post_batches=4, aim_jump_deg=5) makes the device
freeze the recorder by itself, and Session.replay_tracked(fresh_pipeline) runs the session through a tracker again, byte for byte.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import TRACK, LoopState, RecordEntry, RecorderConfig, RmcvError, TriggerConfig, TriggerInfo, lib, ptr


def pack_bound(w_bytes, h):
    """the largest packed size of a plane of h rows of w_bytes bytes (rmcv_pack_bound)"""
    n = lib().rmcv_pack_bound(int(w_bytes), int(h))
    if n < 0:
        raise RmcvError(int(n), "rmcv_pack_bound: w_bytes, h >= 1 and a payload below 2^31 bytes")
    return int(n)


def pack(plane, lag=1):
    """a plane (h, w_bytes) uint8 -- its rows may be strided, its bytes within a row not -- packed losslessly on the host (rmcv_pack_host)
    -> uint8[size]"""
    a = np.asarray(plane)
    assert a.dtype == np.uint8 and a.ndim == 2 and (a.shape[1] == 1 or a.strides[1] == 1) and a.strides[0] >= a.shape[1]
    h, w = a.shape
    out = np.empty(pack_bound(w, h), np.uint8)
    size = C.c_int64(0)
    rc = lib().rmcv_pack_host(a.ctypes.data_as(C.c_void_p), w, h, C.c_int64(a.strides[0]), int(lag), ptr(out), C.c_int64(out.nbytes), C.byref(size))
    if rc:
        raise RmcvError(rc, "rmcv_pack_host")
    return out[:size.value].copy()


def unpack(packed, w_bytes, h, lag=1, out=None):
    """the plane a packed frame holds (rmcv_unpack_host) -> (h, w_bytes) uint8, or written into the rows of `out` (bytes beyond w_bytes left
    alone); RmcvError(ERR_BAD_ARG) for a buffer that is not a packed frame of this geometry"""
    p = np.ascontiguousarray(packed, np.uint8).reshape(-1)
    if out is None:
        out = np.zeros((int(h), int(w_bytes)), np.uint8)
    assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] >= h and out.shape[1] >= w_bytes and (out.shape[1] == 1 or out.strides[1] == 1)
    rc = lib().rmcv_unpack_host(ptr(p) if len(p) else None, C.c_int64(len(p)), int(w_bytes), int(h), int(lag), out.ctypes.data_as(C.c_void_p),
                                C.c_int64(out.strides[0]))
    if rc:
        raise RmcvError(rc, "rmcv_unpack_host: the buffer's header, row table or size do not agree with w_bytes, h and its length")
    return out


def _frames_of(entry, packed):
    """the unpacked frames of an entry: [n_frames, h, w, 3] for BGR, [n_frames, h, w] uint8 / uint16 for a mosaic, [n_frames, h, w_bytes] otherwise"""
    e = entry
    planes = np.stack([unpack(p, e.w_bytes, e.h, e.lag) for p in packed]) if packed else np.zeros((0, e.h, e.w_bytes), np.uint8)
    if e.input_format == abi.INPUT_BGR:
        return planes.reshape(len(packed), e.h, e.w, 3)
    if e.input_format > 0 and e.sample_bits == 16:
        return planes.view("<u2").reshape(len(packed), e.h, e.w)
    return planes


def loop_bound(track_cap):
    """bytes of one loop area (rmcv_loop_bound)"""
    n = lib().rmcv_loop_bound(int(track_cap))
    if n < 0:
        raise RmcvError(abi.ERR_BAD_ARG, "rmcv_loop_bound: track_cap 0 .. 64")
    return int(n)


_FIXED = C.sizeof(LoopState)
_SLOT = TRACK.itemsize + abi.LOOP_SIDE_BYTES


class LoopRecord:
    """one loop record: .raw (uint8, the whole area), .state (a LoopState over it), .tracks (TRACK[n_tracks]) and .side (float32
    (n_tracks, 4, 2)), both views of .raw"""

    def __init__(self, raw):
        self.raw = np.array(raw, np.uint8).reshape(-1)
        assert len(self.raw) >= _FIXED
        self.state = LoopState.from_buffer(self.raw)
        n = self.state.n_tracks
        if n < 0 or _FIXED + n * _SLOT > len(self.raw):
            raise RmcvError(abi.ERR_BAD_ARG, "a loop record whose n_tracks is beyond its area")
        self.tracks = np.ndarray((n,), TRACK, self.raw, _FIXED, (_SLOT,))
        self.side = np.ndarray((n, 4, 2), np.float32, self.raw, _FIXED + TRACK.itemsize, (_SLOT, 8, 4))

    @property
    def truncated(self):
        return bool(self.state.flags & abi.LOOP_TRUNCATED)


def _leaves(ctype, base=0, prefix=""):
    """(name, offset, size) of every leaf field of a ctypes structure"""
    for name, t in ctype._fields_:
        d = getattr(ctype, name)
        if issubclass(t, C.Structure):
            yield from _leaves(t, base + d.offset, prefix + name + ".")
        else:
            yield prefix + name, base + d.offset, d.size


def loop_field_at(offset):
    """the name of the loop record's field that holds byte `offset`"""
    if offset < _FIXED:
        for name, at, size in _leaves(LoopState):
            if at <= offset < at + size:
                return name
        return "padding at %d" % offset
    j, r = divmod(offset - _FIXED, _SLOT)
    if r >= TRACK.itemsize:
        return "side[%d]" % j
    for name in TRACK.names:
        dt, at = TRACK.fields[name][:2]
        if at <= r < at + dt.itemsize:
            return "tracks[%d].%s" % (j, name)
    return "tracks[%d] padding" % j


def _raw_of(rec):
    return rec.raw if isinstance(rec, LoopRecord) else np.frombuffer(bytes(rec), np.uint8)


def loop_trigger(prev, cur, cfg=None, **fields):
    """the trigger rule on the host (rmcv_loop_trigger_host): the RMCV_TRIG_* bits `cur` raises against `prev`, before any mask.  prev / cur:
    LoopRecord, LoopState or bytes; cfg: a TriggerConfig, or its fields (frame_status_mask, aim_jump_deg; default 0, inf)"""
    if cfg is None:
        cfg = TriggerConfig(fields.get("mask", 0), fields.get("post_batches", 0), fields.get("frame_status_mask", 0), 0, fields.get("aim_jump_deg", float("inf")))
    a, b = np.ascontiguousarray(_raw_of(prev)[:_FIXED]), np.ascontiguousarray(_raw_of(cur)[:_FIXED])
    fired = C.c_uint32(0)
    rc = lib().rmcv_loop_trigger_host(ptr(a), ptr(b), C.byref(cfg), C.byref(fired))
    if rc:
        raise RmcvError(rc, "rmcv_loop_trigger_host")
    return fired.value


class _Entries:
    """what Recorder and Session share: entries, packed frames, unpacked frames"""

    def loop(self, i, k):
        """the loop record of frame k of batch i -> LoopRecord; RmcvError(ERR_BAD_ARG) when the batch has none"""
        return LoopRecord(self._loop_raw(i, k))

    def loops(self, i):
        """the loop records of batch i, [] when it has none"""
        e, _ = self.entry(i)
        return [self.loop(i, k) for k in range(e.n_frames)] if e.loop_bytes else []

    def __len__(self):
        return self.count()

    def frames(self, i):
        """the frames of batch i as they were submitted (unpacked on the host)"""
        e, _ = self.entry(i)
        return _frames_of(e, [self.frame(i, k) for k in range(e.n_frames)])


class Recorder(_Entries):
    def __init__(self, device=0, slots=0, max_frames=0, max_w_bytes=0, max_h=0, user_bytes=0, track_cap=0):
        """track_cap > 0: tracked submits also get loop records of up to track_cap tracks a chosen frame (0: none, nothing is allocated)"""
        cfg = RecorderConfig(slots, max_frames, max_w_bytes, max_h, user_bytes, track_cap)
        self.track_cap = int(track_cap)
        h = C.c_void_p()
        rc = lib().rmcv_recorder_create(int(device), C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RmcvError(rc, "rmcv_recorder_create failed (no GPU? this library has no CPU path)")
        self._h, self._lib, self.device = h, lib(), device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmcv_recorder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RmcvError(rc, self._lib.rmcv_recorder_last_error(self._h).decode())

    def set_user(self, data):
        """the user blob of the next batch recorded, and of every one after it until set again: the `data` of logger::write"""
        b = bytes(data)
        self._chk(self._lib.rmcv_recorder_set_user(self._h, b, len(b)))

    def record(self, data_ptr, w_bytes, h, lag=1, frames=None, n=None, stride=None, pitch=None, stream=0):
        """stand-alone: pack frames (indices; None: 0 .. n - 1) of device planes into the next slot, asynchronously on `stream`"""
        fr = None if frames is None else np.ascontiguousarray(frames, np.int32).reshape(-1)
        n = len(fr) if fr is not None else int(n)
        stride = stride or w_bytes
        self._chk(self._lib.rmcv_recorder_record(self._h, data_ptr, int(w_bytes), int(h), int(stride), pitch or stride * h, int(lag), ptr(fr), n, stream or None))

    def freeze(self):
        """from here on nothing is recorded and nothing is overwritten"""
        self._chk(self._lib.rmcv_recorder_freeze(self._h))

    def resume(self):
        self._chk(self._lib.rmcv_recorder_resume(self._h))

    def count(self):
        n = C.c_int32(0)
        self._chk(self._lib.rmcv_recorder_count(self._h, C.byref(n)))
        return n.value

    def entry(self, i):
        """(RecordEntry, user blob) of batch i, 0 the oldest"""
        e, cap = RecordEntry(), 1 << 20
        user = C.create_string_buffer(cap)
        self._chk(self._lib.rmcv_recorder_entry(self._h, int(i), C.byref(e), user, cap))
        return e, user.raw[:e.user_bytes]

    def frame(self, i, k):
        """the packed bytes of frame k of batch i, downloaded"""
        d, size = C.c_void_p(), C.c_int64(0)
        self._chk(self._lib.rmcv_recorder_device_frame(self._h, int(i), int(k), C.byref(d), C.byref(size)))
        out = np.empty(size.value, np.uint8)
        self._chk(self._lib.rmcv_recorder_frame(self._h, int(i), int(k), ptr(out), C.c_int64(out.nbytes), C.byref(size)))
        return out

    def device_frame(self, i, k):
        """(device pointer, size) of the packed frame k of batch i"""
        d, size = C.c_void_p(), C.c_int64(0)
        self._chk(self._lib.rmcv_recorder_device_frame(self._h, int(i), int(k), C.byref(d), C.byref(size)))
        return d.value, size.value

    def save(self, path):
        self._chk(self._lib.rmcv_recorder_save(self._h, str(path).encode()))

    def _loop_raw(self, i, k):
        out = np.zeros(loop_bound(self.track_cap), np.uint8)
        size = C.c_int64(0)
        self._chk(self._lib.rmcv_recorder_loop(self._h, int(i), int(k), ptr(out), C.c_int64(out.nbytes), C.byref(size)))
        return out[:size.value]

    def set_trigger(self, mask, post_batches=0, frame_status_mask=0, aim_jump_deg=float("inf")):
        """arm the device-side trigger (rmcv_recorder_set_trigger): a loop record whose fired & mask is non-zero takes the latch, and the
        recorder freezes by itself post_batches batches after a submit has noticed.  mask None or 0: off.  The pipeline refuses a recorder
        armed on a ring smaller than depth + post_batches."""
        if not mask:
            self._chk(self._lib.rmcv_recorder_set_trigger(self._h, None))
            return
        cfg = TriggerConfig(int(mask), int(post_batches), int(frame_status_mask), 0, float(aim_jump_deg))
        self._chk(self._lib.rmcv_recorder_set_trigger(self._h, C.byref(cfg)))

    def trigger(self):
        """the latch (rmcv_recorder_trigger) -> TriggerInfo: fired, mask, sequence, k, stream, noticed, batches_since"""
        info = TriggerInfo()
        self._chk(self._lib.rmcv_recorder_trigger(self._h, C.byref(info)))
        return info


class Session(_Entries):
    """a saved session, host-side: entries, packed and unpacked frames, and replay"""

    def __init__(self, path):
        h = C.c_void_p()
        rc = lib().rmcv_session_open(str(path).encode(), C.byref(h))
        if rc != 0:
            raise RmcvError(rc, "rmcv_session_open: %s is missing, truncated or inconsistent" % path)
        self._h, self._lib = h, lib()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmcv_session_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self):
        n = C.c_int32(0)
        rc = self._lib.rmcv_session_count(self._h, C.byref(n))
        if rc:
            raise RmcvError(rc, "rmcv_session_count")
        return n.value

    def entry(self, i):
        e, cap = RecordEntry(), 1 << 20
        user = C.create_string_buffer(cap)
        rc = self._lib.rmcv_session_entry(self._h, int(i), C.byref(e), user, cap)
        if rc:
            raise RmcvError(rc, "rmcv_session_entry: no such entry")
        return e, user.raw[:e.user_bytes]

    def frame(self, i, k):
        size = C.c_int64(0)
        rc = self._lib.rmcv_session_frame(self._h, int(i), int(k), None, C.c_int64(0), C.byref(size))
        if rc not in (0, abi.ERR_CAPACITY):
            raise RmcvError(rc, "rmcv_session_frame: no such frame")
        out = np.empty(size.value, np.uint8)
        rc = self._lib.rmcv_session_frame(self._h, int(i), int(k), ptr(out), C.c_int64(out.nbytes), C.byref(size))
        if rc:
            raise RmcvError(rc, "rmcv_session_frame")
        return out

    def _loop_raw(self, i, k):
        size = C.c_int64(0)
        rc = self._lib.rmcv_session_loop(self._h, int(i), int(k), None, C.c_int64(0), C.byref(size))
        if rc not in (0, abi.ERR_CAPACITY):
            raise RmcvError(rc, "rmcv_session_loop: entry %d has no loop record %d" % (i, k))
        out = np.zeros(size.value, np.uint8)
        rc = self._lib.rmcv_session_loop(self._h, int(i), int(k), ptr(out), C.c_int64(out.nbytes), C.byref(size))
        if rc:
            raise RmcvError(rc, "rmcv_session_loop")
        return out

    def replay_tracked(self, pipeline, verify=True):
        """run the session through a tracker again.  Entry 0 is the SEED: a tracker of its n_frames streams is built from its loop records'
        setup and restored from them (its own step is not replayed); entries 1 .. n - 1 are resubmitted -- unpacked frames, the entry's
        parameters, stages and timestamp, the recorded packets -- through submit(..., tracker=), window origins from the TRACKER as in the
        live run.  Each batch's loop records are taken by a recorder of the replay's own on `pipeline` (it replaces any other) and
        re-labelled with the recorded batch's names -- stream, sequence, tracker_config.n_streams, the trigger's two inputs; fired / has_prev from the
        host rule against the replay's previous record where the recorded one had a predecessor -- everything else is what the replay computed.
        Returns [(loops, armours)] per entry: ([LoopRecord], (ARMOUR[], frame_offs) | None for the seed).  verify: raises RmcvError naming
        entry, frame and field at the first byte that differs from the recorded record, and when the effective origins differ from the
        entry's.  The caller supplies what the file does not hold: a pipeline with the recorded input format, the same model loaded, the same
        camera table loaded (a record's cam_eff is an index into it).  Refused: entries that are not consecutive sequences, a truncated
        record, entries without loop records."""
        import torch
        from .tracker import AimConfig, AttitudeConfig, Tracker, TrackerConfig
        dev = "cuda:%d" % pipeline.device
        n_e = self.count()
        if n_e < 1:
            raise RmcvError(abi.ERR_BAD_ARG, "an empty session")
        entries = [self.entry(i)[0] for i in range(n_e)]
        for i, e in enumerate(entries):
            if not e.loop_bytes:
                raise RmcvError(abi.ERR_BAD_ARG, "entry %d has no loop records (an untracked submit, or a recorder with track_cap == 0)" % i)
            if i and (e.sequence != entries[i - 1].sequence + 1 or e.n_frames != entries[0].n_frames or list(e.frames[:e.n_frames]) != list(entries[0].frames[:e.n_frames])):
                raise RmcvError(abi.ERR_BAD_ARG, "entries %d and %d are not consecutive sequences of the same chosen frames" % (i - 1, i))
            if e.input_format != pipeline.input_format or (e.input_format and e.sample_bits != pipeline.sample_bits):
                raise RmcvError(abi.ERR_BAD_ARG, "entry %d was recorded with another input format than the pipeline's" % i)
        recorded = [self.loops(i) for i in range(n_e)]
        for i, recs in enumerate(recorded):
            for k, r in enumerate(recs):
                if r.truncated:
                    raise RmcvError(abi.ERR_BAD_ARG, "entry %d frame %d: the loop record is truncated (RMCV_LOOP_TRUNCATED): it does not hold the stream's whole list" % (i, k))
        e0, seed = entries[0], recorded[0]
        n = e0.n_frames
        L = lib()
        tc = TrackerConfig()
        if L.rmcv_tracker_config_from_loop(ptr(seed[0].raw), C.byref(tc)):
            raise RmcvError(abi.ERR_BAD_ARG, "entry 0: rmcv_tracker_config_from_loop refused the record")
        fields = {name: getattr(tc, name) for name, _ in TrackerConfig._fields_}
        fields["n_streams"] = n
        trk = Tracker(device=pipeline.device, **fields)
        s0 = seed[0].state
        if s0.has_aim:
            cfgs = [AimConfig.from_buffer_copy(bytes(r.state.aim_config)) for r in seed]
            trk.set_aim(cfgs[0])
            if any(bytes(c) != bytes(cfgs[0]) for c in cfgs):
                trk.set_aim_configs(cfgs)
        if s0.has_attitude:
            trk.set_attitude(AttitudeConfig.from_buffer_copy(bytes(s0.attitude_config)))
            g2c = [list(r.state.gripper2camera) for r in seed]
            if any(g != list(s0.attitude_config.gripper2camera) for g in g2c):
                trk.set_stream_cameras(np.array(g2c))
        for k, r in enumerate(seed):
            trk.restore(k, r)
        keep_cams = None
        if s0.has_cameras:
            keep_cams = torch.from_numpy(np.array([r.state.cam_eff for r in seed], np.int32)).to(dev)
            pipeline.set_frame_cameras(keep_cams.data_ptr(), n, keepalive=keep_cams)
        cap = (e0.loop_bytes - _FIXED) // _SLOT
        rec = Recorder(device=pipeline.device, slots=2, max_frames=n, max_w_bytes=e0.w_bytes, max_h=e0.h, track_cap=cap)
        out = [(seed, None)]
        try:
            pipeline.set_recorder(rec, list(range(n)))
            prev = seed
            for i in range(1, n_e):
                e = entries[i]
                fr = torch.from_numpy(np.ascontiguousarray(self.frames(i)).view(np.uint8).reshape(n, e.h, e.w_bytes)).to(dev)
                keep, packets = [fr], None
                if recorded[i][0].state.has_packet:
                    pk = torch.from_numpy(np.array([list(r.state.packet) for r in recorded[i]], np.uint8)).to(dev)
                    keep.append(pk)
                    packets = pk.data_ptr()
                params = abi.Params.from_buffer_copy(bytes(e.params))
                t = pipeline.submit(fr.data_ptr(), n, e.h, e.w, params, e.stages, stride=e.w_bytes, keepalive=keep, tracker=trk, timestamp=e.timestamp, packets=packets)
                arm = pipeline.collect(t)
                got = rec.loops(rec.count() - 1)
                for k, g in enumerate(got):   # the recorded batch's names; the rule on the replay's own records
                    want = recorded[i][k].state
                    g.state.stream, g.state.sequence, g.state.tracker_config.n_streams = want.stream, want.sequence, want.tracker_config.n_streams
                    g.state.has_prev = want.has_prev
                    g.state.trig_frame_status_mask, g.state.trig_aim_jump_deg = want.trig_frame_status_mask, want.trig_aim_jump_deg
                    g.state.fired = loop_trigger(prev[k], g, frame_status_mask=want.trig_frame_status_mask, aim_jump_deg=want.trig_aim_jump_deg) if want.has_prev else 0
                out.append((got, arm))
                if verify:
                    for k, g in enumerate(got):
                        w = recorded[i][k]
                        if e.has_origins and tuple(g.state.origin_eff) != tuple(e.origins[k]):
                            raise RmcvError(abi.ERR_BAD_ARG, "entry %d frame %d: the replay read its window at %s, the recorded batch at %s" % (
                                i, k, tuple(g.state.origin_eff), tuple(e.origins[k])))
                        diff = np.nonzero(g.raw != w.raw)[0]
                        if len(diff):
                            raise RmcvError(abi.ERR_BAD_ARG, "entry %d frame %d: the replay differs from the recorded loop record in field %s (byte %d)" % (
                                i, k, loop_field_at(int(diff[0])), int(diff[0])))
                prev = got
        finally:
            pipeline.set_recorder(None, [])
            if keep_cams is not None:
                pipeline.set_frame_cameras(None)
            rec.close()
            trk.close()
        return out

    def replay(self, pipeline):
        """resubmit every entry's recorded frames to `pipeline` -- a batch of the entry's n_frames frames with its own parameters, stages,
        geometry, window and camps -- and return [(ARMOUR[], frame_offs)] per entry.  The pipeline's input format must be the entries'.
        (A tracked submit replays here as a plain batch at its recorded effective origins; replay_tracked runs it through a tracker.)"""
        import torch
        dev = "cuda:%d" % pipeline.device
        out = []
        for i in range(self.count()):
            e, _ = self.entry(i)
            if e.input_format < 0:
                raise RmcvError(abi.ERR_BAD_ARG, "entry %d is a stand-alone record of byte planes: nothing to detect in" % i)
            if e.input_format != pipeline.input_format or (e.input_format and e.sample_bits != pipeline.sample_bits):
                raise RmcvError(abi.ERR_BAD_ARG, "entry %d was recorded with another input format than the pipeline's" % i)
            n = e.n_frames
            fr = torch.from_numpy(np.ascontiguousarray(self.frames(i)).view(np.uint8).reshape(n, e.h, e.w_bytes)).to(dev)
            keep, windows, camps = [fr], None, None
            if e.has_origins:
                org = torch.from_numpy(np.array([[e.origins[k][0], e.origins[k][1]] for k in range(n)], np.int32)).to(dev)
                keep.append(org)
                windows = (org.data_ptr(), e.win_w, e.win_h)
            if e.has_keys:
                raw = torch.from_numpy(np.array([e.camps[k] for k in range(n)], np.int32)).to(dev)
                lbs = torch.from_numpy(np.array([0 if e.keys[k][3] else e.keys[k][2] for k in range(n)], np.int32)).to(dev)
                keep += [raw, lbs]
                camps = (raw.data_ptr(), lbs.data_ptr())
            params = abi.Params.from_buffer_copy(bytes(e.params))
            t = pipeline.submit(fr.data_ptr(), n, e.h, e.w, params, e.stages, stride=e.w_bytes, keepalive=keep, windows=windows, camps=camps)
            out.append(pipeline.collect(t))
        return out


__all__ = ["Recorder", "Session", "LoopRecord", "loop_trigger", "loop_bound", "loop_field_at", "pack", "unpack", "pack_bound"]
