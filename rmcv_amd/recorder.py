"""The session recorder (include/rmcv_abi.h: rmcv_recorder_*, rmcv_session_*, rmcv_pack_*): the reference's
rm::debug::logger for frames that are resident in HBM.

    rec = Recorder(device=0, slots=8, max_frames=2, max_w_bytes=3 * 1280, max_h=1024)
    pipeline.set_recorder(rec, [0, 3])          # every batch packs its frames 0 and 3, losslessly, on the device
    rec.set_user(b"what logger::write calls data")
    ...                                         # submit / collect as ever
    rec.freeze(); rec.save("missed_target.rmcv")
    armours = Session("missed_target.rmcv").replay(fresh_pipeline)

pack / unpack / pack_bound are the host forms of the packed format (no device).
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import RecordEntry, RecorderConfig, RmcvError, lib, ptr


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


class _Entries:
    """what Recorder and Session share: entries, packed frames, unpacked frames"""

    def __len__(self):
        return self.count()

    def frames(self, i):
        """the frames of batch i as they were submitted (unpacked on the host)"""
        e, _ = self.entry(i)
        return _frames_of(e, [self.frame(i, k) for k in range(e.n_frames)])


class Recorder(_Entries):
    def __init__(self, device=0, slots=0, max_frames=0, max_w_bytes=0, max_h=0, user_bytes=0):
        cfg = RecorderConfig(slots, max_frames, max_w_bytes, max_h, user_bytes, 0)
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

    def replay(self, pipeline):
        """resubmit every entry's recorded frames to `pipeline` -- a batch of the entry's n_frames frames with its own parameters, stages,
        geometry, window and camps -- and return [(ARMOUR[], frame_offs)] per entry.  The pipeline's input format must be the entries'.
        (A tracked submit's frames and timestamp are recorded; its tracker state is not: it replays as a plain batch.)"""
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


__all__ = ["Recorder", "Session", "pack", "unpack", "pack_bound"]
