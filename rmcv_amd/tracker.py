"""rmcv_tracker_* (include/rmcv_abi.h): the device-resident tracker.

The tracking state of a batch of camera streams lives in HBM; one step runs behind a batch (Context.track, Pipeline.submit(...,
tracker=)) and writes the next batch's window origins on the device -- detect, track and re-window without the host.  Tracker.step_host
is the same step for one stream on the CPU (the source the kernel is compiled from), which needs no device.
"""
import ctypes as C

import numpy as np

from .abi import AIM, AIM_INPUT, ARMOUR, ATTITUDE, POINT, SERIAL_PACKET_BYTES, TRACK, RmcvError, lib, ptr

TRACKER_OVF = 1
TRACKER_MAX_CAP = 64


class TrackerConfig(C.Structure):
    """rmcv_tracker_config"""
    _fields_ = [("n_streams", C.c_int32), ("track_cap", C.c_int32), ("process_noise", C.c_double), ("measurement_noise", C.c_double),
                ("error", C.c_double), ("tick_frequency", C.c_double), ("roi_scale_w", C.c_float), ("roi_scale_h", C.c_float),
                ("frame_w", C.c_int32), ("frame_h", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32)]


def default_tracker_config(**kw):
    c = TrackerConfig()
    lib().rmcv_default_tracker_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class AimConfig(C.Structure):
    """rmcv_aim_config"""
    _fields_ = [("g", C.c_double), ("v0", C.c_double), ("height", C.c_double), ("offset_x", C.c_float), ("offset_y", C.c_float),
                ("angle_offset", C.c_double), ("latency_s", C.c_double), ("mode", C.c_int32), ("height_mode", C.c_int32), ("source", C.c_int32),
                ("pick", C.c_int32), ("lead_iterations", C.c_int32), ("max_lost", C.c_int32), ("overloads", C.c_int32), ("identity_mask", C.c_uint32)]


assert C.sizeof(AimConfig) == 80


def default_aim_config(**kw):
    c = AimConfig()
    lib().rmcv_default_aim_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class AttitudeConfig(C.Structure):
    """rmcv_attitude_config"""
    _fields_ = [("gripper2camera", C.c_double * 16), ("motor_angle_mode", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(AttitudeConfig) == 136


def default_attitude_config(**kw):
    """gripper2camera of default_pnp_config, ATT_MOTOR_KEEP; gripper2camera= takes anything that reshapes to 16 doubles"""
    c = AttitudeConfig()
    lib().rmcv_default_attitude_config(C.byref(c))
    for k, v in kw.items():
        if k == "gripper2camera":
            v = (C.c_double * 16)(*np.asarray(v, np.float64).reshape(16))
        setattr(c, k, v)
    return c


def _attitudes(attitudes, n):
    """(n, 3) (roll, pitch, yaw) radians, an ATTITUDE array, or None -> ATTITUDE[n] | None"""
    if attitudes is None:
        return None
    if isinstance(attitudes, np.ndarray) and attitudes.dtype == ATTITUDE:
        a = np.ascontiguousarray(attitudes)
    else:
        v = np.asarray(attitudes, np.float64).reshape(-1, 3)
        a = np.zeros(len(v), ATTITUDE)
        a["roll"], a["pitch"], a["yaw"] = v[:, 0], v[:, 1], v[:, 2]
    assert len(a) == n
    return a


_DEFAULTS = object()   # Tracker.set_aim(): the defaults; set_aim(None): off


def _aim_inputs(inputs, n):
    """(world2camera (4, 4), motor_angle) pairs, an AIM_INPUT array, or None -> AIM_INPUT[n] | None"""
    if inputs is None:
        return None
    if isinstance(inputs, np.ndarray) and inputs.dtype == AIM_INPUT:
        a = np.ascontiguousarray(inputs)
    else:
        a = np.zeros(len(inputs), AIM_INPUT)
        for k, (w2c, motor) in enumerate(inputs):
            a[k]["world2camera"] = np.asarray(w2c, np.float64).reshape(4, 4)
            a[k]["motor_angle"] = motor
    assert len(a) == n
    return a


class Tracker:
    def __init__(self, device=0, **config):
        """config: fields of rmcv_tracker_config (n_streams, track_cap, process_noise, measurement_noise, error, tick_frequency,
        roi_scale_w, roi_scale_h, frame_w, frame_h, win_w, win_h); win_w = 0: track only, no origins"""
        self.config = default_tracker_config(**config)
        h = C.c_void_p()
        rc = lib().rmcv_tracker_create(int(device), C.byref(self.config), C.byref(h))
        if rc != 0:
            raise RmcvError(rc, "rmcv_tracker_create failed (a bad config, or no GPU: the device tracker has no CPU path -- Tracker.step_host has)")
        self._h, self._lib, self.device = h, lib(), device
        self.n_streams, self.track_cap = self.config.n_streams, self.config.track_cap

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmcv_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RmcvError(rc, self._lib.rmcv_tracker_last_error(self._h).decode())

    def reset(self):
        """all lists empty, status cleared"""
        self._chk(self._lib.rmcv_tracker_reset(self._h))

    def set_origins(self, origins):
        """the initial requested window origins: (n_streams, 2) int32 (x, y)"""
        o = np.ascontiguousarray(origins, np.int32).reshape(-1, 2)
        assert len(o) == self.n_streams
        self._chk(self._lib.rmcv_tracker_set_origins(self._h, ptr(o)))

    def device_origins(self):
        """device pointer (int) of the requested origins: what Context.set_windows / Pipeline.submit(windows=) borrow"""
        d = C.c_void_p()
        self._chk(self._lib.rmcv_tracker_device_origins(self._h, C.byref(d)))
        return d.value

    def set_camps(self, camps, lower_bounds=None):
        """per-stream detection keys: n_streams integers each, copied into tables the tracker owns (lower_bounds None: the run's
        params.lower_bound; camps None: off).  Pipeline.submit(..., tracker=) on such a tracker detects stream f with camps[f]."""
        if camps is None:
            self._chk(self._lib.rmcv_tracker_set_camps(self._h, None, None))
            return
        c = np.ascontiguousarray(camps, np.int32).reshape(-1)
        lb = None if lower_bounds is None else np.ascontiguousarray(lower_bounds, np.int32).reshape(-1)
        assert len(c) == self.n_streams and (lb is None or len(lb) == self.n_streams)
        self._chk(self._lib.rmcv_tracker_set_camps(self._h, ptr(c), ptr(lb)))

    def device_camps(self):
        """device pointers (ints) of the tracker's camps and lower-bounds tables (n_streams int32 each): for a device-side writer, and what
        Context.set_frame_camps / Pipeline.submit(camps=) borrow"""
        d, e = C.c_void_p(), C.c_void_p()
        self._chk(self._lib.rmcv_tracker_device_camps(self._h, C.byref(d), C.byref(e)))
        return d.value, e.value

    def counts(self):
        """(n_tracking int32[n_streams], status int32[n_streams]); synchronous"""
        n, st = np.zeros(self.n_streams, np.int32), np.zeros(self.n_streams, np.int32)
        self._chk(self._lib.rmcv_tracker_counts(self._h, ptr(n), ptr(st), self.n_streams))
        return n, st

    def get(self, stream):
        """(TRACK[n], last vertices float32 (n, 4, 2), (x, y) requested origin) of one stream; synchronous"""
        tr, side = np.zeros(self.track_cap, TRACK), np.zeros((self.track_cap, 4, 2), np.float32)
        n, o = C.c_int32(0), np.zeros(1, POINT)
        self._chk(self._lib.rmcv_tracker_get(self._h, int(stream), ptr(tr), self.track_cap, C.byref(n), ptr(side), ptr(o)))
        return tr[:n.value].copy(), side[:n.value].copy(), (int(o[0]["x"]), int(o[0]["y"]))

    # ---------------------------------------------------------------- aiming
    def set_aim(self, config=_DEFAULTS, **fields):
        """aiming on: an AimConfig, or fields of rmcv_aim_config over the defaults (g, v0, height, offset_x, offset_y, angle_offset, latency_s,
        mode, height_mode, source, pick, lead_iterations, max_lost, overloads, identity_mask).  set_aim(None): off -- no aim kernel is
        launched and the records stay as they are.  Waits for the step in flight."""
        if config is None:
            assert not fields
            self._chk(self._lib.rmcv_tracker_set_aim(self._h, None))
            return None
        c = default_aim_config(**fields) if config is _DEFAULTS else config
        self._chk(self._lib.rmcv_tracker_set_aim(self._h, C.byref(c)))
        return c

    def set_aim_configs(self, configs):
        """per-stream ballistics: n_streams AimConfig, copied (rmcv_tracker_set_aim_configs); k_aim then reads stream f's own.  None: back to
        set_aim's one.  Aiming must be on.  Waits for the step in flight."""
        if configs is None:
            self._chk(self._lib.rmcv_tracker_set_aim_configs(self._h, None))
            return
        configs = list(configs)
        assert len(configs) == self.n_streams, "one AimConfig per stream"
        self._chk(self._lib.rmcv_tracker_set_aim_configs(self._h, (AimConfig * len(configs))(*configs)))

    def set_aim_inputs(self, inputs=None):
        """per stream (world2camera (4, 4), motor_angle) -- a list of pairs or an AIM_INPUT array; None: identity, 0"""
        a = _aim_inputs(inputs, self.n_streams)
        self._chk(self._lib.rmcv_tracker_set_aim_inputs(self._h, ptr(a)))

    def device_aim_inputs(self):
        """device pointer (int) of the n_streams rmcv_aim_input: a caller may write them on its own stream before a submit"""
        d = C.c_void_p()
        self._chk(self._lib.rmcv_tracker_device_aim_inputs(self._h, C.byref(d)))
        return d.value

    def device_aims(self):
        """device pointer (int) of the n_streams rmcv_aim records"""
        d = C.c_void_p()
        self._chk(self._lib.rmcv_tracker_device_aims(self._h, C.byref(d)))
        return d.value

    def aim(self, now, stream=None):
        """the aim step alone, on the lists as they are; asynchronous"""
        self._chk(self._lib.rmcv_tracker_aim(self._h, C.c_int64(int(now)), C.c_void_p(stream or 0)))

    def aims(self):
        """AIM[n_streams]; synchronous.  Zeros until the first aim step."""
        out = np.zeros(self.n_streams, AIM)
        self._chk(self._lib.rmcv_tracker_get_aims(self._h, ptr(out), self.n_streams))
        return out

    # ---------------------------------------------------------------- gimbal attitude
    def set_attitude(self, config=_DEFAULTS, **fields):
        """attitude on: an AttitudeConfig, or fields of rmcv_attitude_config over the defaults (gripper2camera, motor_angle_mode).
        set_attitude(None): off -- no kernel is launched and the tables stay as they are.  Waits for the step in flight."""
        if config is None:
            assert not fields
            self._chk(self._lib.rmcv_tracker_set_attitude(self._h, None))
            return None
        c = default_attitude_config(**fields) if config is _DEFAULTS else config
        self._chk(self._lib.rmcv_tracker_set_attitude(self._h, C.byref(c)))
        return c

    def set_stream_cameras(self, cameras):
        """per-stream hand-eye matrices for the attitude step (rmcv_tracker_set_stream_cameras): n_streams PnpConfig (their gripper2camera
        is taken), or anything that reshapes to (n_streams, 16) doubles; copied.  None: back to the config's one.  Waits for the step in
        flight.  Keep it consistent with the contexts' camera table (Context.pnp_load_cameras)."""
        if cameras is None:
            self._chk(self._lib.rmcv_tracker_set_stream_cameras(self._h, None))
            return
        if not isinstance(cameras, np.ndarray):
            cameras = [list(c.gripper2camera) if hasattr(c, "gripper2camera") else c for c in cameras]
        m = np.ascontiguousarray(np.asarray(cameras, np.float64).reshape(-1, 16))
        assert len(m) == self.n_streams, "one gripper2camera per stream"
        self._chk(self._lib.rmcv_tracker_set_stream_cameras(self._h, ptr(m)))

    def set_attitudes(self, attitudes=None):
        """per stream (roll, pitch, yaw) in radians -- (n_streams, 3) or an ATTITUDE array; None: zeros"""
        a = _attitudes(attitudes, self.n_streams)
        self._chk(self._lib.rmcv_tracker_set_attitudes(self._h, ptr(a)))

    def attitudes(self):
        """(ATTITUDE[n_streams], packet_errors int32[n_streams]); synchronous.  Zeros before first use."""
        out, err = np.zeros(self.n_streams, ATTITUDE), np.zeros(self.n_streams, np.int32)
        self._chk(self._lib.rmcv_tracker_get_attitudes(self._h, ptr(out), ptr(err), self.n_streams))
        return out, err

    def device_attitudes(self):
        """device pointer (int) of the n_streams rmcv_attitude: a device-side producer may write them on its own stream"""
        d = C.c_void_p()
        self._chk(self._lib.rmcv_tracker_device_attitudes(self._h, C.byref(d)))
        return d.value

    def aim_inputs(self):
        """AIM_INPUT[n_streams] as the device holds them; synchronous.  The defaults before first use."""
        out = np.zeros(self.n_streams, AIM_INPUT)
        self._chk(self._lib.rmcv_tracker_get_aim_inputs(self._h, ptr(out), self.n_streams))
        return out

    @staticmethod
    def attitude_host(config, packet, attitude, camp=None, packet_errors=0, aim_input=None, base2gripper=True):
        """rmcv_attitude_step_host: one stream's attitude step on the CPU (the kernel's source).  packet 24 bytes | None; attitude a
        1-element ATTITUDE array, one record of one, or (roll, pitch, yaw); camp an int | None (camp table off); aim_input a 1-element AIM_INPUT array | None
        (the defaults).  Returns (ATTITUDE record, camp | None, packet_errors, base2gripper (4, 4) | None, AIM_INPUT record)."""
        if isinstance(attitude, np.void):   # (one record of an ATTITUDE array)
            attitude = np.array([attitude], ATTITUDE)
        a = _attitudes(attitude if isinstance(attitude, np.ndarray) else [attitude], 1).copy()
        pk = None if packet is None else np.frombuffer(bytes(packet), np.uint8)
        assert pk is None or len(pk) == SERIAL_PACKET_BYTES
        cm, err = C.c_int32(0 if camp is None else int(camp)), C.c_int32(int(packet_errors))
        b = np.zeros((4, 4)) if base2gripper else None
        if aim_input is None:
            inp = np.zeros(1, AIM_INPUT)
            inp[0]["world2camera"] = np.eye(4)
        else:
            inp = np.ascontiguousarray(aim_input, AIM_INPUT).reshape(1).copy()
        rc = lib().rmcv_attitude_step_host(C.byref(config), ptr(pk), ptr(a), None if camp is None else C.byref(cm), C.byref(err), ptr(b), ptr(inp))
        if rc != 0:
            raise RmcvError(rc, "rmcv_attitude_step_host: bad argument (a config rmcv_tracker_set_attitude would refuse)")
        return a[0], (None if camp is None else cm.value), err.value, b, inp[0]

    def put(self, stream, tracks, last_vertices=None):
        """seed or restore one stream's current list: TRACK[n] (n <= track_cap), last vertices (n, 4, 2) | None: zeros; synchronous"""
        tr = np.ascontiguousarray(tracks, TRACK)
        side = None if last_vertices is None else np.ascontiguousarray(last_vertices, np.float32).reshape(-1, 4, 2)
        assert side is None or len(side) == len(tr)
        self._chk(self._lib.rmcv_tracker_put(self._h, int(stream), ptr(tr) if len(tr) else None, len(tr), ptr(side) if side is not None and len(tr) else None))

    def restore(self, stream, loop_record):
        """one stream back to what a recorder's loop record holds (rmcv_tracker_restore): list, side records, count, status, requested
        origin, camp and lower bound, aim record and input, attitude.  loop_record: a LoopRecord or its bytes.  Refused: a truncated record,
        an aim or attitude part on a tracker whose aiming / attitude is off.  Synchronous."""
        raw = np.ascontiguousarray(loop_record.raw if hasattr(loop_record, "raw") else np.frombuffer(bytes(loop_record), np.uint8))
        self._chk(self._lib.rmcv_tracker_restore(self._h, int(stream), ptr(raw)))

    @staticmethod
    def aim_host(config, tick_frequency, tracks, now, aim_input=None):
        """rmcv_aim_step_host: one stream's aim step on the CPU (the kernel's source).  tracks TRACK[n], aim_input a (world2camera,
        motor_angle) pair | None.  Returns one AIM record."""
        tr = np.ascontiguousarray(tracks, TRACK)
        a = _aim_inputs(None if aim_input is None else [aim_input], 1)
        out = np.zeros(1, AIM)
        rc = lib().rmcv_aim_step_host(C.byref(config), float(tick_frequency), ptr(tr) if len(tr) else None, len(tr), ptr(a), C.c_int64(int(now)), ptr(out))
        if rc != 0:
            raise RmcvError(rc, "rmcv_aim_step_host: bad argument (a config rmcv_tracker_set_aim would refuse, more than 64 tracks, a bad tick frequency)")
        return out[0]

    @staticmethod
    def step_host(config, tracks, last_vertices, status, origin, armours, identities=None, positions=None, eff=(0, 0), timestamp=0):
        """rmcv_tracker_step_host: one stream's step on the CPU.  tracks TRACK[n], last_vertices (n, 4, 2), armours ARMOUR[k] in window
        coordinates with effective origin `eff`, identities int32[k] | None, positions (k, 3) | None.
        Returns (tracks, last_vertices, status, (x, y) origin)."""
        cap = config.track_cap
        tr, side = np.zeros(cap, TRACK), np.zeros((cap, 4, 2), np.float32)
        n = len(tracks)
        if n:
            tr[:n] = tracks
            side[:n] = last_vertices
        a = np.ascontiguousarray(armours, ARMOUR)
        ids = None if identities is None else np.ascontiguousarray(identities, np.int32)
        pos = None if positions is None else np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        assert (ids is None or len(ids) == len(a)) and (pos is None or len(pos) == len(a))
        nt, st, o = C.c_int32(n), C.c_int32(int(status)), np.zeros(1, POINT)
        o[0] = (int(origin[0]), int(origin[1]))
        rc = lib().rmcv_tracker_step_host(C.byref(config), ptr(tr), ptr(side), C.byref(nt), C.byref(st), ptr(o), ptr(a) if len(a) else None, len(a),
                                          ptr(ids) if ids is not None and len(a) else None, ptr(pos) if pos is not None and len(a) else None,
                                          int(eff[0]), int(eff[1]), C.c_int64(int(timestamp)))
        if rc != 0:
            raise RmcvError(rc, "rmcv_tracker_step_host: bad argument")
        return tr[:nt.value].copy(), side[:nt.value].copy(), st.value, (int(o[0]["x"]), int(o[0]["y"]))
