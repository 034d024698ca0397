"""Host-side mirror of the reference's detection interface over the C-ABI.

Same names, argument meaning and result order as the reference's
  rm::extract_color      include/imgproc.h:29      (src/imgproc.cpp:50-75)
  rm::filter_lightblobs  include/objdetect.h:47-49 (src/objdetect.cpp:55-87)
  rm::filter_armours     include/objdetect.h:70-71 (src/objdetect.cpp:114-166)
plus the batch entry point the north star adds (independent frames resident in HBM).
Every call runs on the GPU through librmcv_hip.so; nothing here computes on the CPU.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import delta_height, distance, projectile_angle, rigid_inverse, solve_gea  # noqa: F401  (rm::ProjectileAngle / SolveGEA / DeltaHeight / Distance: host-side)
from .abi import (ARMOUR, CAMP_BLUE, LIGHTBLOB, MORPH_CLOSE, POINT, RRECT, STAGE_ALL, LegacyParams, Limits, Params, PnpConfig, RmcvError, default_pnp_config,
                  default_params, lib, ptr)


class Context:
    """One rmcv_ctx: a GPU, its HBM work buffers and a stream.  Single-owner, like the reference's
    process_thread (executable/main.cpp:55)."""

    def __init__(self, device=0, **limits):
        lim = Limits()
        lib().rmcv_default_limits(C.byref(lim))
        for k, v in limits.items():
            setattr(lim, k, v)
        self.limits = lim
        h = C.c_void_p()
        rc = lib().rmcv_ctx_create(int(device), C.byref(lim), C.byref(h))
        if rc != 0:
            raise RmcvError(rc, "rmcv_ctx_create failed (no GPU? this library has no CPU path)")
        self._h = h
        self._made_by = lib()                                     # (a process can hold two builds: bench.py's RMCV_BENCH_AB=lib:...)
        self.device = device
        self._frames_ref = None
        self.input_format = abi.INPUT_BGR
        self.sample_bits = 8

    @classmethod
    def borrowed(cls, handle, limits, device=0):
        """a view of a context somebody else owns (a slot of a Pipeline): the same methods, no destroy"""
        self = cls.__new__(cls)
        self.limits, self._h, self._made_by, self.device, self._frames_ref, self._borrowed = limits, C.c_void_p(handle), lib(), device, None, True
        self.input_format = abi.INPUT_BGR
        self.sample_bits = 8
        return self

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._made_by.rmcv_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RmcvError(rc, lib().rmcv_last_error(self._h).decode())

    # ---------------------------------------------------------------- single frame
    def extract_color(self, image, target=CAMP_BLUE, lower_bound=80, morph=MORPH_CLOSE):
        """rm::extract_color -> (contours, binary); contours = list of (n,2) int32 arrays in
        cv::findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) order"""
        pts, offs, binary = self.extract_color_csr(image, target, lower_bound, morph)
        xy = np.stack([pts["x"], pts["y"]], axis=1) if len(pts) else np.zeros((0, 2), np.int32)
        return [xy[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], binary

    def _frame(self, image):
        """(image, h, w, row bytes) of one host frame: (h, w, 3) BGR, or (h, w) under a Bayer input format (uint16 with 16-bit samples)"""
        if self.input_format:
            image = np.ascontiguousarray(image, self._sample_dtype())
            assert image.ndim == 2, "a Bayer input format takes (h, w) mosaics"
            h, w = image.shape
            return image, h, w, w * image.itemsize
        image = np.ascontiguousarray(image, np.uint8)
        h, w, ch = image.shape
        assert ch == 3
        return image, h, w, 3 * w

    def set_input_format(self, fmt):
        """RMCV_OPT_INPUT_FORMAT: abi.INPUT_BGR (0) or one of abi.BAYER_PATTERNS -- what the frames handed in from now on hold"""
        self.set_option(abi.OPT_INPUT_FORMAT, fmt)
        self.input_format = int(fmt)

    def _sample_dtype(self):
        return np.dtype("<u2") if self.sample_bits == 16 else np.dtype(np.uint8)

    def set_input_layout(self, sample_bits=8, valid_bit=0, mirror=False, flip=False):
        """the Bayer frame as the sensor delivers it (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT): 8- or 16-bit samples, the
        first of the 8 bits of a 16-bit sample that are the pixel (0 .. 4), mirrored left-right and / or flipped top-bottom.  Every
        result is that of the oriented 8-bit mosaic; the pattern of set_input_format stays that of the buffer as delivered."""
        self.set_option(abi.OPT_INPUT_SAMPLE_BITS, sample_bits)
        self.sample_bits = int(sample_bits)
        self.set_option(abi.OPT_INPUT_VALID_BIT, valid_bit)
        self.set_option(abi.OPT_INPUT_ORIENT, (abi.ORIENT_MIRROR if mirror else 0) | (abi.ORIENT_FLIP if flip else 0))

    def demosaic_raw(self, raw, pattern, valid_bit=0, mirror=False, flip=False):
        """D(T(r)) of one delivered (h, w) uint8 or uint16 buffer as the (h, w, 3) BGR frame of the oriented mosaic (rmcv_demosaic_raw)"""
        raw = np.asarray(raw)
        bits = 16 if raw.dtype.itemsize == 2 else 8
        raw = np.ascontiguousarray(raw, np.dtype("<u2") if bits == 16 else np.uint8)
        h, w = raw.shape
        out = np.empty((h, w, 3), np.uint8)
        orient = (abi.ORIENT_MIRROR if mirror else 0) | (abi.ORIENT_FLIP if flip else 0)
        self._chk(lib().rmcv_demosaic_raw(self._h, ptr(raw), w, h, w * raw.itemsize, int(pattern), bits, int(valid_bit), orient, ptr(out), 3 * w))
        return out

    def demosaic(self, raw, pattern):
        """D(m) of one (h, w) uint8 mosaic as an (h, w, 3) BGR frame (rmcv_demosaic: the library's demosaic, on the GPU)"""
        raw = np.ascontiguousarray(raw, np.uint8)
        h, w = raw.shape
        out = np.empty((h, w, 3), np.uint8)
        self._chk(lib().rmcv_demosaic(self._h, ptr(raw), w, h, w, int(pattern), ptr(out), 3 * w))
        return out

    # ---------------------------------------------------------------- exposure-adaptive detection (rm::CalcGamma / rm::AutoEnhance)
    def set_enhance(self, on=True, max_gain=None, min_gain=None):
        """RMCV_OPT_ENHANCE: frames handed in from now on are read through their rm::AutoEnhance table (gains: the reference's 100, 50
        unless given); every result is that of the enhanced frame, which is never written"""
        if max_gain is not None or min_gain is not None:
            self._chk(lib().rmcv_ctx_set_enhance_gains(self._h, C.c_float(abi.ENHANCE_MAX_GAIN if max_gain is None else max_gain),
                                                       C.c_float(abi.ENHANCE_MIN_GAIN if min_gain is None else min_gain)))
        self.set_option(abi.OPT_ENHANCE, 1 if on else 0)

    def get_enhance(self):
        """(RMCV_OPT_ENHANCE, max_gain, min_gain) as the context is set"""
        on, hi, lo = C.c_int32(0), C.c_float(0), C.c_float(0)
        self._chk(lib().rmcv_ctx_get_enhance(self._h, C.byref(on), C.byref(hi), C.byref(lo)))
        return bool(on.value), hi.value, lo.value

    def calc_gamma(self, image, gamma, inplace=False):
        """rm::CalcGamma of a uint8 image of any shape whose last axes are contiguous rows ((h, w), (h, w, c)): the table of `gamma`
        applied to every byte, on the GPU"""
        img = image if inplace else np.ascontiguousarray(image, np.uint8)
        assert img.dtype == np.uint8 and img.flags.c_contiguous and img.ndim >= 2
        rows, rowb = img.shape[0], img.strides[0]
        out = img if inplace else np.empty_like(img)
        self._chk(lib().rmcv_calc_gamma(self._h, ptr(img), rowb, rows, rowb, C.c_float(gamma), ptr(out), rowb))
        return out

    def auto_enhance(self, image, max_gain=abi.ENHANCE_MAX_GAIN, min_gain=abi.ENHANCE_MIN_GAIN, inplace=False):
        """rm::AutoEnhance of one (h, w, 3) BGR frame -> (enhanced frame, gamma); sums, table and mapping on the GPU"""
        img = image if inplace else np.ascontiguousarray(image, np.uint8)
        assert img.dtype == np.uint8 and img.flags.c_contiguous and img.ndim == 3 and img.shape[2] == 3
        h, w, _ = img.shape
        out = img if inplace else np.empty_like(img)
        g = C.c_float(0)
        self._chk(lib().rmcv_auto_enhance(self._h, ptr(img), w, h, 3 * w, C.c_float(max_gain), C.c_float(min_gain), ptr(out), 3 * w, C.byref(g)))
        return out, np.float32(g.value)

    def gammas(self):
        """the gamma each frame of the last batch run (or the last extract_color, as frame 0) was read with"""
        n = self.shape[0]
        out = np.empty(n, np.float32)
        self._chk(lib().rmcv_batch_get_gammas(self._h, ptr(out), n))
        return out

    def extract_color_csr(self, image, target=CAMP_BLUE, lower_bound=80, morph=MORPH_CLOSE):
        image, h, w, rowb = self._frame(image)
        binary = np.empty((h, w), np.uint8)
        cap_p, cap_c = self.limits.max_points, self.limits.max_contours
        pts = np.empty(cap_p, POINT)
        offs = np.empty(cap_c + 1, np.int32)
        nc, npnt = C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_extract_color(self._h, ptr(image), w, h, rowb, int(target), int(lower_bound), int(morph),
                                           ptr(binary), ptr(pts), cap_p, ptr(offs), cap_c, C.byref(nc), C.byref(npnt)))
        self.shape = (1, h, w)
        return pts[:npnt.value].copy(), offs[:nc.value + 1].copy(), binary

    def filter_lightblobs(self, pts, offs, tilt_max=70.0, ratio_range=(1.5, 80.0), area_range=(10.0, 99999.0),
                          enemy=CAMP_BLUE):
        """rm::filter_lightblobs on CSR contours -> (positive LIGHTBLOB[], source contour index[], negative contour index[])"""
        pts = np.ascontiguousarray(pts, POINT)
        offs = np.ascontiguousarray(offs, np.int32)
        n = len(offs) - 1
        cap = self.limits.max_blobs
        blobs = np.empty(cap, LIGHTBLOB)
        src = np.empty(cap, np.int32)
        neg = np.empty(max(n, 1), np.int32)
        nb, nn = C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_filter_lightblobs(self._h, ptr(pts), ptr(offs), n, C.c_float(tilt_max),
                                               C.c_float(ratio_range[0]), C.c_float(ratio_range[1]),
                                               C.c_double(area_range[0]), C.c_double(area_range[1]), int(enemy),
                                               ptr(blobs), cap, C.byref(nb), ptr(src), ptr(neg), C.byref(nn)))
        return blobs[:nb.value].copy(), src[:nb.value].copy(), neg[:nn.value].copy()

    def filter_armours(self, lightblobs, angle_difference_max=12.0, shear_max=22.0, lenght_ratio_max=0.4, enemy=CAMP_BLUE):
        """rm::filter_armours -> ARMOUR[] in (i,j) lexicographic order"""
        lightblobs = np.ascontiguousarray(lightblobs, LIGHTBLOB)
        cap = self.limits.max_armours
        out = np.empty(cap, ARMOUR)
        na = C.c_int32(0)
        self._chk(lib().rmcv_filter_armours(self._h, ptr(lightblobs), len(lightblobs), C.c_float(angle_difference_max),
                                            C.c_float(shear_max), C.c_float(lenght_ratio_max), int(enemy), ptr(out), cap,
                                            C.byref(na)))
        return out[:na.value].copy()

    def fit_ellipse(self, pts):
        """cv::fitEllipseDirect of one contour (stage-wise parity hook)"""
        pts = np.ascontiguousarray(pts, POINT)
        out = np.zeros(1, RRECT)
        self._chk(lib().rmcv_fit_ellipse(self._h, ptr(pts), len(pts), ptr(out)))
        return out[0]

    def set_option(self, option, value):
        """tuning knobs (abi.OPT_SPARSE_WAVES: 8 = latency of a lone batch, 4 = throughput with several batches in flight)"""
        self._chk(lib().rmcv_ctx_set_option(self._h, int(option), int(value)))

    def check_guards(self):
        """(number of damaged guard zones around the context's device buffers, description of the first) -- 0 in a correct build"""
        n = C.c_int32(-1)
        self._chk(lib().rmcv_ctx_check_guards(self._h, C.byref(n)))
        return n.value, lib().rmcv_last_error(self._h).decode()

    # ---------------------------------------------------------------- armour pose (src/mobility.cpp:166-190, main.cpp:183-192)
    def pnp_load(self, cfg=None):
        """camera matrix, distortion, gripper->camera transform, square size (defaults: the reference's main.cpp literals)"""
        self._pnp = cfg or default_pnp_config()
        self._chk(lib().rmcv_pnp_load(self._h, C.byref(self._pnp)))

    def pnp_load_cameras(self, cfgs):
        """the context's camera table: a sequence of PnpConfig, one per physical camera of the fleet (rmcv_pnp_load_cameras).  Entry 0 is
        also locate_armours' camera; set_frame_cameras picks an entry per frame.  Switches per-frame selection off."""
        cfgs = list(cfgs)
        arr = (PnpConfig * max(len(cfgs), 1))(*cfgs)
        self._chk(lib().rmcv_pnp_load_cameras(self._h, arr, len(cfgs)))
        self._pnp = arr

    def set_frame_cameras(self, idx, keepalive=None):
        """every frame bound is located through its own entry of the camera table: n integers on the host (each inside the table, else
        RmcvError and nothing changes), or an int = device pointer to n int32 (borrowed; read again by every run with STAGE_POSE; any
        values: frame_cameras() shows what the kernel used).  None: camera 0 for every frame (a new binding returns to that too)."""
        if idx is None:
            self._chk(lib().rmcv_batch_set_frame_cameras(self._h, None))
            return
        if isinstance(idx, (int, np.integer)):
            self._cams_ref = keepalive
            self._chk(lib().rmcv_batch_set_device_frame_cameras(self._h, C.c_void_p(int(idx))))
            return
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        assert len(i) == self.shape[0], "one camera index per frame bound"
        self._chk(lib().rmcv_batch_set_frame_cameras(self._h, ptr(i)))

    def frame_cameras(self):
        """the effective camera index of every frame in the last run with STAGE_POSE, int32 (n,); zeros without selection"""
        out = np.zeros(self.shape[0], np.int32)
        self._chk(lib().rmcv_batch_get_frame_cameras(self._h, ptr(out), len(out)))
        return out

    frame_camera = staticmethod(abi.frame_camera)

    def locate_armours(self, armours, base2gripper=None):
        """per armour: rm::solve_PnP on its vertices + the world transform; returns (rvecs, tvecs, positions), each [n, 3]"""
        arm = np.ascontiguousarray(armours, ARMOUR)
        n = len(arm)
        r, t, p = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
        b = None if base2gripper is None else np.ascontiguousarray(base2gripper, np.float64).reshape(16)
        self._chk(lib().rmcv_locate_armours(self._h, ptr(arm), n, ptr(b) if b is not None else None, ptr(r), ptr(t), ptr(p)))
        return r[:n], t[:n], p[:n]

    def set_base2gripper(self, mats):
        """one row-major 4x4 per frame of the batch (h_base2gripper, main.cpp:170)"""
        m = np.ascontiguousarray(mats, np.float64).reshape(-1, 16)
        self._chk(lib().rmcv_batch_set_base2gripper(self._h, ptr(m), len(m)))

    def base2gripper(self):
        """(n_frames, 4, 4): the matrices the bound batch's STAGE_POSE reads -- the attitude step's (Context.attitude) or set_base2gripper's;
        synchronous"""
        out = np.zeros((self.shape[0], 4, 4))
        self._chk(lib().rmcv_batch_get_base2gripper(self._h, ptr(out), len(out)))
        return out

    def attitude(self, tracker, packets=None, stream=None):
        """the attitude step of a tracker with set_attitude, enqueued in front of run() for the bound batch (rmcv_batch_attitude): frame f is
        stream f.  packets: device pointer to n_streams x 24 bytes (keep them alive until the step has run) | None: the tracker's attitude
        table as it stands.  Asynchronous; never synchronises."""
        self._chk(lib().rmcv_batch_attitude(self._h, tracker._h, C.c_void_p(int(packets)) if packets else None, C.c_void_p(stream or 0)))

    def poses(self):
        """(rvecs, tvecs, positions) of all armours of the batch in the order of armours()"""
        cap = self.shape[0] * self.limits.max_armours
        r, t, p = np.zeros((cap, 3)), np.zeros((cap, 3)), np.zeros((cap, 3))
        tot = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_poses(self._h, ptr(r), ptr(t), ptr(p), cap, C.byref(tot)))
        return r[:tot.value].copy(), t[:tot.value].copy(), p[:tot.value].copy()

    # ---------------------------------------------------------------- legacy matcher (src/objdetect.cpp:9-53, 89-112)
    def min_area_rect(self, pts):
        """cv::minAreaRect of one contour (stage-wise parity hook)"""
        pts = np.ascontiguousarray(pts, POINT)
        out = np.zeros(1, RRECT)
        self._chk(lib().rmcv_min_area_rect(self._h, ptr(pts), len(pts), ptr(out)))
        return out[0]

    def match_lightblob(self, contour, min_ratio, max_ratio, tilt_angle, min_area, max_area, fit_ellipse=True):
        """rm::MatchLightBlob: returns (matched, box)"""
        pts = np.ascontiguousarray(contour, POINT)
        lp = LegacyParams(min_ratio, max_ratio, tilt_angle, min_area, max_area, int(bool(fit_ellipse)))
        out = np.zeros(1, RRECT)
        m = C.c_int32(0)
        self._chk(lib().rmcv_match_lightblob(self._h, ptr(pts), len(pts), C.byref(lp), ptr(out), C.byref(m)))
        return bool(m.value), out[0]

    def find_lightblobs(self, pts, offs, min_ratio, max_ratio, tilt_angle, min_area, max_area, source, fit_ellipse=True):
        """rm::FindLightBlobs on CSR contours: returns (blobs, blob_src, boxes); camps are voted from `source` (h, w, 3 BGR)"""
        source = np.ascontiguousarray(source, np.uint8)
        h, w, ch = source.shape
        assert ch == 3
        pts = np.ascontiguousarray(pts, POINT)
        offs = np.ascontiguousarray(offs, np.int32)
        n = len(offs) - 1
        lp = LegacyParams(min_ratio, max_ratio, tilt_angle, min_area, max_area, int(bool(fit_ellipse)))
        cap = max(n, 1)
        blobs, src, boxes = np.zeros(cap, LIGHTBLOB), np.zeros(cap, np.int32), np.zeros(cap, RRECT)
        nb = C.c_int32(0)
        self._chk(lib().rmcv_find_lightblobs(self._h, ptr(source), w, h, 3 * w, ptr(pts), ptr(offs), n, C.byref(lp), ptr(blobs), cap,
                                             C.byref(nb), ptr(src), ptr(boxes)))
        self.shape = (1, h, w)
        return blobs[:nb.value].copy(), src[:nb.value].copy(), boxes[:nb.value].copy()

    @staticmethod
    def lightblob_overlap(blobs, left, right):
        """rm::LightBlobOverlap; raises RmcvError for right == len(blobs), where the reference reads past the end"""
        blobs = np.ascontiguousarray(blobs, LIGHTBLOB)
        o = C.c_int32(0)
        rc = lib().rmcv_lightblob_overlap(ptr(blobs), len(blobs), int(left), int(right), C.byref(o))
        if rc:
            raise RmcvError(rc, "rightIndex == size(): out of range in the reference")
        return bool(o.value)

    @staticmethod
    def max_iou(self_armour, armours):
        """rm::armour::max_IoU: (index, IoU) of the best-overlapping armour, index -1 when none overlaps"""
        me = np.ascontiguousarray(self_armour, ARMOUR).reshape(1)
        arr = np.ascontiguousarray(armours, ARMOUR)
        idx, iou = C.c_int32(0), C.c_float(0)
        rc = lib().rmcv_max_iou(ptr(me), ptr(arr), len(arr), C.byref(idx), C.byref(iou))
        if rc:
            raise RmcvError(rc, "rmcv_max_iou")
        return idx.value, iou.value

    @staticmethod
    def identity_max(history):
        """rm::armour::identity_max over {identity: count}: (identity, probability)"""
        ids = np.array(sorted(history), np.int32)
        cnt = np.array([history[int(k)] for k in ids], np.int32)
        mid, pr = C.c_int32(0), C.c_double(0)
        rc = lib().rmcv_identity_max(ptr(ids), ptr(cnt), len(ids), C.byref(mid), C.byref(pr))
        if rc:
            raise RmcvError(rc, "rmcv_identity_max")
        return mid.value, pr.value

    # ---------------------------------------------------------------- tracker state (src/core.cpp:51-122, main.cpp:57-88)
    @staticmethod
    def track_new(armour, identity, timestamp, position, noise=(5e-5, 0.5, 0.05)):
        """a detected armour as the process loop hands it to the tracking thread (main.cpp:178-195): constructed, identity /
        position / timestamp assigned, reset(5e-5, 0.5, 0.05) -> abi.TRACK record"""
        t = np.zeros(1, abi.TRACK)
        a = np.ascontiguousarray(armour, ARMOUR).reshape(1)
        pos = np.ascontiguousarray(position, np.float64)
        lib().rmcv_track_init(ptr(t), ptr(a), int(identity), C.c_int64(int(timestamp)), ptr(pos))
        if noise is not None:
            lib().rmcv_track_reset(ptr(t), C.c_double(noise[0]), C.c_double(noise[1]), C.c_double(noise[2]))
        return t[0]

    @staticmethod
    def track_update(track, observation, tick_frequency=1e9):
        """rm::armour::update(const armour&): returns the updated abi.TRACK record"""
        t = np.array([track], abi.TRACK)
        o = np.array([observation], abi.TRACK)
        rc = lib().rmcv_track_update(ptr(t), ptr(o), C.c_double(tick_frequency))
        if rc:
            raise RmcvError(rc, "rmcv_track_update")
        return t[0]

    @staticmethod
    def track_predict(track, new_timestamp, tick_frequency=1e9):
        """rm::armour::update(int64)"""
        t = np.array([track], abi.TRACK)
        rc = lib().rmcv_track_predict(ptr(t), C.c_int64(int(new_timestamp)), C.c_double(tick_frequency))
        if rc:
            raise RmcvError(rc, "rmcv_track_predict")
        return t[0]

    @staticmethod
    def track_step(tracking, observations, cap=64, tick_frequency=1e9):
        """one pass of the tracking thread's loop (main.cpp:60-85): returns the new tracking list"""
        buf = np.zeros(cap, abi.TRACK)
        nt = C.c_int32(len(tracking))
        if len(tracking):
            buf[:len(tracking)] = tracking
        obs = np.array(observations, abi.TRACK).copy() if len(observations) else np.zeros(1, abi.TRACK)
        no = C.c_int32(len(observations))
        rc = lib().rmcv_track_step(ptr(buf), C.byref(nt), cap, ptr(obs), C.byref(no), C.c_double(tick_frequency))
        if rc:
            raise RmcvError(rc, "rmcv_track_step")
        return buf[:nt.value].copy()

    def run_legacy(self, legacy, params=None, stages=STAGE_ALL, stream=None):
        """batch path with rm::FindLightBlobs (legacy: LegacyParams) in place of rm::filter_lightblobs"""
        self._params = params or default_params()
        self._legacy = legacy
        self._chk(lib().rmcv_batch_run_legacy(self._h, C.byref(self._params), C.byref(legacy), int(stages), C.c_void_p(stream or 0)))

    # ---------------------------------------------------------------- batch
    def upload(self, frames):
        """frames: uint8 [n, h, w, 3] on the host (or [n, h, w] mosaics under a Bayer input format, uint16 with 16-bit samples) -> the
        context's HBM buffer"""
        if self.input_format:
            frames = np.ascontiguousarray(frames, self._sample_dtype())
            assert frames.ndim == 3, "a Bayer input format takes (n, h, w) mosaics"
            n, h, w = frames.shape
            rowb = w * frames.itemsize
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            n, h, w, ch = frames.shape
            assert ch == 3
            rowb = 3 * w
        self._chk(lib().rmcv_batch_upload(self._h, ptr(frames), n, w, h, rowb, C.c_int64(rowb * h)))
        self.shape, self._windowed = (n, h, w), False

    def bind_device_frames(self, data_ptr, n, h, w, stride=None, frame_pitch=None, keepalive=None):
        """borrow frames already in HBM (e.g. torch_tensor.data_ptr()); strides are bytes, the default is 3 w, under a Bayer input
        format w (2 w with 16-bit samples)"""
        stride = stride or (w * self.sample_bits // 8 if self.input_format else 3 * w)
        frame_pitch = frame_pitch or stride * h
        self._frames_ref = keepalive
        self._chk(lib().rmcv_batch_set_device_frames(self._h, C.c_void_p(data_ptr), n, w, h, stride, C.c_int64(frame_pitch)))
        self.shape, self._windowed = (n, h, w), False

    # ---------------------------------------------------------------- windowed detection (rm::utils::GetROI -> extract_color(image(roi)))
    def set_windows(self, origins, win_w, win_h, keepalive=None):
        """read every frame bound through a win_w x win_h window: origins = (n, 2) integers (x, y) on the host (a numpy array or
        anything that converts to one), or an int = a device pointer to n rmcv_point (borrowed; read again by every run).  Any values:
        the library clamps them into the frame and snaps x down to a multiple of 16 (windows()).  binary / contours / blobs / armours
        are then those of the crops, in window coordinates.  win_w = 0: whole frames again."""
        n = self.shape[0]
        if not getattr(self, "_windowed", False):
            self._frame_shape = self.shape           # (n, h, w) of the frames as bound
        if win_w == 0:
            self._chk(lib().rmcv_batch_set_windows(self._h, None, 0, 0))
            self.shape, self._windowed = self._frame_shape, False
            return
        if isinstance(origins, (int, np.integer)):
            self._win_ref = keepalive
            self._chk(lib().rmcv_batch_set_device_windows(self._h, C.c_void_p(int(origins)), int(win_w), int(win_h)))
        else:
            o = np.ascontiguousarray(origins, np.int32).reshape(-1, 2)
            assert len(o) == n, "one origin per frame bound"
            self._chk(lib().rmcv_batch_set_windows(self._h, ptr(o), int(win_w), int(win_h)))
        self.shape, self._windowed = (n, int(win_h), int(win_w)), True

    def windows(self):
        """(effective origins int32 (n, 2) as (x, y), win_w, win_h) of the frames bound; zeros and (0, 0) without windows"""
        n = self.shape[0]
        eff = np.zeros((n, 2), np.int32)
        ww, wh = C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_batch_get_windows(self._h, ptr(eff), n, C.byref(ww), C.byref(wh)))
        return eff, ww.value, wh.value

    def device_windows(self):
        """(device pointer of the effective-origin table or None, win_w, win_h)"""
        d, ww, wh = C.c_void_p(), C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_batch_device_windows(self._h, C.byref(d), C.byref(ww), C.byref(wh)))
        return d.value, ww.value, wh.value

    get_roi = staticmethod(abi.get_roi)
    window_origin = staticmethod(abi.window_origin)
    armours_to_frame = staticmethod(abi.armours_to_frame)

    # ---------------------------------------------------------------- per-frame detection keys (serial_package::target per frame)
    def set_frame_camps(self, camps, lower_bounds=None, keepalive=None):
        """every frame bound gets its own camp and, optionally, its own lower bound: n integers each on the host (numpy arrays or
        anything that converts to one), or ints = device pointers to n int32 (borrowed; read again by every run).  Any values:
        frame_keys() shows what the kernels use.  lower_bounds None: the run's params.lower_bound.  camps None: per-run keys again
        (a new binding returns to them too)."""
        n = self.shape[0]
        if camps is None:
            self._chk(lib().rmcv_batch_set_frame_camps(self._h, None, None))
            return
        if isinstance(camps, (int, np.integer)):
            assert lower_bounds is None or isinstance(lower_bounds, (int, np.integer)), "device camps take device lower bounds"
            self._keys_ref = keepalive
            self._chk(lib().rmcv_batch_set_device_frame_camps(self._h, C.c_void_p(int(camps)), None if lower_bounds is None else C.c_void_p(int(lower_bounds))))
            return
        c = np.ascontiguousarray(camps, np.int32).reshape(-1)
        lb = None if lower_bounds is None else np.ascontiguousarray(lower_bounds, np.int32).reshape(-1)
        assert len(c) == n and (lb is None or len(lb) == n), "one camp (and one lower bound) per frame bound"
        self._chk(lib().rmcv_batch_set_frame_camps(self._h, ptr(c), ptr(lb)))

    def frame_keys(self):
        """the effective keys of the last run, int32 (n, 4): channel A, channel B, bound 1 .. 256, all-pass flag per frame"""
        n = self.shape[0]
        out = np.zeros((n, 4), np.int32)
        self._chk(lib().rmcv_batch_get_frame_keys(self._h, ptr(out), n))
        return out

    frame_key = staticmethod(abi.frame_key)

    def run(self, params=None, stages=STAGE_ALL, stream=None):
        self._params = params or default_params()
        self._chk(lib().rmcv_batch_run(self._h, C.byref(self._params), int(stages), C.c_void_p(stream or 0)))

    def track(self, tracker, timestamp, stream=None):
        """rmcv_batch_track: one step of a device-resident Tracker behind this context's last run (which included STAGE_ARMOURS), on
        that batch -- frame f is the next frame of the tracker's stream f.  Asynchronous; never synchronises."""
        self._chk(lib().rmcv_batch_track(self._h, tracker._h, C.c_int64(int(timestamp)), C.c_void_p(stream or 0)))

    def run_timed(self, params=None, stages=STAGE_ALL, stream=None):
        """returns ms of [binary, contours, blobs, armours, total] measured with HIP events on the launch stream"""
        self._params = params or default_params()
        ms = (C.c_float * 5)()
        self._chk(lib().rmcv_batch_run_timed(self._h, C.byref(self._params), int(stages), C.c_void_p(stream or 0), ms))
        return [float(x) for x in ms]

    def sync(self):
        self._chk(lib().rmcv_batch_sync(self._h))

    def counts(self):
        n = self.shape[0]
        a = [np.empty(n, np.int32) for _ in range(5)]
        self._chk(lib().rmcv_batch_counts(self._h, *[ptr(x) for x in a]))
        return dict(n_contours=a[0], n_points=a[1], n_blobs=a[2], n_armours=a[3], status=a[4])

    def binary(self, frame):
        n, h, w = self.shape
        out = np.empty((h, w), np.uint8)
        self._chk(lib().rmcv_batch_get_binary(self._h, int(frame), ptr(out)))
        return out

    def contours(self, frame):
        cap_p, cap_c = self.limits.max_points, self.limits.max_contours
        pts = np.empty(cap_p, POINT)
        offs = np.empty(cap_c + 1, np.int32)
        nc, npnt = C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_batch_get_contours(self._h, int(frame), ptr(pts), cap_p, ptr(offs), cap_c, C.byref(nc),
                                                C.byref(npnt)))
        return pts[:npnt.value].copy(), offs[:nc.value + 1].copy()

    def blobs(self, frame):
        cap = self.limits.max_blobs
        blobs = np.empty(cap, LIGHTBLOB)
        src = np.empty(cap, np.int32)
        nb = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_blobs(self._h, int(frame), ptr(blobs), cap, C.byref(nb), ptr(src)))
        return blobs[:nb.value].copy(), src[:nb.value].copy()

    def armours(self):
        """all armours of the batch, frame-major -> (ARMOUR[total], frame_offs[n+1])"""
        n = self.shape[0]
        cap = n * self.limits.max_armours
        out = np.empty(cap, ARMOUR)
        offs = np.empty(n + 1, np.int32)
        tot = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_armours(self._h, ptr(out), cap, ptr(offs), C.byref(tot)))
        return out[:tot.value].copy(), offs

    # ---------------------------------------------------------------- the operator's debug view
    def debug_views(self, frames, size=(1024, 768), flags=abi.VIEW_ALL, out=None, stream=None):
        """the debug images (executable/main.cpp:200-207, no text) of the chosen frames of the batch run last, rendered on the device at
        `size` = (vw, vh) (rmcv_batch_debug_views; asynchronous, behind the run).  out: a device pointer of the caller's for n contiguous
        (vh, vw, 3) views, e.g. a torch uint8 tensor's data_ptr() -- then returns None; without it the views come back as a host
        (n, vh, vw, 3) uint8 array (through a device buffer of the call's own; synchronises)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vw, vh = int(size[0]), int(size[1])
        pitch = 3 * vw * vh
        if out is not None:
            self._chk(lib().rmcv_batch_debug_views(self._h, ptr(fr), len(fr), vw, vh, int(flags), C.c_void_p(int(out)), 3 * vw, pitch, C.c_void_p(stream or 0)))
            return None
        d = C.c_void_p()
        nbytes = max(len(fr), 1) * max(pitch, 1)
        if lib().rmcv_device_alloc(self.device, C.c_int64(nbytes), C.byref(d)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            self._chk(lib().rmcv_batch_debug_views(self._h, ptr(fr), len(fr), vw, vh, int(flags), d, 3 * vw, pitch, C.c_void_p(stream or 0)))
            self.sync()
            host = np.empty((len(fr), vh, vw, 3), np.uint8)
            rc = lib().rmcv_device_download(self.device, ptr(host), d, C.c_int64(host.nbytes))
            if rc:
                raise RmcvError(rc, "rmcv_device_download")
            return host
        finally:
            lib().rmcv_device_free(self.device, d)

    def debug_view(self, frame, size=(1024, 768), flags=abi.VIEW_ALL):
        """one frame's debug image on the host, (vh, vw, 3) uint8 BGR (rmcv_batch_get_debug_view; refuses a frame with an overflow status)"""
        vw, vh = int(size[0]), int(size[1])
        out = np.empty((max(vh, 0), max(vw, 0), 3), np.uint8)
        self._chk(lib().rmcv_batch_get_debug_view(self._h, int(frame), vw, vh, int(flags), ptr(out), 3 * vw))
        return out

    def debug_view_of(self, binary, blobs=None, negatives=None, armours=None, size=(1024, 768), flags=abi.VIEW_ALL):
        """stage-wise: the debug image of host lists through the same kernels (rmcv_debug_view; arguments as abi.debug_view_host)"""
        args, out, keep = abi.view_args(binary, blobs, negatives, armours, flags, size)
        self._chk(lib().rmcv_debug_view(self._h, *args))
        return out

    # ---------------------------------------------------------------- the source view
    def source_views(self, frames, dst=None, size=(1024, 768), flags=abi.VIEW_ALL, stream=None):
        """the labeler's pictures (executable/svm/labeler.cpp:108-111, no text) of the chosen frames of the batch run last: the frame the
        results are defined on -- demosaiced, through its gamma table, cropped to its window, as the batch was read -- with the overlays
        of `flags` over it, rendered on the device at `size` = (vw, vh) (rmcv_batch_source_views; asynchronous, behind the run).  dst: a
        device pointer of the caller's for n contiguous (vh, vw, 3) views -- then returns None, and borrowed frames must stay valid until
        the views have finished; without it the views come back as a host (n, vh, vw, 3) uint8 array (synchronises)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vw, vh = int(size[0]), int(size[1])
        pitch = 3 * vw * vh
        if dst is not None:
            self._chk(lib().rmcv_batch_source_views(self._h, ptr(fr), len(fr), vw, vh, int(flags), C.c_void_p(int(dst)), 3 * vw, pitch, C.c_void_p(stream or 0)))
            return None
        d = C.c_void_p()
        nbytes = max(len(fr), 1) * max(pitch, 1)
        if lib().rmcv_device_alloc(self.device, C.c_int64(nbytes), C.byref(d)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            self._chk(lib().rmcv_batch_source_views(self._h, ptr(fr), len(fr), vw, vh, int(flags), d, 3 * vw, pitch, C.c_void_p(stream or 0)))
            self.sync()
            host = np.empty((len(fr), vh, vw, 3), np.uint8)
            rc = lib().rmcv_device_download(self.device, ptr(host), d, C.c_int64(host.nbytes))
            if rc:
                raise RmcvError(rc, "rmcv_device_download")
            return host
        finally:
            lib().rmcv_device_free(self.device, d)

    def source_view(self, frame, size=(1024, 768), flags=abi.VIEW_ALL):
        """one frame's source view on the host, (vh, vw, 3) uint8 BGR (rmcv_batch_get_source_view; refuses a frame with an overflow status)"""
        vw, vh = int(size[0]), int(size[1])
        out = np.empty((max(vh, 0), max(vw, 0), 3), np.uint8)
        self._chk(lib().rmcv_batch_get_source_view(self._h, int(frame), vw, vh, int(flags), ptr(out), 3 * vw))
        return out

    def source_view_of(self, bgr, blobs=None, negatives=None, armours=None, size=(1024, 768), flags=abi.VIEW_ALL):
        """stage-wise: the source view of a host BGR image and host lists through the same kernels (rmcv_source_view; arguments as
        abi.source_view_host)"""
        args, out, keep = abi.source_view_args(bgr, blobs, negatives, armours, flags, size)
        self._chk(lib().rmcv_source_view(self._h, *args))
        return out

    # ---------------------------------------------------------------- corner refinement
    def refine_corners(self, frames, corners, counts=None, win=(8, 8), zero_zone=(-1, -1), max_iters=40, eps=0.001, status=None, per_frame=None, stream=None):
        """cornerSubPix (executable/calibration/hand_eye.cpp:121) for the corners of the chosen frames of the batch bound, on the device
        (rmcv_batch_refine_corners; asynchronous).  corners: a host (n, per_frame, 2) array -- then returns (corners float32, status int32
        (n, per_frame)) (synchronises; counts: host (n,) or None) -- or a device pointer of the caller's to such a float32 table, with per_frame
        given, refined in place: counts and status are then device pointers or None, and the call returns None.  Corners are in the coordinates
        of the image the frame's results are defined on (a windowed batch: the window's)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        rule = (int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]), int(max_iters), float(eps))
        if isinstance(corners, (int, C.c_void_p)):
            d = lambda p: C.c_void_p(p.value if isinstance(p, C.c_void_p) else (int(p) if p else 0))
            self._chk(lib().rmcv_batch_refine_corners(self._h, ptr(fr), len(fr), d(corners), int(per_frame or 0), d(counts), *rule, d(status), C.c_void_p(stream or 0)))
            return None
        c = np.array(corners, np.float32)
        assert c.ndim == 3 and c.shape[2] == 2 and c.shape[0] == len(fr), "corners: (n, per_frame, 2)"
        n, per = c.shape[0], c.shape[1]
        cnt = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(-1)
        assert cnt is None or len(cnt) == n, "counts: one per chosen frame"
        st = np.zeros((n, per), np.int32)
        o_st, o_cnt = c.nbytes, c.nbytes + st.nbytes
        d = C.c_void_p()
        if lib().rmcv_device_alloc(self.device, C.c_int64(max(o_cnt + 4 * n, 1)), C.byref(d)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            at = lambda o: C.c_void_p((d.value or 0) + o)
            for o, a in ((0, c), (o_st, st)) + (((o_cnt, cnt),) if cnt is not None else ()):
                if a.nbytes and lib().rmcv_device_upload(self.device, at(o), ptr(a), C.c_int64(a.nbytes)):
                    raise RmcvError(abi.ERR_HIP, "rmcv_device_upload")
            self._chk(lib().rmcv_batch_refine_corners(self._h, ptr(fr), n, at(0), per, at(o_cnt) if cnt is not None else None, *rule, at(o_st), C.c_void_p(stream or 0)))
            self.sync()
            for o, a in ((0, c), (o_st, st)):
                if a.nbytes and lib().rmcv_device_download(self.device, ptr(a), at(o), C.c_int64(a.nbytes)):
                    raise RmcvError(abi.ERR_HIP, "rmcv_device_download")
            return c, st
        finally:
            lib().rmcv_device_free(self.device, d)

    def refined_corners(self, frame, corners, win=(8, 8), zero_zone=(-1, -1), max_iters=40, eps=0.001):
        """one frame of the batch bound, host corners in and out (rmcv_batch_get_refined_corners) -> (corners (n, 2) float32, status (n,) int32)"""
        c = np.array(corners, np.float32).reshape(-1, 2)
        st = np.zeros(len(c), np.int32)
        self._chk(lib().rmcv_batch_get_refined_corners(self._h, int(frame), ptr(c), len(c), int(win[0]), int(win[1]), int(zero_zone[0]), int(zero_zone[1]),
                                                       int(max_iters), float(eps), ptr(st)))
        return c, st

    def refine_corners_of(self, bgr, corners, win=(8, 8), zero_zone=(-1, -1), max_iters=40, eps=0.001):
        """stage-wise: a host BGR image and host corners through the same kernel (rmcv_corner_subpix; arguments and result as
        abi.corner_subpix_host)"""
        bgr, c, st = abi.corner_args(bgr, corners)
        self._chk(lib().rmcv_corner_subpix(self._h, ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], ptr(c), len(c), int(win[0]), int(win[1]),
                                           int(zero_zone[0]), int(zero_zone[1]), int(max_iters), float(eps), ptr(st)))
        return c, st

    # ---------------------------------------------------------------- the chessboard detector
    def find_chessboards(self, frames, cols, rows, params=None, corners=None, per_frame=None, counts=None, status=None, stream=None, **changes):
        """the inner corners of a cols x rows chessboard (findChessboardCorners, executable/calibration/hand_eye.cpp:119) in the chosen frames
        of the batch bound, on the device (rmcv_batch_find_chessboards; asynchronous).  Without `corners`: tables of this call's own ->
        (corners (n, cols rows, 2) float32, NaN where no board was found, counts (n,) int32, status (n,) int32) (synchronises).  With `corners`,
        a device pointer of the caller's to a float32 [n][per_frame][2] table: counts (int32 [n]) and status (int32 [n] or None) are device
        pointers too, and the call returns None -- the tables are what refine_corners takes.  params: a dict of abi.chess_defaults' keys."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        prm = abi.chess_params(params, **changes)
        d = lambda p: C.c_void_p(p.value if isinstance(p, C.c_void_p) else (int(p) if p else 0))
        if corners is not None:
            self._chk(lib().rmcv_batch_find_chessboards(self._h, ptr(fr), len(fr), int(cols), int(rows), ptr(prm), d(corners), int(per_frame or 0), d(counts), d(status),
                                                        C.c_void_p(stream or 0)))
            return None
        n, per = len(fr), max(int(cols) * int(rows), 1)
        c, cnt, st = np.full((n, per, 2), np.nan, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        o_cnt, o_st = c.nbytes, c.nbytes + 4 * n
        dev = C.c_void_p()
        if lib().rmcv_device_alloc(self.device, C.c_int64(max(o_st + 4 * n, 1)), C.byref(dev)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            at = lambda o: C.c_void_p((dev.value or 0) + o)
            if c.nbytes and lib().rmcv_device_upload(self.device, at(0), ptr(c), C.c_int64(c.nbytes)):
                raise RmcvError(abi.ERR_HIP, "rmcv_device_upload")
            self._chk(lib().rmcv_batch_find_chessboards(self._h, ptr(fr), n, int(cols), int(rows), ptr(prm), at(0), per, at(o_cnt), at(o_st), C.c_void_p(stream or 0)))
            self.sync()
            for o, a in ((0, c), (o_cnt, cnt), (o_st, st)):
                if a.nbytes and lib().rmcv_device_download(self.device, ptr(a), at(o), C.c_int64(a.nbytes)):
                    raise RmcvError(abi.ERR_HIP, "rmcv_device_download")
            return c, cnt, st
        finally:
            lib().rmcv_device_free(self.device, dev)

    def chessboard_of(self, frame, cols, rows, params=None, **changes):
        """one frame of the batch bound (rmcv_batch_get_chessboard) -> (corners (cols rows, 2) float32 or None, status, candidates (n, 3) int32)"""
        out = abi.chess_outputs(cols, rows)
        self._chk(lib().rmcv_batch_get_chessboard(self._h, int(frame), int(cols), int(rows), ptr(abi.chess_params(params, **changes)), *[ptr(a) for a in out]))
        return abi.chess_result(out)

    def find_chessboard(self, bgr, cols, rows, params=None, **changes):
        """stage-wise: a host BGR image through the same kernels (rmcv_find_chessboard; arguments and result as abi.find_chessboard_host)"""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        assert bgr.ndim == 3 and bgr.shape[2] == 3, "find_chessboard takes an (h, w, 3) BGR image"
        out = abi.chess_outputs(cols, rows)
        self._chk(lib().rmcv_find_chessboard(self._h, ptr(bgr), bgr.shape[1], bgr.shape[0], 3 * bgr.shape[1], int(cols), int(rows),
                                             ptr(abi.chess_params(params, **changes)), *[ptr(a) for a in out]))
        return abi.chess_result(out)

    def capture_corners(self, frames, cols, rows, win=(8, 8), params=None, zero_zone=(-1, -1), max_iters=40, eps=0.001):
        """a calibration capture: find then refine on one device table, two asynchronous calls with no host step in between ->
        (corners (n, cols rows, 2) float32, NaN where no board was found, counts (n,), board status (n,), corner status (n, cols rows)) int32"""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        n, per = len(fr), max(int(cols) * int(rows), 1)
        c, cnt, st, cst = np.full((n, per, 2), np.nan, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, per), np.int32)
        o_cnt, o_st, o_cst = c.nbytes, c.nbytes + 4 * n, c.nbytes + 8 * n
        dev = C.c_void_p()
        if lib().rmcv_device_alloc(self.device, C.c_int64(max(o_cst + cst.nbytes, 1)), C.byref(dev)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            at = lambda o: (dev.value or 0) + o
            for o, a in ((0, c), (o_cst, cst)):
                if a.nbytes and lib().rmcv_device_upload(self.device, C.c_void_p(at(o)), ptr(a), C.c_int64(a.nbytes)):
                    raise RmcvError(abi.ERR_HIP, "rmcv_device_upload")
            self.find_chessboards(fr, cols, rows, params, corners=at(0), per_frame=per, counts=at(o_cnt), status=at(o_st))
            self.refine_corners(fr, at(0), at(o_cnt), win, zero_zone, max_iters, eps, status=at(o_cst), per_frame=per)
            self.sync()
            for o, a in ((0, c), (o_cnt, cnt), (o_st, st), (o_cst, cst)):
                if a.nbytes and lib().rmcv_device_download(self.device, ptr(a), C.c_void_p(at(o)), C.c_int64(a.nbytes)):
                    raise RmcvError(abi.ERR_HIP, "rmcv_device_download")
            return c, cnt, st, cst
        finally:
            lib().rmcv_device_free(self.device, dev)

    # ---------------------------------------------------------------- the calibration solve
    def _dev_tables(self, arrays):
        """one device allocation holding the host arrays one behind the other, each at a multiple of 8 -> (base c_void_p, offsets)"""
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += (a.nbytes + 7) & ~7
        dev = C.c_void_p()
        if lib().rmcv_device_alloc(self.device, C.c_int64(max(total, 8)), C.byref(dev)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        return dev, offs

    def _dev_copy(self, dev, off, a, up):
        call = lib().rmcv_device_upload if up else lib().rmcv_device_download
        args = (C.c_void_p((dev.value or 0) + off), ptr(a)) if up else (ptr(a), C.c_void_p((dev.value or 0) + off))
        if a.nbytes and call(self.device, *args, C.c_int64(a.nbytes)):
            raise RmcvError(abi.ERR_HIP, "rmcv_device_upload" if up else "rmcv_device_download")

    def calibrate_cameras(self, corners, counts, cols, rows, square, size, view_camera=None, n_cameras=1, params=None, guesses=None, results=None, views=None,
                          per_frame=None, n_views=None, stream=None, **changes):
        """camera matrix and distortion of every camera of a fleet from its chessboard views, on the device (calibrateCamera,
        executable/calibration/hand_eye.cpp:128-131; rmcv_calibrate_cameras; asynchronous).  With host arrays -- corners (n_views, per_frame, 2)
        float32, counts (n_views,) or None, view_camera (n_views,) int32 or None -- returns ([CalibResult per camera], views: a CALIB_VIEW record
        array) (synchronises; `results` / `views`: record arrays the device tables start from, zeroed by default).  With `results`, a device
        pointer of the caller's to n_cameras struct rmcv_calib_result: corners, counts, view_camera (or None) and views are device pointers too --
        the tables find_chessboards and refine_corners wrote -- per_frame and n_views say their shape, and the call returns None.
        size = (w, h); guesses: abi.calib_guesses' forms (a host table either way)."""
        prm = abi.calib_params(params, **changes)
        g = abi.calib_guesses(guesses, int(n_cameras))
        d = lambda p: C.c_void_p(p.value if isinstance(p, C.c_void_p) else (int(p) if p else 0))
        call = lambda cor, cnt, vc, res, vw, per, n: self._chk(lib().rmcv_calibrate_cameras(
            self._h, cor, int(per), cnt, int(n), vc, int(n_cameras), int(cols), int(rows), float(square), int(size[0]), int(size[1]), ptr(prm), ptr(g), res, vw,
            C.c_void_p(stream or 0)))
        if results is not None and not isinstance(results, np.ndarray):
            call(d(corners), d(counts), d(view_camera), d(results), d(views), per_frame or 0, n_views or 0)
            return None
        corners, counts = abi.calib_tables(corners, counts)
        n = len(corners)
        vc = np.zeros(0, np.int32) if view_camera is None else np.ascontiguousarray(view_camera, np.int32).reshape(-1)
        assert view_camera is None or len(vc) == n, "one camera index per view"
        res0, views0 = abi.calib_outputs(max(int(n_cameras), 0), n)
        res = res0 if results is None else np.array(results, abi.CALIB_RESULT).reshape(-1)
        vw = views0 if views is None else np.array(views, abi.CALIB_VIEW).reshape(-1)
        tabs = [corners, counts, vc, res, vw]
        dev, offs = self._dev_tables(tabs)
        try:
            for o, a in zip(offs, tabs):
                self._dev_copy(dev, o, a, True)
            at = lambda k: C.c_void_p((dev.value or 0) + offs[k])
            call(at(0), at(1), at(2) if view_camera is not None else C.c_void_p(0), at(3), at(4), corners.shape[1], n)
            self.sync()
            self._dev_copy(dev, offs[3], res, False)
            self._dev_copy(dev, offs[4], vw, False)
            return [abi.CalibResult(r) for r in res], vw
        finally:
            lib().rmcv_device_free(self.device, dev)

    def calibrate_camera(self, corners, counts, cols, rows, square, size, params=None, guess=None, **changes):
        """stage-wise: one camera, host tables through the same kernels (rmcv_calibrate_camera; arguments and result as
        abi.calibrate_camera_host)"""
        corners, counts = abi.calib_tables(corners, counts)
        res, views = abi.calib_outputs(1, len(corners))
        g = abi.calib_guesses(None if guess is None else [guess], 1)
        self._chk(lib().rmcv_calibrate_camera(self._h, ptr(corners), corners.shape[1], ptr(counts), len(corners), int(cols), int(rows), float(square), int(size[0]),
                                              int(size[1]), ptr(abi.calib_params(params, **changes)), ptr(g), ptr(res), ptr(views)))
        return abi.CalibResult(res[0]), views

    # ---------------------------------------------------------------- the hand-eye solve
    def calibrate_hand_eyes(self, views, attitudes, gripper_t=None, view_camera=None, n_cameras=1, params=None, results=None, rows=None, n_views=None, stream=None,
                            **changes):
        """the mounting of every camera of a fleet on its gimbal from the calibration solve's view rows and the gimbals' attitudes, on the device
        (calibrateHandEye and the check loop, executable/calibration/hand_eye.cpp:140-180; rmcv_calibrate_hand_eyes; asynchronous).  With host
        arrays -- views CALIB_VIEW (n_views,), attitudes ATTITUDE (n_views,) or (n_views, 3) (roll, pitch, yaw), gripper_t (n_views, 3) or None,
        view_camera (n_views,) int32 or None -- returns ([HandEyeResult per camera], rows: a HANDEYE_VIEW record array) (synchronises;
        `results` / `rows`: record arrays the device tables start from, zeroed by default).  With `results`, a device pointer of the caller's to
        n_cameras struct rmcv_handeye_result: views, attitudes, gripper_t (or None), view_camera (or None) and rows are device pointers too --
        views as calibrate_cameras wrote them, attitudes for instance a Tracker's device_attitudes() -- n_views says their length, and the call
        returns None."""
        prm = abi.handeye_params(params, **changes)
        d = lambda p: C.c_void_p(p.value if isinstance(p, C.c_void_p) else (int(p) if p else 0))
        call = lambda vw, att, gt, vc, res, out, n: self._chk(lib().rmcv_calibrate_hand_eyes(self._h, vw, att, gt, int(n), vc, int(n_cameras), ptr(prm), res, out,
                                                                                            C.c_void_p(stream or 0)))
        if results is not None and not isinstance(results, np.ndarray):
            call(d(views), d(attitudes), d(gripper_t), d(view_camera), d(results), d(rows), n_views or 0)
            return None
        views, attitudes, gripper_t = abi.handeye_tables(views, attitudes, gripper_t)
        n = len(views)
        gt = np.zeros(0, np.float64) if gripper_t is None else gripper_t
        vc = np.zeros(0, np.int32) if view_camera is None else np.ascontiguousarray(view_camera, np.int32).reshape(-1)
        assert view_camera is None or len(vc) == n, "one camera index per view"
        res0, rows0 = abi.handeye_outputs(max(int(n_cameras), 0), n)
        res = res0 if results is None else np.array(results, abi.HANDEYE_RESULT).reshape(-1)
        out = rows0 if rows is None else np.array(rows, abi.HANDEYE_VIEW).reshape(-1)
        tabs = [views, attitudes, gt, vc, res, out]
        dev, offs = self._dev_tables(tabs)
        try:
            for o, a in zip(offs, tabs):
                self._dev_copy(dev, o, a, True)
            at = lambda k: C.c_void_p((dev.value or 0) + offs[k])
            none = C.c_void_p(0)
            call(at(0), at(1), at(2) if gripper_t is not None else none, at(3) if view_camera is not None else none, at(4), at(5), n)
            self.sync()
            self._dev_copy(dev, offs[4], res, False)
            self._dev_copy(dev, offs[5], out, False)
            return [abi.HandEyeResult(r) for r in res], out
        finally:
            lib().rmcv_device_free(self.device, dev)

    def calibrate_hand_eye(self, views, attitudes, gripper_t=None, params=None, **changes):
        """stage-wise: one camera, host tables through the same kernel (rmcv_calibrate_hand_eye; arguments and result as
        abi.calibrate_hand_eye_host)"""
        views, attitudes, gripper_t = abi.handeye_tables(views, attitudes, gripper_t)
        res, rows = abi.handeye_outputs(1, len(views))
        self._chk(lib().rmcv_calibrate_hand_eye(self._h, ptr(views), ptr(attitudes), ptr(gripper_t), len(views), ptr(abi.handeye_params(params, **changes)), ptr(res),
                                                ptr(rows)))
        return abi.HandEyeResult(res[0]), rows

    def calibrate(self, frames, cols, rows, square, size=None, win=(8, 8), chess_params=None, zero_zone=(-1, -1), corner_iters=40, corner_eps=0.001, params=None,
                  guess=None, attitudes=None, gripper_t=None, handeye_params=None, **changes):
        """a calibration from the frames bound: find, refine and solve on one device allocation, three asynchronous calls with no host step in
        between (beside capture_corners) -> (CalibResult, views (n,) CALIB_VIEW records, corners (n, cols rows, 2) float32 -- NaN where no board
        was found --, counts (n,), board status (n,), corner status (n, cols rows)) int32.  size: (w, h) of the frames, the bound batch's by default.
        With attitudes (one per frame: an ATTITUDE array or (n, 3) (roll, pitch, yaw) radians; gripper_t (n, 3) optional) the hand-eye solve is
        enqueued as a fourth call behind the third on the same allocation, and (HandEyeResult, rows (n,) HANDEYE_VIEW records) is appended to the
        tuple returned."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        n, per = len(fr), max(int(cols) * int(rows), 1)
        size = size or (self.shape[2], self.shape[1])
        c, cnt, st, cst = np.full((n, per, 2), np.nan, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, per), np.int32)
        res, vw = abi.calib_outputs(1, n)
        tabs = [c, cnt, st, cst, res, vw]
        if attitudes is not None:
            _, att, gt = abi.handeye_tables(vw, attitudes, gripper_t)
            hres, hrows = abi.handeye_outputs(1, n)
            tabs += [att, hres, hrows] + ([gt] if gt is not None else [])
        dev, offs = self._dev_tables(tabs)
        try:
            for o, a in zip(offs, tabs):
                self._dev_copy(dev, o, a, True)
            at = lambda k: (dev.value or 0) + offs[k]
            self.find_chessboards(fr, cols, rows, chess_params, corners=at(0), per_frame=per, counts=at(1), status=at(2))
            self.refine_corners(fr, at(0), at(1), win, zero_zone, corner_iters, corner_eps, status=at(3), per_frame=per)
            self.calibrate_cameras(at(0), at(1), cols, rows, square, size, params=params, guesses=None if guess is None else [guess], results=at(4), views=at(5),
                                   per_frame=per, n_views=n, **changes)
            if attitudes is not None:
                self.calibrate_hand_eyes(at(5), at(6), at(9) if gt is not None else None, params=handeye_params, results=at(7), rows=at(8), n_views=n)
            self.sync()
            for o, a in zip(offs, tabs):
                self._dev_copy(dev, o, a, False)
            if attitudes is not None:
                return abi.CalibResult(res[0]), vw, c, cnt, st, cst, abi.HandEyeResult(hres[0]), hrows
            return abi.CalibResult(res[0]), vw, c, cnt, st, cst
        finally:
            lib().rmcv_device_free(self.device, dev)

    # ---------------------------------------------------------------- the icon strip and the labeler's sheet
    def _to_host(self, call, n, rows, row_bytes):
        """run call(device pointer) into a device buffer of this call's own for n images of rows x row_bytes bytes; synchronise; download"""
        d = C.c_void_p()
        if lib().rmcv_device_alloc(self.device, C.c_int64(max(n * rows * row_bytes, 1)), C.byref(d)):
            raise RmcvError(abi.ERR_NOMEM, "rmcv_device_alloc")
        try:
            call(d)
            self.sync()
            host = np.empty((n, rows, row_bytes // 3, 3), np.uint8)
            rc = lib().rmcv_device_download(self.device, ptr(host), d, C.c_int64(host.nbytes))
            if rc:
                raise RmcvError(rc, "rmcv_device_download")
            return host
        finally:
            lib().rmcv_device_free(self.device, d)

    def icon_strips(self, frames, side=80, cap=None, dst=None, stream=None, counts=None):
        """the labeler's icon strips (executable/svm/labeler.cpp:93-106) of the chosen frames of the batch run last: every armour's icon
        rectified to side x side on the frame the results are defined on, slot j at columns [j side, (j + 1) side), zeros from the frame's
        count on (rmcv_batch_icon_strips; asynchronous, behind the run).  cap: slots per strip (default: the context's max_armours).
        dst: a device pointer of the caller's for n contiguous (side, cap side, 3) strips -- then returns None; counts: a device pointer for n
        int32, the icons rendered.  Without dst the strips come back as a host (n, side, cap side, 3) uint8 array (synchronises)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        side, cap = int(side), int(self.limits.max_armours if cap is None else cap)
        stride = 3 * cap * side
        cnt = C.c_void_p(int(counts)) if counts is not None else None

        def call(d):
            self._chk(lib().rmcv_batch_icon_strips(self._h, ptr(fr), len(fr), side, cap, d, stride, stride * side, cnt, C.c_void_p(stream or 0)))
        if dst is not None:
            call(C.c_void_p(int(dst)))
            return None
        return self._to_host(call, len(fr), max(side, 0), max(stride, 0))

    def icon_strip(self, frame, side=80, cap=None):
        """one frame's icon strip on the host -> ((side, cap side, 3) uint8 BGR, icons rendered) (rmcv_batch_get_icon_strip; refuses a frame
        with an overflow status)"""
        side, cap = int(side), int(self.limits.max_armours if cap is None else cap)
        out = np.empty((max(side, 0), max(cap * side, 0), 3), np.uint8)
        na = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_icon_strip(self._h, int(frame), side, cap, ptr(out), 3 * cap * side, C.byref(na)))
        return out, na.value

    def icon_strip_of(self, bgr, armours, side=80, cap=None):
        """stage-wise: the icon strip of a host BGR image and host armours through the same kernel (rmcv_icon_strip; arguments as
        abi.icon_strip_host)"""
        args, out, keep = abi.icon_strip_args(bgr, armours, side, cap)
        self._chk(lib().rmcv_icon_strip(self._h, *args))
        return out

    def labeler_sheets(self, frames, size=(640, 512), side=80, flags=abi.VIEW_ALL, dst=None, stream=None):
        """the labeler's sheets (executable/svm/labeler.cpp:113-119) of the chosen frames of the batch run last at view size `size` =
        (vw, vh): the source view with `flags` | the plain binary as BGR, over the icon strip -- (vh + side, 2 vw, 3) each
        (rmcv_batch_labeler_sheets; asynchronous, behind the run).  dst: a device pointer of the caller's for n contiguous sheets -- then
        returns None; without it the sheets come back as a host (n, vh + side, 2 vw, 3) uint8 array (synchronises)."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vw, vh, side = int(size[0]), int(size[1]), int(side)
        stride, rows = 6 * vw, vh + side

        def call(d):
            self._chk(lib().rmcv_batch_labeler_sheets(self._h, ptr(fr), len(fr), vw, vh, side, int(flags), d, stride, stride * rows, C.c_void_p(stream or 0)))
        if dst is not None:
            call(C.c_void_p(int(dst)))
            return None
        return self._to_host(call, len(fr), max(rows, 0), max(stride, 0))

    def labeler_sheet(self, frame, size=(640, 512), side=80, flags=abi.VIEW_ALL):
        """one frame's sheet on the host, (vh + side, 2 vw, 3) uint8 BGR (rmcv_batch_get_labeler_sheet; refuses a frame with an overflow status)"""
        vw, vh, side = int(size[0]), int(size[1]), int(side)
        out = np.empty((max(vh + side, 0), max(2 * vw, 0), 3), np.uint8)
        self._chk(lib().rmcv_batch_get_labeler_sheet(self._h, int(frame), vw, vh, side, int(flags), ptr(out), 6 * vw))
        return out

    # ---------------------------------------------------------------- view labels
    def view_labels(self, view, geometry, scale=1, armours=None, identities=None, positions=None, tracks=None, last_vertices=None, origin=(0, 0), stride=None):
        """stage-wise: the label pass over a HOST view through the kernel, in place (rmcv_view_labels; arguments as abi.view_labels_host,
        which is the same on the CPU)"""
        args, keep = abi.view_labels_args(view, geometry, scale, armours, identities, positions, tracks, last_vertices, origin, stride)
        self._chk(lib().rmcv_view_labels(self._h, *args))
        return view

    def batch_view_labels(self, frames, views, size=(1024, 768), scale=1, stride=None, pitch=None, stream=None):
        """the armours' lines -- 'identity: x, y, z' at vertices[0] -- of the chosen frames of the batch run last over their FINISHED views
        (rmcv_batch_view_labels; asynchronous, behind the run).  views: a device pointer to n views of `size` = (vw, vh), as debug_views /
        source_views wrote them for the same frames (rows `stride` bytes apart, views `pitch`; default: contiguous)"""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vw, vh = int(size[0]), int(size[1])
        stride = 3 * vw if stride is None else int(stride)
        pitch = stride * vh if pitch is None else int(pitch)
        self._chk(lib().rmcv_batch_view_labels(self._h, ptr(fr), len(fr), vw, vh, int(scale), C.c_void_p(int(views)), stride, pitch, C.c_void_p(stream or 0)))

    def batch_view_tracks(self, tracker, frames, views, size=(1024, 768), scale=1, stride=None, pitch=None, stream=None):
        """the targets `tracker` holds for the streams `frames` (frame f of the batch is stream f) over their finished views: quadrilateral
        and 'identity: x, y, z, lost_count' (rmcv_batch_view_tracks; asynchronous, behind the run and the tracker's step in flight)"""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        vw, vh = int(size[0]), int(size[1])
        stride = 3 * vw if stride is None else int(stride)
        pitch = stride * vh if pitch is None else int(pitch)
        self._chk(lib().rmcv_batch_view_tracks(self._h, tracker._h if tracker is not None else None, ptr(fr), len(fr), vw, vh, int(scale), C.c_void_p(int(views)),
                                               stride, pitch, C.c_void_p(stream or 0)))

    def device_views(self):
        """(armours device pointer, counts device pointer, per-frame capacity, n_frames) for a collective"""
        a, c = C.c_void_p(), C.c_void_p()
        cap, n = C.c_int32(0), C.c_int32(0)
        self._chk(lib().rmcv_batch_device_views(self._h, C.byref(a), C.byref(c), C.byref(cap), C.byref(n)))
        return a.value, c.value, cap.value, n.value

    def compact_armours_into(self, d_armours_ptr, cap, d_frame_offs_ptr, stream=None):
        """device-side compaction into caller HBM (async on `stream`)"""
        self._chk(lib().rmcv_batch_compact_armours(self._h, C.c_void_p(d_armours_ptr), int(cap), C.c_void_p(d_frame_offs_ptr),
                                                   C.c_void_p(stream or 0)))

    # ---------------------------------------------------------------- icon classifier (BASELINE config 5)
    def svm_load(self, weights, rho, labels):
        """linear one-vs-one C_SVC: weights [n_df, 1200] f32, rho [n_df] f64, labels [n_class] i32"""
        weights = np.ascontiguousarray(weights, np.float32)
        rho = np.ascontiguousarray(rho, np.float64)
        labels = np.ascontiguousarray(labels, np.int32)
        n_class = len(labels)
        assert weights.shape == (n_class * (n_class - 1) // 2, abi.SVM_FEATURES) and len(rho) == weights.shape[0]
        self._chk(lib().rmcv_svm_load(self._h, ptr(weights), ptr(rho), ptr(labels), n_class))

    def svm_predict(self, samples, model=0):
        """rmcv_svm_predict: the loaded model's labels of uint8 [n, 1200] icon rows, in the arithmetic of RMCV_STAGE_IDENTITY.
        model=k: entry k of the table of svm_load_models (rmcv_svm_predict_model); entry 0 is the loaded model."""
        s = np.ascontiguousarray(samples, np.uint8)
        s = s.reshape(len(s), -1) if s.size else s.reshape(0, abi.SVM_FEATURES)
        assert s.shape[1] == abi.SVM_FEATURES
        out = np.zeros(len(s), np.int32)
        if model:
            self._chk(lib().rmcv_svm_predict_model(self._h, int(model), ptr(s) if len(s) else None, len(s), ptr(out) if len(s) else None))
        else:
            self._chk(lib().rmcv_svm_predict(self._h, ptr(s) if len(s) else None, len(s), ptr(out) if len(s) else None))
        return out

    def svm_load_models(self, models):
        """the context's model table (rmcv_svm_load_models): a sequence of (weights [n_df, 1200] f32, rho [n_df] f64, labels [n_class] i32),
        or of objects with those attributes (rmcv_amd.svm.Model), one per colour or per robot.  Entry 0 is also what classify_armours
        and svm_predict use; set_frame_models picks an entry per frame.  Switches per-frame selection off."""
        keep, arr = [], (abi.SvmModel * max(len(models), 1))()
        for k, m in enumerate(models):
            w, r, l = (m.weights, m.rho, m.labels) if hasattr(m, "weights") else m
            w, r, l = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(r, np.float64), np.ascontiguousarray(l, np.int32)
            n_class = len(l)
            assert w.size == n_class * (n_class - 1) // 2 * abi.SVM_FEATURES and r.size * abi.SVM_FEATURES == w.size
            keep.append((w, r, l))
            arr[k] = abi.SvmModel(w.ctypes.data, r.ctypes.data, l.ctypes.data, n_class, 0)
        self._chk(lib().rmcv_svm_load_models(self._h, arr, len(models)))

    def set_frame_models(self, idx, keepalive=None):
        """every frame bound is classified with its own entry of the model table: n integers on the host (each inside the table, else
        RmcvError and nothing changes), or an int = device pointer to n int32 (borrowed; read again by every run with STAGE_IDENTITY; any
        values: frame_models() shows what the kernel used -- a device camps table works as it is with the table [svm_red, svm_blue]).
        None: model 0 for every frame (a new binding returns to that too)."""
        if idx is None:
            self._chk(lib().rmcv_batch_set_frame_models(self._h, None))
            return
        if isinstance(idx, (int, np.integer)):
            self._models_ref = keepalive
            self._chk(lib().rmcv_batch_set_device_frame_models(self._h, C.c_void_p(int(idx))))
            return
        i = np.ascontiguousarray(idx, np.int32).reshape(-1)
        assert len(i) == self.shape[0], "one model index per frame bound"
        self._chk(lib().rmcv_batch_set_frame_models(self._h, ptr(i)))

    def frame_models(self):
        """the effective model index of every frame in the last run with STAGE_IDENTITY and selection on, int32 (n,); zeros without selection"""
        out = np.zeros(self.shape[0], np.int32)
        self._chk(lib().rmcv_batch_get_frame_models(self._h, ptr(out), len(out)))
        return out

    frame_model = staticmethod(abi.frame_model)

    def harvest(self, ds, labels, flags=0, tag=0, stream=None):
        """rmcv_batch_harvest: append the bound batch's armours' icon rows to the DeviceDataset `ds`, behind its last run (which included
        STAGE_ARMOURS; no model needed).  labels: one int per frame (HARVEST_SKIP: the frame contributes nothing), or a device pointer (int)
        to them, borrowed (rmcv_batch_harvest_device).  flags: HARVEST_MISSES keeps only the armours the loaded model gives another label.
        Asynchronous: ds.count waits."""
        if isinstance(labels, int):
            self._chk(lib().rmcv_batch_harvest_device(self._h, ds._h, C.c_void_p(labels), int(flags), int(tag), stream))
            return
        lb = np.ascontiguousarray(labels, np.int32).reshape(-1)
        shape = getattr(self, "shape", None)
        if shape is not None and len(lb) != shape[0]:
            raise RmcvError(abi.ERR_BAD_ARG, "harvest: one label per frame bound")
        self._chk(lib().rmcv_batch_harvest(self._h, ds._h, ptr(lb), int(flags), int(tag), stream))

    def svm_train(self, samples, responses, perm=None, **params):
        """rmcv_svm_train on this context's GPU -> rmcv_amd.svm.Model (rmcv_amd.svm.train_auto with ctx=self)"""
        from . import svm
        return svm.train_auto(samples, responses, perm, ctx=self, **params)

    def classify_armours(self, image, armours):
        """main.cpp:178-181 for one frame -> (identity int32[n], armours with clamped icon, icons uint8[n,20,20,3])"""
        image, h, w, rowb = self._frame(image)
        arm = np.ascontiguousarray(armours, ARMOUR).copy()
        n = len(arm)
        ident = np.empty(max(n, 1), np.int32)
        icons = np.empty((max(n, 1), 20, 20, 3), np.uint8)
        self._chk(lib().rmcv_classify_armours(self._h, ptr(image), w, h, rowb, ptr(arm), n, ptr(ident), ptr(icons)))
        return ident[:n].copy(), arm, icons[:n].copy()

    def identities(self):
        n = self.shape[0]
        cap = n * self.limits.max_armours
        out = np.empty(cap, np.int32)
        tot = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_identities(self._h, ptr(out), cap, C.byref(tot)))
        return out[:tot.value].copy()

    def icons(self, frame):
        cap = self.limits.max_armours
        out = np.empty((cap, 20, 20, 3), np.uint8)
        na = C.c_int32(0)
        self._chk(lib().rmcv_batch_get_icons(self._h, int(frame), ptr(out), cap, C.byref(na)))
        return out[:na.value].copy()

    def detect_batch(self, frames, params=None):
        """the whole path of executable/main.cpp:172-176 on a batch of host frames"""
        self.upload(frames)
        self.run(params)
        self.sync()
        return self.armours()


def debug_view(ctx, binary, blobs=None, negatives=None, armours=None, size=(1024, 768), flags=abi.VIEW_ALL):
    """the debug image of host lists, rendered on ctx's device (rmcv_debug_view: the stage-wise form of Context.debug_views; arguments as
    rmcv_amd.debug_view_host, which is the same on the CPU)"""
    return ctx.debug_view_of(binary, blobs, negatives, armours, size, flags)
