"""Shared cases of the loop-record tests (tests/test_loop_cpu.py, tests/test_gpu_loop.py): the small session without loop records whose
bytes tests/golden/session_plain.rmcv holds as the commit before loop records wrote them, and seeded loop records for the trigger rule."""
import ctypes as C

import numpy as np

PLAIN_W, PLAIN_H, PLAIN_LAG = 300, 5, 3


def plain_planes():
    """the two planes of the plain session: seeded bytes, a flat run and a ramp in each"""
    rng = np.random.default_rng(20240917)
    out = []
    for k in range(2):
        p = (rng.poisson(3 + 20 * k, (PLAIN_H, PLAIN_W)) & 0xFF).astype(np.uint8)
        p[1, 40:200] = 7
        p[3] = (np.arange(PLAIN_W) * (k + 1)) & 0xFF
        out.append(p)
    return out


def write_plain_session(L, entry_type, path):
    """two records WITHOUT loop records through rmcv_session_append of the library handle L (entry_type: its RecordEntry), every call and
    every field the same whichever build L is"""
    planes = plain_planes()
    packed = []
    for p in planes:
        cap = L.rmcv_pack_bound(PLAIN_W, PLAIN_H)
        buf = np.zeros(cap, np.uint8)
        size = C.c_int64(0)
        rc = L.rmcv_pack_host(p.ctypes.data_as(C.c_void_p), PLAIN_W, PLAIN_H, C.c_int64(PLAIN_W), PLAIN_LAG, buf.ctypes.data_as(C.c_void_p), C.c_int64(cap),
                              C.byref(size))
        assert rc == 0
        packed.append(buf[:size.value].copy())
    for t in range(2):
        e = entry_type()
        C.memset(C.byref(e), 0, C.sizeof(e))
        e.ticket, e.sequence, e.timestamp = 10 + t, t, 1000 * t
        e.n_frames, e.batch_frames = 1 + t, 4
        e.w, e.h, e.w_bytes, e.stride, e.lag = PLAIN_W // 3, PLAIN_H, PLAIN_W, PLAIN_W, PLAIN_LAG
        e.input_format, e.sample_bits, e.stages = 0, 8, 15
        e.user_bytes = 5 * t
        e.params.camp, e.params.lower_bound = 1, 60 + t
        for k in range(e.n_frames):
            e.frames[k], e.sizes[k] = 3 - k, len(packed[k])
        ptrs = (C.c_void_p * 2)(*[p.ctypes.data for p in packed])
        assert L.rmcv_session_append(str(path).encode(), C.byref(e), b"hello"[:e.user_bytes], ptrs) == 0
    return packed


# ---- seeded loop records for the trigger rule -------------------------------------------------------------------------------------------
def blank_state(abi):
    """a calm fixed part: one armour, one track, a solved target of identity 3, aim and attitude on"""
    s = abi.LoopState()
    s.n_armours, s.n_tracking, s.n_tracks = 1, 1, 1
    s.has_aim, s.has_attitude = 1, 1
    s.aim.identity, s.aim.yaw, s.aim.pitch = 3, 10.0, -2.0
    return s


def directed_pairs(abi):
    """(name, prev, cur, frame_status_mask, aim_jump_deg, bit, expected) -- every bit both ways, every guard, NaN yaw and pitch"""
    nan, out = float("nan"), []

    def pair(name, bit, want, mask=0, jump=5.0, prev=None, cur=None):
        p, c = blank_state(abi), blank_state(abi)
        for s, kw in ((p, prev or {}), (c, cur or {})):
            for key, v in kw.items():
                obj = s
                *path, leaf = key.split(".")
                for part in path:
                    obj = getattr(obj, part)
                setattr(obj, leaf, v)
        out.append((name, p, c, mask, jump, bit, want))

    pair("armours gone", 1, True, cur={"n_armours": 0})
    pair("armours never there", 1, False, prev={"n_armours": 0}, cur={"n_armours": 0})
    pair("armours still there", 1, False, prev={"n_armours": 2}, cur={"n_armours": 1})
    pair("track dropped", 2, True, prev={"n_tracking": 3}, cur={"n_tracking": 2})
    pair("track added", 2, False, prev={"n_tracking": 2}, cur={"n_tracking": 3})
    pair("tracker overflow new", 4, True, cur={"status": 1})
    pair("tracker overflow old", 4, False, prev={"status": 1}, cur={"status": 1})
    pair("frame status new bit in mask", 8, True, mask=2 | 16, cur={"frame_status": 16})
    pair("frame status new bit outside mask", 8, False, mask=2, cur={"frame_status": 16})
    pair("frame status old bit", 8, False, mask=16, prev={"frame_status": 16}, cur={"frame_status": 16})
    pair("frame status zero mask", 8, False, mask=0, cur={"frame_status": 0x7F})
    pair("target lost", 16, True, cur={"aim.status": 1})
    pair("target never there", 16, False, prev={"aim.status": 1}, cur={"aim.status": 1})
    pair("target lost, no aim in prev", 16, False, prev={"has_aim": 0}, cur={"aim.status": 1})
    pair("target lost, no aim in cur", 16, False, cur={"aim.status": 1, "has_aim": 0})
    pair("target switch", 32, True, cur={"aim.identity": 4})
    pair("target same", 32, False)
    pair("target switch but cur has none", 32, False, cur={"aim.identity": 4, "aim.status": 1})
    pair("target switch but prev had none", 32, False, prev={"aim.status": 1}, cur={"aim.identity": 4})
    pair("target switch, no aim in prev", 32, False, prev={"has_aim": 0}, cur={"aim.identity": 4})
    pair("no solution new", 64, True, cur={"aim.status": 2})
    pair("no solution old", 64, False, prev={"aim.status": 2}, cur={"aim.status": 2})
    pair("no solution, no aim in cur", 64, False, cur={"aim.status": 2, "has_aim": 0})
    pair("yaw jump", 128, True, cur={"aim.yaw": 15.5})
    pair("yaw jump down", 128, True, cur={"aim.yaw": 4.5})
    pair("yaw at the bound", 128, False, cur={"aim.yaw": 15.0})
    pair("pitch jump", 128, True, cur={"aim.pitch": 3.5})
    pair("jump with an infinite bound", 128, False, jump=float("inf"), cur={"aim.yaw": 1e300})
    pair("jump with a zero bound", 128, True, jump=0.0, cur={"aim.yaw": 10.0 + 2 ** -40})
    pair("NaN yaw", 128, False, cur={"aim.yaw": nan})
    pair("NaN pitch in prev", 128, False, prev={"aim.pitch": nan})
    pair("NaN yaw but pitch jumps", 128, True, cur={"aim.yaw": nan, "aim.pitch": 30.0})
    pair("jump without a solution in cur", 128, False, cur={"aim.yaw": 50.0, "aim.status": 2})
    pair("jump without a target in prev", 128, False, prev={"aim.status": 1}, cur={"aim.yaw": 50.0})
    pair("jump, no aim in prev", 128, False, prev={"has_aim": 0}, cur={"aim.yaw": 50.0})
    pair("packet error", 256, True, cur={"packet_errors": 1})
    pair("packet errors equal", 256, False, prev={"packet_errors": 4}, cur={"packet_errors": 4})
    pair("packet error, no attitude in prev", 256, False, prev={"has_attitude": 0}, cur={"packet_errors": 1})
    pair("packet error, no attitude in cur", 256, False, cur={"packet_errors": 1, "has_attitude": 0})
    return out


def seeded_pairs(abi, n=400, seed=7):
    """(prev, cur, frame_status_mask, aim_jump_deg): fields drawn from small sets so that every comparison goes both ways many times"""
    rng = np.random.default_rng(seed)
    nan = float("nan")

    def draw():
        s = blank_state(abi)
        s.n_armours, s.n_tracking = int(rng.integers(0, 3)), int(rng.integers(0, 4))
        s.status, s.frame_status = int(rng.integers(0, 2)), int(rng.integers(0, 128))
        s.has_aim, s.has_attitude = int(rng.integers(0, 4) > 0), int(rng.integers(0, 4) > 0)
        s.aim.status, s.aim.identity = int(rng.choice([0, 0, 0, 1, 2, 3])), int(rng.integers(1, 4))
        s.aim.yaw = float(rng.choice([0.0, 1.0, 2.5, -3.0, nan, float("inf")]))
        s.aim.pitch = float(rng.choice([0.0, 0.5, 2.0, -4.0, nan]))
        s.packet_errors = int(rng.integers(0, 3))
        return s
    return [(draw(), draw(), int(rng.choice([0, 1, 16, 0x7F])), float(rng.choice([0.0, 1.0, 2.0, float("inf")]))) for _ in range(n)]


def seeded_loop_record(abi, cap, n_tracks, seed):
    """a loop area of rmcv_loop_bound(cap) bytes with n_tracks seeded tracks: bytes everywhere a recorder writes some, zeros behind"""
    rng = np.random.default_rng(seed)
    fixed, slot = C.sizeof(abi.LoopState), abi.TRACK.itemsize + abi.LOOP_SIDE_BYTES
    raw = np.zeros(fixed + cap * slot, np.uint8)
    raw[:fixed + n_tracks * slot] = rng.integers(0, 256, fixed + n_tracks * slot, dtype=np.uint8)
    s = abi.LoopState.from_buffer(raw)
    s.n_tracks = s.n_tracking = n_tracks
    s.flags = 0
    return raw
