"""The recorder's loop records on the CPU: rmcv_loop_trigger_host equals the plain restatement of the header's rule
(tests/loop_ref.py) on directed pairs -- every bit both ways, every "needs aim / attitude in both" guard, NaN yaw and pitch, a zero mask --
and on seeded pairs; a session record with and without loop records round-trips byte for byte; a session written WITHOUT loop records is
byte-identical to what the commit before them wrote (tests/golden/session_plain.rmcv).  No GPU: none of these entry points needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_cases as K
import loop_ref as R
from rmcv_amd import abi, loop_bound, loop_trigger
from rmcv_amd.abi import LoopState, RecordEntry, RmcvError, TriggerConfig, lib, ptr
from rmcv_amd.recorder import LoopRecord, Session, loop_field_at

HERE = os.path.dirname(os.path.abspath(__file__))


def host_rule(p, c, mask, jump):
    cfg = TriggerConfig(0, 0, mask, 0, jump)
    fired = C.c_uint32(0xDEAD)
    assert lib().rmcv_loop_trigger_host(C.byref(p), C.byref(c), C.byref(cfg), C.byref(fired)) == 0
    return fired.value, cfg


def test_layout_sizes():
    assert C.sizeof(LoopState) % 8 == 0 and loop_bound(0) == C.sizeof(LoopState)
    assert loop_bound(16) == C.sizeof(LoopState) + 16 * (abi.TRACK.itemsize + 32)
    assert lib().rmcv_loop_bound(-1) == -1 and lib().rmcv_loop_bound(65) == -1
    assert loop_field_at(0) == "stream" and loop_field_at(C.sizeof(LoopState)) == "tracks[0].armour"
    assert loop_field_at(LoopState.aim.offset + 24) == "aim.yaw"


@pytest.mark.parametrize("case", K.directed_pairs(abi), ids=lambda c: c[0])
def test_trigger_rule_directed(case):
    _, p, c, mask, jump, bit, want = case
    fired, cfg = host_rule(p, c, mask, jump)
    assert fired == R.trigger(p, c, cfg)
    assert bool(fired & bit) == want
    assert loop_trigger(p, c, frame_status_mask=mask, aim_jump_deg=jump) == fired      # the Python face is the same call


def test_trigger_rule_calm_pair_raises_nothing():
    p, c = K.blank_state(abi), K.blank_state(abi)
    assert host_rule(p, c, 0x7F, 0.0)[0] == 0


def test_trigger_rule_seeded_pairs_equal_the_restatement():
    seen = 0
    for p, c, mask, jump in K.seeded_pairs(abi):
        fired, cfg = host_rule(p, c, mask, jump)
        assert fired == R.trigger(p, c, cfg), (bytes(p).hex(), bytes(c).hex(), mask, jump)
        seen |= fired
    assert seen == abi.TRIG_ALL                                                          # the seeds reach every bit


def test_trigger_host_refuses_null():
    s, f, cfg = K.blank_state(abi), C.c_uint32(0), TriggerConfig(0, 0, 0, 0, 1.0)
    for args in ((None, C.byref(s), C.byref(cfg), C.byref(f)), (C.byref(s), None, C.byref(cfg), C.byref(f)), (C.byref(s), C.byref(s), None, C.byref(f)),
                 (C.byref(s), C.byref(s), C.byref(cfg), None)):
        assert lib().rmcv_loop_trigger_host(*args) == abi.ERR_BAD_ARG


def _entry(packed, n_frames, loop_bytes, seq):
    e = RecordEntry()
    e.ticket = e.sequence = seq
    e.n_frames, e.batch_frames = n_frames, 4
    e.w, e.h, e.w_bytes, e.stride, e.lag = K.PLAIN_W // 3, K.PLAIN_H, K.PLAIN_W, K.PLAIN_W, K.PLAIN_LAG
    e.sample_bits, e.stages, e.user_bytes, e.loop_bytes = 8, 15, 3, loop_bytes
    for k in range(n_frames):
        e.frames[k], e.sizes[k] = k, len(packed[k])
    return e


def test_session_round_trip_with_and_without_loop_records(tmp_path):
    from rmcv_amd import pack
    packed = [pack(p, K.PLAIN_LAG) for p in K.plain_planes()]
    path = str(tmp_path / "loops.rmcv").encode()
    cap = 3
    loops = [K.seeded_loop_record(abi, cap, n, 100 + n) for n in (0, 3)]
    pp = (C.c_void_p * 2)(*[p.ctypes.data for p in packed])
    lp = (C.c_void_p * 2)(*[r.ctypes.data for r in loops])
    e0, e1 = _entry(packed, 2, loop_bound(cap), 0), _entry(packed, 1, 0, 1)
    assert lib().rmcv_session_append_loop(path, C.byref(e0), b"abc", pp, lp) == 0
    assert lib().rmcv_session_append(path, C.byref(e1), b"xyz", pp) == 0
    # loop records and an entry must agree before anything is written
    assert lib().rmcv_session_append(path, C.byref(e0), b"abc", pp) == abi.ERR_BAD_ARG
    assert lib().rmcv_session_append_loop(path, C.byref(e1), b"abc", pp, lp) == abi.ERR_BAD_ARG
    bad = _entry(packed, 2, loop_bound(cap) + 8, 2)
    assert lib().rmcv_session_append_loop(path, C.byref(bad), b"abc", pp, lp) == abi.ERR_BAD_ARG
    over = [loops[0].copy(), loops[1].copy()]
    LoopState.from_buffer(over[1]).n_tracks = cap + 1
    op = (C.c_void_p * 2)(*[r.ctypes.data for r in over])
    assert lib().rmcv_session_append_loop(path, C.byref(_entry(packed, 2, loop_bound(cap), 2)), b"abc", pp, op) == abi.ERR_BAD_ARG
    s = Session(path.decode())
    assert s.count() == 2
    g0, u0 = s.entry(0)
    assert bytes(g0) == bytes(e0) and u0 == b"abc" and g0.loop_bytes == loop_bound(cap)
    for k in range(2):
        assert np.array_equal(s.frame(0, k), packed[k])
        rec = s.loop(0, k)
        assert isinstance(rec, LoopRecord) and np.array_equal(rec.raw, loops[k])
        assert rec.tracks.tobytes() == b"".join(loops[k][800 + j * 2584:800 + j * 2584 + 2552].tobytes() for j in range(rec.state.n_tracks))
    g1, u1 = s.entry(1)
    assert bytes(g1) == bytes(e1) and u1 == b"xyz" and np.array_equal(s.frame(1, 0), packed[0])
    assert s.loops(1) == []
    with pytest.raises(RmcvError):
        s.loop(1, 0)                                                                     # an entry without loop records
    with pytest.raises(RmcvError):
        s.loop(0, 2)
    size = C.c_int64(0)
    assert lib().rmcv_session_loop(s._h, 0, 0, None, C.c_int64(0), C.byref(size)) == abi.ERR_CAPACITY and size.value == loop_bound(cap)
    s.close()


def test_session_without_loop_records_is_byte_identical_to_the_golden_file(tmp_path):
    path = tmp_path / "plain.rmcv"
    K.write_plain_session(lib(), RecordEntry, path)
    with open(os.path.join(HERE, "golden", "session_plain.rmcv"), "rb") as f:
        assert path.read_bytes() == f.read()
    s = Session(str(path))
    assert [s.entry(i)[0].loop_bytes for i in range(2)] == [0, 0]
    s.close()


def test_extractors_hand_out_the_setup_and_refuse_a_truncated_record():
    from rmcv_amd.tracker import AimConfig, AttitudeConfig, TrackerConfig
    s = K.blank_state(abi)
    s.tracker_config.n_streams, s.tracker_config.track_cap, s.tracker_config.tick_frequency = 5, 7, 1e6
    s.aim_config.v0, s.attitude_config.motor_angle_mode, s.gripper2camera[5] = 22.0, 1, 0.25
    tc, ac, tt, g, has = TrackerConfig(), AimConfig(), AttitudeConfig(), (C.c_double * 16)(), C.c_int32(-1)
    assert lib().rmcv_tracker_config_from_loop(C.byref(s), C.byref(tc)) == 0 and (tc.n_streams, tc.track_cap, tc.tick_frequency) == (5, 7, 1e6)
    assert lib().rmcv_tracker_aim_config_from_loop(C.byref(s), C.byref(ac), C.byref(has)) == 0 and has.value == 1 and ac.v0 == 22.0
    assert lib().rmcv_tracker_attitude_config_from_loop(C.byref(s), C.byref(tt), g, C.byref(has)) == 0 and has.value == 1 and tt.motor_angle_mode == 1 and g[5] == 0.25
    s.has_aim = 0
    assert lib().rmcv_tracker_aim_config_from_loop(C.byref(s), C.byref(ac), C.byref(has)) == 0 and has.value == 0
    for field, v in (("flags", abi.LOOP_TRUNCATED), ("n_tracks", -1), ("n_tracks", 65), ("n_tracking", 2)):
        t = abi.LoopState.from_buffer_copy(bytes(s))
        setattr(t, field, v)
        assert lib().rmcv_tracker_config_from_loop(C.byref(t), C.byref(tc)) == abi.ERR_BAD_ARG, field
        assert lib().rmcv_tracker_aim_config_from_loop(C.byref(t), C.byref(ac), C.byref(has)) == abi.ERR_BAD_ARG
        assert lib().rmcv_tracker_attitude_config_from_loop(C.byref(t), C.byref(tt), g, C.byref(has)) == abi.ERR_BAD_ARG
