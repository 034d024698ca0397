"""The session recorder for the closed loop on the GPU: loop records behind every tracked batch's step equal the tracker's
and the context's getters byte for byte; a saved session replays through a tracker with every byte back; the device-side trigger takes the
latch at the right record and the recorder freezes by itself, within the bound the header states; a record without a predecessor raises
nothing; a recorder with track_cap == 0 records what it always did; refusals leave everything usable.  Frames are the tracker tests'
1280 x 1024 with 512 x 384 windows, at most 6 streams and 10 batches; every GPU step runs once, with the library's deadlines."""
import ctypes as C

import numpy as np
import pytest

from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Pipeline, Recorder, RmcvError, Session, Tracker, abi, default_aim_config,
                      default_attitude_config, default_params, get_roi, loop_bound, loop_trigger, serial_encode, synth, window_origin)
from rmcv_amd.abi import LoopState, RecordEntry, lib

pytestmark = pytest.mark.gpu

FW, FH, WW, WH = 1280, 1024, 512, 384
MS = 1_000_000
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
N = 6


def device_array(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def moving(base, k, dx=2, dy=1):
    f = np.zeros_like(base)
    sx, sy = k * dx, k * dy
    f[:, sy:, sx:] = base[:, :FH - sy, :FW - sx]
    return f


@pytest.fixture(scope="module")
def base():
    """N frames with an armour each, and the window origin that centres each one's first armour (from the library's own whole-frame run)"""
    frames = synth.batch(0, N, FW, FH, CAMP_BLUE, 0, threads=16)
    pl = Pipeline(device=0, max_frames=N, max_width=FW, max_height=FH)
    d = device_array(frames)
    arm, offs = pl.collect(pl.submit(d.data_ptr(), N, FH, FW, default_params(), STAGE_ALL))
    pl.close()
    origins = []
    for f in range(N):
        assert offs[f + 1] > offs[f]
        origins.append(window_origin(get_roi(arm[offs[f]]["vertices"], (1.0, 1.0), (FW, FH)), WW, WH))
    return frames, np.array(origins, np.int32)


def new_pipeline(n=N, **kw):
    pl = Pipeline(device=0, max_frames=n, max_width=FW, max_height=FH, **kw)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
    return pl


def new_tracker(origins, n=N, windows=True, aim=True, attitude=True, camps=True, track_cap=8):
    win = dict(win_w=WW, win_h=WH) if windows else {}
    trk = Tracker(device=0, n_streams=n, track_cap=track_cap, frame_w=FW, frame_h=FH, **win)
    if windows:
        trk.set_origins(origins[:n])
    if aim:
        trk.set_aim(default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, lead_iterations=1))
    if camps:
        trk.set_camps(np.full(n, CAMP_BLUE, np.int32), np.full(n, 80, np.int32))
    if attitude:
        trk.set_attitude(default_attitude_config(motor_angle_mode=abi.ATT_MOTOR_PITCH))
    return trk


def packets(n, k, broken=()):
    """(n, 24) uint8 of step k: every stream's angles change every step; `broken`: streams whose CRC is wrong"""
    out = []
    for f in range(n):
        p = bytearray(serial_encode(CAMP_BLUE, 4.0 * (k + 1) + 11.0 * f, -2.5 * k + 3.0 * f - 4.0, 1.5 * k - 2.0 * f))
        if f in broken:
            p[23] ^= 0x40
        out.append(bytes(p))
    return np.frombuffer(b"".join(out), np.uint8).reshape(n, 24).copy()


def submit(pl, trk, dev, k, pk=None):
    return pl.submit(dev.data_ptr(), trk.n_streams, FH, FW, default_params(), FULL, tracker=trk, timestamp=(k + 1) * 8 * MS,
                     packets=None if pk is None else pk.data_ptr(), keepalive=(dev, pk))


def check_against_getters(rec_loops, chosen, trk, ctx, cap, on):
    """every loop record of the newest entry against the tracker's and the context's getters"""
    counts, status = trk.counts()
    aims, (atts, errs), inputs = trk.aims(), trk.attitudes(), trk.aim_inputs()
    eff, ww, wh = ctx.windows()
    n_arm = ctx.counts()
    for k, f in enumerate(chosen):
        r, s = rec_loops[k], rec_loops[k].state
        tracks, side, origin = trk.get(f)
        keep = min(len(tracks), cap)
        assert (s.stream, s.n_tracking, s.status) == (f, counts[f], status[f]) and s.n_tracking == len(tracks)
        assert s.n_tracks == keep and bool(s.flags & abi.LOOP_TRUNCATED) == (len(tracks) > cap)
        assert r.tracks.tobytes() == tracks[:keep].tobytes() and r.side.tobytes() == side[:keep].tobytes()
        assert not r.raw[loop_bound(keep):].any()                                      # the tail of the area is zero
        assert tuple(s.origin_next) == origin
        assert tuple(s.origin_eff) == (tuple(eff[f]) if on["windows"] else (0, 0))
        assert (s.n_armours, s.frame_status) == (n_arm["n_armours"][f], n_arm["status"][f])
        assert s.has_aim == int(on["aim"]) and s.has_attitude == int(on["attitude"]) and s.has_camps == (3 if on["camps"] else 0)
        assert bytes(s.aim) == aims[f].tobytes() and bytes(s.aim_input) == inputs[f].tobytes()
        if on["attitude"]:
            assert bytes(s.attitude) == atts[f].tobytes() and s.packet_errors == errs[f]
        else:
            assert bytes(s.attitude) == bytes(24) and s.packet_errors == 0 and not s.has_packet
        if on["camps"]:
            assert (s.camp, s.lower_bound) == (CAMP_BLUE, 80) and s.has_key and list(s.key) == list(ctx.frame_keys()[f])
        assert bytes(s.tracker_config) == bytes(trk.config)


# ---------------------------------------------------------------- 1. loop records equal the getters
@pytest.mark.parametrize("everything,chosen", [(True, [5, 0, 2]), (False, [2])], ids=["all_on_max_frames", "all_off_one_frame"])
def test_loop_records_equal_the_getters(base, everything, chosen):
    frames, origins = base
    on = dict(windows=everything, aim=everything, attitude=everything, camps=everything)
    cap = 1                                                                             # stream 0: exactly cap; stream 2: above; stream 5: none
    pl, trk = new_pipeline(), new_tracker(origins, **on)
    rec = Recorder(device=0, slots=3, max_frames=len(chosen), max_w_bytes=3 * FW, max_h=FH, track_cap=cap)
    pl.set_recorder(rec, chosen)
    steps = 4
    for k in range(steps):
        fr = moving(frames, k)
        fr[5] = 0                                                                       # stream 5 never sees an armour: no tracks
        dev = device_array(fr)
        pk = device_array(packets(N, k, broken=(2,) if k == 2 else ())) if everything else None
        t = submit(pl, trk, dev, k, pk)
        with pytest.raises(RmcvError) as e:                                             # the step is enqueued by the next call: no half-written record
            rec.count()
        assert e.value.code == abi.ERR_BAD_ARG and "tracker step" in str(e.value)
        pl.wait(t)
        i = rec.count() - 1
        entry, _ = rec.entry(i)
        assert entry.sequence == k and entry.loop_bytes == loop_bound(cap) and entry.n_frames == len(chosen)
        loops = rec.loops(i)
        check_against_getters(loops, chosen, trk, pl.context_of(t), cap, on)
        for k2, r in enumerate(loops):
            s = r.state
            assert s.sequence == k and s.timestamp == (k + 1) * 8 * MS and s.has_prev == int(k > 0)
            if everything:
                assert bytes(s.packet) == packets(N, k, broken=(2,) if k == 2 else ())[chosen[k2]].tobytes() and s.has_packet
                assert list(s.gripper2camera) == list(default_attitude_config().gripper2camera)
        if k == 0:                                                                      # one more track for stream 2, far from the others: it only ages
            tracks, side, _ = trk.get(2)
            grown = len(tracks) + 1
            assert 2 <= grown <= trk.track_cap and (not everything or grown == 2)
            more, side2 = np.concatenate([tracks, tracks[:1]]), np.concatenate([side, side[:1]])
            more["armour"]["bbox"][-1, :2] += 400
            trk.put(2, more, side2)
    n_tr = trk.counts()[0]
    assert n_tr[2] == grown > cap and n_tr[5] == 0 and (not everything or n_tr[0] == cap)
    if everything:
        assert trk.attitudes()[1][2] == 1                                               # the broken packet was counted: the record above held it
    assert pl.get_info().host_blocking_calls == 0
    rec.close(); trk.close(); pl.close()


# ---------------------------------------------------------------- 2. tracked replay
NR, SLOTS_R, STEPS_R = 3, 4, 6


@pytest.fixture(scope="module")
def recorded_session(base, tmp_path_factory):
    """a moving target recorded for more batches than the ring has slots, saved; with the live armours of every batch"""
    frames, origins = base
    pl, trk = new_pipeline(NR), new_tracker(origins, NR)
    rec = Recorder(device=0, slots=SLOTS_R, max_frames=NR, max_w_bytes=3 * FW, max_h=FH, track_cap=4)
    pl.set_recorder(rec, [0, 1, 2])
    live = {}
    for k in range(STEPS_R):
        dev, pk = device_array(moving(frames[:NR], k)), device_array(packets(NR, k))
        live[k] = pl.collect(submit(pl, trk, dev, k, pk))
    path = str(tmp_path_factory.mktemp("loop") / "moving.rmcv")
    rec.save(path)
    rec.close(); trk.close(); pl.close()
    return path, live


def test_tracked_replay_gives_every_byte_back(recorded_session):
    path, live = recorded_session
    s = Session(path)
    assert s.count() == SLOTS_R and [s.entry(i)[0].sequence for i in range(SLOTS_R)] == list(range(STEPS_R - SLOTS_R, STEPS_R))
    pl = new_pipeline(NR)
    out = s.replay_tracked(pl, verify=True)
    assert len(out) == SLOTS_R and out[0][1] is None
    for i in range(1, SLOTS_R):
        loops, (arm, offs) = out[i]
        for k in range(NR):
            assert np.array_equal(loops[k].raw, s.loop(i, k).raw), (i, k)
            assert loops[k].state.n_tracks >= 1 and loops[k].state.has_prev == 1
        seq = s.entry(i)[0].sequence
        assert arm.tobytes() == live[seq][0].tobytes() and offs.tolist() == live[seq][1].tolist()
    assert pl.get_info().host_blocking_calls == 0
    pl.close()
    s.close()


def _loop_offset(s, i, k):
    """file offset of loop record k of entry i (session_file.h: header 16; per record 8 + entry + blob to 8 + frames + loop records)"""
    at = 16
    for j in range(i + 1):
        e, _ = s.entry(j)
        body = C.sizeof(RecordEntry) + ((e.user_bytes + 7) & ~7) + sum(e.sizes[q] for q in range(e.n_frames))
        if j == i:
            return at + 8 + body + k * e.loop_bytes
        at += 8 + body + e.n_frames * e.loop_bytes


@pytest.mark.parametrize("what", ["state_post", "packet"])
def test_replay_names_an_altered_byte(recorded_session, tmp_path, what):
    path, _ = recorded_session
    s = Session(path)
    data = bytearray(open(path, "rb").read())
    fixed = C.sizeof(LoopState)
    if what == "state_post":    # a recorded RESULT: the replay computes the true value and names the field
        at = _loop_offset(s, 2, 1) + fixed + abi.TRACK.fields["state_post"][1] + 1
        expect = ["tracks[0].state_post"]
    else:                       # a recorded INPUT: the replay reads the altered packet, its CRC fails, and the consequence is named
        at = _loop_offset(s, 2, 1) + LoopState.packet.offset + 5
        expect = ["packet_errors", "attitude."]
    s.close()
    data[at] ^= 0x04
    alt = tmp_path / "altered.rmcv"
    alt.write_bytes(bytes(data))
    pl = new_pipeline(NR)
    with pytest.raises(RmcvError) as e:
        Session(str(alt)).replay_tracked(pl, verify=True)
    assert "entry 2 frame 1" in str(e.value) and any(name in str(e.value) for name in expect), str(e.value)
    out = Session(str(alt)).replay_tracked(pl, verify=False)                             # without verify the replay runs through
    assert len(out) == SLOTS_R
    pl.close()


# ---------------------------------------------------------------- 3. / 5. triggers, deterministic; no predecessor, no trigger
def check_fired_against_the_host_rule(rec):
    """for every pair of consecutive held entries: fired of the newer record is the host rule on the pair (0 without a predecessor)"""
    n, seen = rec.count(), 0
    for i in range(n):
        e, _ = rec.entry(i)
        for k, r in enumerate(rec.loops(i)):
            s = r.state
            if not s.has_prev:
                assert s.fired == 0
                continue
            if i == 0:                                                                  # its predecessor has left the ring
                continue
            assert rec.entry(i - 1)[0].sequence + 1 == e.sequence
            prev = rec.loop(i - 1, k)
            assert s.fired == loop_trigger(prev, r, frame_status_mask=s.trig_frame_status_mask, aim_jump_deg=s.trig_aim_jump_deg), (i, k)
            seen |= s.fired
    return seen


def test_triggers_deterministic(base):
    frames, origins = base
    n, chosen, post = 3, [2, 0], 2
    pl, trk = new_pipeline(n), new_tracker(origins, n)
    rec = Recorder(device=0, slots=pl.depth + post, max_frames=2, max_w_bytes=3 * FW, max_h=FH, track_cap=4)
    rec.set_trigger(abi.TRIG_NO_ARMOURS, post_batches=post)
    pl.set_recorder(rec, chosen)
    blank_at, k = 3, 0

    def step(blank=None, noise=None):
        nonlocal k
        fr = moving(frames[:n], k)
        if blank is not None:
            fr[blank] = 0
        if noise is not None:
            fr[noise] = np.random.default_rng(5).integers(0, 256, fr[noise].shape, dtype=np.uint8)
        dev, pk = device_array(fr), device_array(packets(n, k))
        t = submit(pl, trk, dev, k, pk)
        pl.wait(t)
        k += 1
        return t

    for _ in range(blank_at):
        step()
    assert not rec.trigger().fired
    step(blank=0)                                                                       # stream 0 = chosen frame k = 1 sees nothing at sequence 3
    info = rec.trigger()
    assert info.fired and (info.sequence, info.k, info.stream, info.mask) == (blank_at, 1, 0, abi.TRIG_NO_ARMOURS) and not info.noticed
    for _ in range(post + 3):                                                           # post more are recorded, the rest is not
        step()
    info = rec.trigger()
    assert info.noticed and info.batches_since == post
    held = [rec.entry(i)[0].sequence for i in range(rec.count())]
    assert held[-1] == blank_at + post and blank_at in held                             # exactly post batches behind s; frozen since
    assert check_fired_against_the_host_rule(rec) & abi.TRIG_NO_ARMOURS
    assert rec.loop(held.index(blank_at), 1).state.fired & abi.TRIG_NO_ARMOURS
    assert not rec.loop(held.index(blank_at), 0).state.fired & abi.TRIG_NO_ARMOURS
    # resume re-arms; the first batch behind it has no predecessor; then bits from real detections: the aim moves with the target (any
    # change is a jump against a bound of 0) and a frame of noise raises status bits the calm frames never had
    rec.set_trigger(abi.TRIG_AIM_JUMP | abi.TRIG_FRAME_STATUS, post_batches=1, frame_status_mask=0x7F, aim_jump_deg=0.0)
    rec.resume()
    assert not rec.trigger().fired and not rec.trigger().noticed
    step()
    first = rec.loops(rec.count() - 1)
    assert all(r.state.has_prev == 0 and r.state.fired == 0 for r in first) and not rec.trigger().fired
    seq0 = rec.entry(rec.count() - 1)[0].sequence
    step(noise=2)                                                                       # stream 2 = chosen frame k = 0
    info = rec.trigger()
    assert info.fired and info.sequence == seq0 + 1 and info.mask & (abi.TRIG_AIM_JUMP | abi.TRIG_FRAME_STATUS)
    got = rec.loop(rec.count() - 1, info.k).state
    assert got.stream == info.stream and got.fired & info.mask == info.mask
    assert rec.loop(rec.count() - 1, 0).state.fired & abi.TRIG_FRAME_STATUS              # the noise frame's new status bits
    for _ in range(3):
        step()
    held = [rec.entry(i)[0].sequence for i in range(rec.count())]
    assert held[-1] == seq0 + 2                                                          # post_batches = 1 behind the trigger
    seen = check_fired_against_the_host_rule(rec)
    assert seen & abi.TRIG_FRAME_STATUS
    assert pl.get_info().host_blocking_calls == 0
    rec.close(); trk.close(); pl.close()


def test_no_predecessor_no_trigger(base):
    frames, origins = base
    n = 2
    pl = new_pipeline(n)
    trk_a, trk_b = new_tracker(origins, n), new_tracker(origins, n)
    rec = Recorder(device=0, slots=pl.depth + 1, max_frames=1, max_w_bytes=3 * FW, max_h=FH, track_cap=2)
    rec.set_trigger(abi.TRIG_ALL, post_batches=1, frame_status_mask=0x7F, aim_jump_deg=0.0)
    pl.set_recorder(rec, [1])
    blank = np.zeros_like(frames[:n])
    dev, dev_blank, pk = device_array(frames[:n]), device_array(blank), device_array(packets(n, 0))

    def newest():
        i = rec.count() - 1
        return rec.entry(i)[0], rec.loops(i)

    # the first recorded batch
    pl.wait(submit(pl, trk_a, dev, 0, pk))
    e, loops = newest()
    assert e.loop_bytes and loops[0].state.has_prev == 0 and loops[0].state.fired == 0
    # an untracked submit gets no loop record while track_cap > 0 ...
    t = pl.submit(dev.data_ptr(), n, FH, FW, default_params(), FULL, keepalive=dev)
    pl.wait(t)
    e, loops = newest()
    assert e.loop_bytes == 0 and loops == []
    with pytest.raises(RmcvError):
        rec.loop(rec.count() - 1, 0)
    # ... and the tracked batch behind it has no predecessor, although its frame went blank
    pl.wait(submit(pl, trk_a, dev_blank, 1, pk))
    e, loops = newest()
    assert e.loop_bytes and loops[0].state.has_prev == 0 and loops[0].state.fired == 0 and loops[0].state.n_armours == 0
    # a batch of another tracker: nothing is compared either, in both directions
    pl.wait(submit(pl, trk_b, dev, 0, pk))
    assert newest()[1][0].state.has_prev == 0
    pl.wait(submit(pl, trk_a, dev_blank, 2, pk))
    assert newest()[1][0].state.has_prev == 0
    # the same tracker twice in a row: compared (the control -- the cases above are not vacuous)
    pl.wait(submit(pl, trk_a, dev, 3, pk))
    s = newest()[1][0].state
    assert s.has_prev == 1
    assert not rec.trigger().fired or rec.trigger().sequence == rec.entry(rec.count() - 1)[0].sequence
    rec.close(); trk_a.close(); trk_b.close(); pl.close()


# ---------------------------------------------------------------- 4. triggers, free-running
def test_triggers_free_running_within_the_bound(base):
    frames, origins = base
    n, post, blank_at, steps = 2, 1, 3, 10
    pl, trk = new_pipeline(n, depth=3), new_tracker(origins, n)
    depth = pl.depth
    rec = Recorder(device=0, slots=depth + post, max_frames=1, max_w_bytes=3 * FW, max_h=FH, track_cap=2)   # the ring at the refusal bound
    rec.set_trigger(abi.TRIG_NO_ARMOURS, post_batches=post)
    pl.set_recorder(rec, [0])
    devs = []
    for k in range(steps):
        fr = moving(frames[:n], k)
        if k == blank_at:
            fr[0] = 0
        devs.append((device_array(fr), device_array(packets(n, k))))
    tickets = []
    for k in range(steps):                                                              # no wait behind a submit: only the pipeline's own contract,
        if k >= depth:                                                                  # ticket t is collected before ticket t + depth is submitted
            pl.collect(tickets[k - depth])
        tickets.append(submit(pl, trk, devs[k][0], k, devs[k][1]))
    pl.drain()
    assert pl.get_info().host_blocking_calls == 0
    info = rec.trigger()
    assert info.fired and info.sequence == blank_at and info.noticed and info.batches_since == post
    held = [rec.entry(i)[0].sequence for i in range(rec.count())]
    assert blank_at in held                                                             # the triggering batch is still there
    assert blank_at + post <= held[-1] <= blank_at + depth + post - 1                    # the bound of rmcv_recorder_set_trigger
    assert held[-1] < steps - 1                                                         # frozen: the last submits recorded nothing
    before = rec.count()
    pl.wait(submit(pl, trk, devs[0][0], steps, devs[0][1]))
    assert rec.count() == before
    rec.close(); trk.close(); pl.close()


# ---------------------------------------------------------------- 6. off means off
def test_track_cap_zero_records_what_it_always_did(base):
    frames, origins = base
    n, steps = 3, 3
    runs = []
    for cap in (0, 4):
        pl, trk = new_pipeline(n), new_tracker(origins, n)
        rec = Recorder(device=0, slots=4, max_frames=2, max_w_bytes=3 * FW, max_h=FH, track_cap=cap)
        pl.set_recorder(rec, [2, 0])
        arms = []
        for k in range(steps):
            dev, pk = device_array(moving(frames[:n], k)), device_array(packets(n, k))
            arms.append(pl.collect(submit(pl, trk, dev, k, pk)))
        entries = []
        for i in range(rec.count()):
            e, user = rec.entry(i)
            assert e.loop_bytes == (loop_bound(cap) if cap else 0)
            e.loop_bytes = 0
            entries.append((bytes(e), user, [rec.frame(i, k).tobytes() for k in range(e.n_frames)]))
        state = (trk.aims().tobytes(), [tuple(x.tobytes() if hasattr(x, "tobytes") else x for x in trk.get(f)) for f in range(n)],
                 [c.tolist() for c in trk.counts()], trk.attitudes()[0].tobytes())
        runs.append((entries, [(a.tobytes(), o.tolist()) for a, o in arms], state))
        assert pl.get_info().host_blocking_calls == 0
        rec.close(); trk.close(); pl.close()
    assert runs[0][0] == runs[1][0]                                                     # packed frames and every pre-existing field of every entry
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]                        # the armours and the tracker's state


# ---------------------------------------------------------------- 7. refusals leave everything usable
def test_refusals_leave_everything_usable(base, recorded_session, tmp_path):
    frames, origins = base
    n = 2
    pl, trk = new_pipeline(n), new_tracker(origins, n)
    dev, pk = device_array(frames[:n]), device_array(packets(n, 0))
    # a mask on a recorder without loop records
    plain = Recorder(device=0, slots=8, max_frames=1, max_w_bytes=3 * FW, max_h=FH)
    with pytest.raises(RmcvError) as e:
        plain.set_trigger(abi.TRIG_NO_ARMOURS)
    assert e.value.code == abi.ERR_BAD_ARG and "track_cap" in str(e.value)
    for bad in (dict(post_batches=-1), dict(aim_jump_deg=float("nan")), dict(aim_jump_deg=-1.0)):
        rec = Recorder(device=0, slots=2, max_frames=1, max_w_bytes=3 * FW, max_h=FH, track_cap=1)
        with pytest.raises(RmcvError):
            rec.set_trigger(abi.TRIG_NO_ARMOURS, **bad)
        rec.close()
    # triggers armed on a ring below depth + post_batches: refused at set_recorder, and at the submit when armed afterwards
    small = Recorder(device=0, slots=pl.depth + 1, max_frames=1, max_w_bytes=3 * FW, max_h=FH, track_cap=1)
    small.set_trigger(abi.TRIG_NO_ARMOURS, post_batches=2)
    with pytest.raises(RmcvError) as e:
        pl.set_recorder(small, [0])
    assert e.value.code == abi.ERR_BAD_ARG and "ring" in str(e.value)
    small.set_trigger(None)
    pl.set_recorder(small, [0])
    small.set_trigger(abi.TRIG_NO_ARMOURS, post_batches=2)
    with pytest.raises(RmcvError) as e:
        submit(pl, trk, dev, 0, pk)
    assert e.value.code == abi.ERR_BAD_ARG and "ring" in str(e.value)
    small.set_trigger(abi.TRIG_NO_ARMOURS, post_batches=1)                              # at the bound: taken
    pl.wait(submit(pl, trk, dev, 0, pk))
    assert small.count() == 1 and small.loop(0, 0).state.n_tracks == 1
    # rmcv_tracker_restore from a truncated record: refused, the tracker as it was
    two = np.concatenate([trk.get(0)[0]] * 2)
    two["armour"]["bbox"][1, :2] += 400
    trk.put(0, two, np.concatenate([trk.get(0)[1]] * 2))
    pl.wait(submit(pl, trk, dev, 1, pk))
    r = small.loop(small.count() - 1, 0)
    assert r.truncated and r.state.n_tracking == 2 and r.state.n_tracks == 1
    before = trk.get(1)
    with pytest.raises(RmcvError) as e:
        trk.restore(1, r)
    assert e.value.code == abi.ERR_BAD_ARG and "truncated" in str(e.value)
    assert trk.get(1)[0].tobytes() == before[0].tobytes()
    pl.set_recorder(None, [])
    small.close(); plain.close(); trk.close()
    # replay of non-consecutive entries: a file of entries 0 and 2 of the recorded session
    path, _ = recorded_session
    s = Session(path)
    gap = str(tmp_path / "gap.rmcv").encode()
    for i in (0, 2):
        e, user = s.entry(i)
        fr, lp = [s.frame(i, k) for k in range(e.n_frames)], [s.loop(i, k).raw for k in range(e.n_frames)]
        pp, ll = (C.c_void_p * len(fr))(*[a.ctypes.data for a in fr]), (C.c_void_p * len(lp))(*[a.ctypes.data for a in lp])
        assert lib().rmcv_session_append_loop(gap, C.byref(e), user, pp, ll) == 0
    pl3 = new_pipeline(NR)
    with pytest.raises(RmcvError) as e:
        Session(gap.decode()).replay_tracked(pl3)
    assert "consecutive" in str(e.value)
    out = s.replay_tracked(pl3)                                                         # the pipeline is as usable as before
    assert len(out) == s.count()
    s.close(); pl3.close(); pl.close()
