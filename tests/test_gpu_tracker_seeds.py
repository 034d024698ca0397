"""k_track's hard branches on the GPU: the seeded cases of tests/track_seeds.py (more than 8 slots -- further rounds of the slot loop over
ws[wave] --, erase and TRK_KEEP, both overflow refusals, the 33rd identity, NaN states, dt <= 0, a step without observations on a
non-empty list, rmcv_tracker_put onto list 1) put into a tracker's streams and stepped by the kernel behind real batches.  After every
step every stream's tracks, side records, status and origin equal -- byte for byte -- the seeded RefStream (the oracle's tracker, hypot
pinned) and rmcv_tracker_step_host fed with what the GPU collected; the census every case asserts on the CPU is asserted again on the
GPU's own observations.  Every GPU step runs once, with the library's deadlines as they are."""
import numpy as np
import pytest

import track_seeds as K
import window_ref as W
from rmcv_amd import STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Context, Pipeline, Tracker, default_params, synth
from test_gpu_tracker import same

pytestmark = pytest.mark.gpu

FW, FH, WW, WH = K.FW, K.FH, K.WW, K.WH
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
OVF = 1


@pytest.fixture(scope="module")
def context():
    c = Context(device=0, max_frames=max(len(K.group_cases(g)) for g in K.GROUPS), max_width=FW, max_height=FH)
    assert c.limits.max_armours == 256
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    yield c
    c.close()


def collected(c, n):
    """what the batch left, per frame: Obs in window coordinates (read-only)"""
    arm, offs = c.armours()
    ids, pos, eff = c.identities(), c.poses()[2], c.windows()[0]
    assert len(ids) == len(pos) == len(arm) == offs[n]
    return [K.Obs(arm[offs[f]:offs[f + 1]].copy(), ids[offs[f]:offs[f + 1]].copy(), pos[offs[f]:offs[f + 1]].copy(), (int(eff[f][0]), int(eff[f][1])))
            for f in range(n)]


# ---------------------------------------------------------------- 1. context path: one tracker and one batch per group
@pytest.mark.parametrize("group", list(K.GROUPS))
def test_context_seeded_cases_three_chained_steps(group, context):
    c, cases, g = context, K.group_cases(group), K.GROUPS[group]
    n = len(cases)
    trk = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, **g.config)
    trk.set_origins(np.tile(np.array(K.ORIGIN0, np.int32), (n, 1)))
    streams = [K.Stream(case) for case in cases]
    refs = [s.ref for s in streams]
    frames = np.stack([K.frame(case.frame) for case in cases])
    black = np.zeros_like(frames)
    req = None if g.whole else np.array([case.request for case in cases], np.int32)
    refused = np.array([case.name in K.REFUSED for case in cases])
    reput = None
    for k, ts in enumerate(K.STAMPS):
        c.upload(black if k == 1 else frames)
        c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
        if req is None:
            c.set_windows(None, 0, 0)
        else:
            c.set_windows(req, WW, WH)
        c.run(default_params(), FULL)
        c.sync()
        obs = collected(c, n)
        if req is not None:                                 # clamped and snapped: (fx, fy) are those of track_seeds' table
            assert [o.eff for o in obs] == [K.effective_origin(case) for case in cases]
            assert np.array_equal(c.windows()[0], W.effective_origins(req, FW, FH, WW, WH))
        if k == 0:
            for f, s in enumerate(streams):
                tr, side = s.seed(obs[f], ts)
                trk.put(f, tr, side)
                s.put(tr, side)
                got = trk.get(f)
                assert got[0].tobytes() == tr.tobytes() and got[1].tobytes() == side.tobytes() and got[2] == K.ORIGIN0
        if k == 2:                                          # one applied step, one without observations: list 1 is current -- put lands there
            tr, side = streams[reput].seed(obs[reput], ts)
            trk.put(reput, tr, side)
            streams[reput].put(tr, side)
        c.track(trk, ts)
        c.sync()
        census = [s.step(o, ts) for s, o in zip(streams, obs)]   # (asserts rmcv_tracker_step_host == the seeded reference)
        same(trk, refs)
        st = trk.counts()[1]
        if k == 0:
            for case, cs in zip(cases, census):
                case.check(cs)
            assert np.array_equal(st == OVF, refused), st   # exactly the refused streams ...
            reput = next(f for f, cs in enumerate(census) if cs["applied"])
        elif k == 1:
            assert not any(cs["applied"] or cs["refused"] for cs in census)
            assert np.array_equal(st == OVF, refused), st   # ... and the flag is sticky
        else:
            cases[reput].check(census[reput])
            assert np.array_equal(st == OVF, refused | np.array([cs["refused"] for cs in census])), st
            assert (st[refused] == OVF).all()
        if group == "bare":
            assert all(r.origin == K.ORIGIN0 for r in refs)
    assert c.check_guards()[0] == 0
    trk.close()


# ---------------------------------------------------------------- 2. pipeline path: seeds put before anything is submitted
def test_pipeline_burst_over_seeded_lists(oracle):
    """two tracked submits per tracker in a burst, nothing collected in between: a whole-frame tracker over tile4 / plain frames and a
    windowed one whose second batch reads the origins its first step wrote.  Seeds come from the oracle's detection."""
    import torch
    svm = synth.svm_weights()
    whole = [K.Case("p_many_match", "bare", ("tile4", 0), None, K.b_many_match, K.c_many_match),
             K.Case("p_mixed", "bare", ("tile4", 32), None, K.b_mixed, K.c_mixed),
             K.Case("p_stamps", "bare", ("plain", 3), None, K.b_stamps, K.c_stamps)]
    wind = [K.Case("p_win_mixed", "win", ("plain", 26), (1001, 500), K.b_win_mixed, K.c_win_mixed),
            K.Case("p_win_stamps", "win", ("plain", 46), (213, 100), K.b_stamps, K.c_stamps)]
    ts0, ts1 = K.STAMPS[0], K.STAMPS[1]
    sides = []
    for cases in (whole, wind):
        n = len(cases)
        g = K.GROUPS[cases[0].group]
        trk = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, **g.config)
        origins = np.array([case.request or K.ORIGIN0 for case in cases], np.int32)
        trk.set_origins(origins)
        streams = [K.Stream(case, origin=tuple(origins[f])) for f, case in enumerate(cases)]
        for f, (case, s) in enumerate(zip(cases, streams)):
            eff = K.effective_origin(case)
            img = K.frame(case.frame) if case.request is None else W.crop(K.frame(case.frame), eff, WW, WH)
            arm = oracle.detect_frame(img, oracle.default_params())["armours"]
            tr, side = s.seed(K.Obs(arm, oracle.classify_armours(img, arm, svm)[0], None, eff), ts0)
            trk.put(f, tr, side)
            s.put(tr, side)
        dev = torch.from_numpy(np.stack([K.frame(case.frame) for case in cases])).cuda()
        sides.append((cases, trk, streams, dev))
    n_max = max(len(s[0]) for s in sides)
    # (hot_contexts off: the per-stage getters of a ticket need its context untouched by the rotation, as in test_gpu_tracker.py)
    pl = Pipeline(device=0, hot_contexts=-1, armour_cap=64, max_frames=n_max, max_width=FW, max_height=FH)     # (two tile4 frames: ~40 armours)
    for c in pl.contexts:
        c.svm_load(*svm)
        c.pnp_load()
        c.set_base2gripper(np.tile(np.eye(4), (n_max, 1, 1)))
    p = default_params()
    tickets = []
    for ts in (ts0, ts1):
        for cases, trk, streams, dev in sides:
            tickets.append((ts, pl.submit(dev.data_ptr(), len(cases), FH, FW, p, FULL, tracker=trk, timestamp=ts), cases, streams))
            assert pl.get_info().host_blocking_calls == 0
    for ts, t, cases, streams in tickets:
        n = len(cases)
        arm, offs = pl.collect(t)
        c = pl.context_of(t)
        ids, pos, eff = c.identities(), c.poses()[2], c.windows()[0]
        if cases[0].request is not None:                    # the windows the batch read: the clamp and snap of what the last step asked for
            assert np.array_equal(eff[:n], W.effective_origins(np.array([s.ref.origin for s in streams], np.int32), FW, FH, WW, WH)), ts
        else:
            eff = np.zeros((n, 2), np.int32)
        for f, (case, s) in enumerate(zip(cases, streams)):
            lo, hi = int(offs[f]), int(offs[f + 1])
            cs = s.step(K.Obs(arm[lo:hi].copy(), ids[lo:hi].copy(), pos[lo:hi].copy(), (int(eff[f][0]), int(eff[f][1]))), ts)
            if ts == ts0:
                case.check(cs)
            else:
                assert cs["applied"]
    for cases, trk, streams, dev in sides:
        same(trk, [s.ref for s in streams])
        assert not trk.counts()[1].any()
    assert any(s.ref.origin != tuple(case.request) for case, s in zip(wind, sides[1][2]))     # the windows followed their targets
    assert pl.get_info().host_blocking_calls == 0
    pl.close()
    for _, trk, _, _ in sides:
        trk.close()
