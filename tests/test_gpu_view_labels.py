"""View labels on the GPU (k_view_text.hip): what the kernel draws over finished views equals the sequential restatement
rmcv_view_labels_host byte for byte -- the stage-wise helper on every case of tests/label_cases.py (which tests/test_view_labels_cpu.py
holds against the independent numpy reference), the batch route behind both view kinds fed from the getters (with and without identity
and pose, windowed, a non-identity frame list), the tracker's targets fed from rmcv_tracker_get, the refusals, and a pipeline's labelled
views.  Small shapes: 4 frames of 128 x 96, views of 96 x 40 and 160 x 120."""
import numpy as np
import pytest

import label_cases as K
from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_BINARY, STAGE_BLOBS, STAGE_CONTOURS, STAGE_IDENTITY, STAGE_POSE, VIEW_ARMOURS, Context, Pipeline, RmcvError, Tracker,
                      debug_view_host, default_params, source_view_host, synth, view_labels_host)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

FW, FH, N = 128, 96, 4
WW, WH = 96, 80
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
MS = 1_000_000
LIMITS = dict(max_frames=N, max_width=160, max_height=120)
# synthetic frames that carry 1, 1, 5 and 0 armours at this size: frame 2 needs a second trip of the kernel's four wavefronts, frame 3 draws nothing
INDICES = (1, 3, 18, 0)


def batch(shift0=0):
    """the 4-frame batch; shift0: frame 0 moved right by that many pixels (its target then no longer overlaps where it was)"""
    fr = np.stack([synth.frame(i, FW, FH, CAMP_BLUE, 0) for i in INDICES])
    if shift0:
        moved = np.zeros_like(fr[0])
        moved[:, shift0:] = fr[0][:, :FW - shift0]
        fr[0] = moved
    return fr


@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0, **LIMITS)
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    yield c
    c.close()


def device_buffer(nbytes, fill=0x5A):
    import torch
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


# ---- the kernel on host lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", K.SCALES)
def test_stagewise_labels_equal_the_host_restatement(ctx, scale):
    for case in K.cases():
        args = (case["geometry"] + (K.VW, K.VH), scale, case["armours"], case["identities"], case["positions"], case["tracks"], case["side"], case["origin"])
        want = view_labels_host(K.background(case["stride"]), *args, stride=case["stride"])
        got = ctx.view_labels(K.background(case["stride"]), *args, stride=case["stride"])
        assert np.array_equal(got, want), case["name"]


# ---- the batch route ----------------------------------------------------------------------------------------------------------------------
def lists_of(c, stages):
    """per frame (armours, identities | None, positions | None) from the getters"""
    c.sync()
    arm, offs = c.armours()
    ids = c.identities() if stages & STAGE_IDENTITY else None
    pos = c.poses()[2] if stages & STAGE_POSE else None
    return [(arm[offs[f]:offs[f + 1]], None if ids is None else ids[offs[f]:offs[f + 1]], None if pos is None else pos[offs[f]:offs[f + 1]]) for f in range(N)]


def base_view(c, frames, f, lists, dst, source, eff, geometry):
    if source:
        x, y = int(eff[f][0]), int(eff[f][1])
        crop = np.ascontiguousarray(frames[f][y:y + geometry[1], x:x + geometry[0]])
        return source_view_host(crop, None, None, lists[f][0], dst, VIEW_ARMOURS)
    return debug_view_host(c.binary(f), None, None, lists[f][0], dst, VIEW_ARMOURS)


def labelled_views(c, chosen, dst, scale, source):
    """views of the batch run last, rendered and labelled on the device -> host (n, vh, vw, 3)"""
    buf = device_buffer(len(chosen) * 3 * dst[0] * dst[1])
    if source:
        c.source_views(chosen, dst=buf.data_ptr(), size=dst, flags=VIEW_ARMOURS)
    else:
        c.debug_views(chosen, size=dst, flags=VIEW_ARMOURS, out=buf.data_ptr())
    c.batch_view_labels(chosen, buf.data_ptr(), dst, scale)
    c.sync()
    return buf.cpu().numpy().reshape(len(chosen), dst[1], dst[0], 3)


@pytest.mark.parametrize("stages", [FULL, STAGE_ALL], ids=["identity+pose", "neither"])
@pytest.mark.parametrize("source", [False, True], ids=["debug", "source"])
@pytest.mark.parametrize("windowed", [False, True], ids=["frames", "windows"])
def test_batch_labels_equal_the_restatement_fed_from_the_getters(ctx, stages, source, windowed):
    c, frames, chosen, dst, scale = ctx, batch(), [2, 0], (K.VW, K.VH), 1
    c.upload(frames)
    c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
    c.set_windows(np.array([[32, 16], [16, 8], [32, 16], [0, 0]], np.int32), WW, WH) if windowed else c.set_windows(None, 0, 0)
    try:
        c.run(default_params(), stages)
        lists = lists_of(c, stages)
        eff = c.windows()[0]
        geometry = (WW, WH) if windowed else (FW, FH)
        assert [len(l[0]) >= 1 for l in lists] == [True, True, True, False]   # frame 3 has no armours; frame 2 has more than the kernel has wavefronts
        assert len(lists[2][0]) > 4
        got = labelled_views(c, chosen, dst, scale, source)
        for k, f in enumerate(chosen):
            want = base_view(c, frames, f, lists, dst, source, eff, geometry)
            plain = want.copy()
            view_labels_host(want, geometry, scale, *lists[f])
            assert (want != plain).any(), f
            assert np.array_equal(got[k], want), (f, stages, source, windowed)
            if stages == STAGE_ALL:
                assert abi.label_text(-1) == "-1: 0.000000, 0.000000, 0.000000"   # what every line of such a run says
        # frame 3: the labels leave its view as the renderer wrote it
        got3 = labelled_views(c, [3], dst, scale, source)
        assert np.array_equal(got3[0], base_view(c, frames, 3, lists, dst, source, eff, geometry))
        assert c.check_guards()[0] == 0
    finally:
        c.set_windows(None, 0, 0)


def test_batch_labels_scale_stride_and_pitch(ctx):
    """a larger view at scale 2 in a caller's layout: rows and views padded, the rows not a multiple of 4, the first view one byte into its buffer"""
    c, frames, chosen, dst, scale = ctx, batch(), [2, 0, 1], (160, 120), 2
    c.upload(frames)
    c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
    c.run(default_params(), FULL)
    lists = lists_of(c, FULL)
    stride, pitch = 3 * dst[0] + 7, (3 * dst[0] + 7) * dst[1] + 5
    buf = device_buffer(1 + len(chosen) * pitch)
    fr = np.array(chosen, np.int32)
    c._chk(abi.lib().rmcv_batch_debug_views(c._h, abi.ptr(fr), len(fr), dst[0], dst[1], VIEW_ARMOURS, buf.data_ptr() + 1, stride, pitch, None))
    c.batch_view_labels(chosen, buf.data_ptr() + 1, dst, scale, stride=stride, pitch=pitch)
    c.sync()
    host = buf.cpu().numpy()
    assert host[0] == 0x5A
    for k, f in enumerate(chosen):
        rows = host[1 + k * pitch:1 + k * pitch + stride * dst[1]].reshape(dst[1], stride)
        want = view_labels_host(debug_view_host(c.binary(f), None, None, lists[f][0], dst, VIEW_ARMOURS), (FW, FH), scale, *lists[f])
        assert np.array_equal(rows[:, :3 * dst[0]].reshape(dst[1], dst[0], 3), want), f
        assert (rows[:, 3 * dst[0]:] == 0x5A).all() and (host[1 + k * pitch + stride * dst[1]:1 + (k + 1) * pitch] == 0x5A).all()
    assert c.check_guards()[0] == 0


# ---- the tracker's targets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windowed", [False, True], ids=["frames", "windows"])
def test_batch_tracks_equal_the_restatement_fed_from_the_tracker(ctx, windowed):
    c, dst, scale, chosen = ctx, (K.VW, K.VH), 1, [1, 3, 0, 2]
    win = dict(win_w=WW, win_h=WH) if windowed else {}
    trk = Tracker(device=0, n_streams=N, track_cap=4, frame_w=FW, frame_h=FH, **win)
    try:
        if windowed:
            trk.set_origins(np.array([[32, 16], [16, 8], [32, 16], [0, 0]], np.int32))
        for step, frames in enumerate((batch(), batch(shift0=28))):   # step 2: stream 0's target has moved away from its track
            c.upload(frames)
            c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
            if windowed:
                c.set_windows(trk.device_origins(), WW, WH)
            c.run(default_params(), FULL)
            c.track(trk, (step + 1) * 8 * MS)
        buf = device_buffer(len(chosen) * 3 * dst[0] * dst[1])
        c.debug_views(chosen, size=dst, flags=VIEW_ARMOURS, out=buf.data_ptr())
        c.batch_view_tracks(trk, chosen, buf.data_ptr(), dst, scale)
        c.sync()
        got = buf.cpu().numpy().reshape(len(chosen), dst[1], dst[0], 3)
        lists = lists_of(c, FULL)
        eff = c.windows()[0]
        geometry = (WW, WH) if windowed else (FW, FH)
        counts, lost = [], 0
        for k, f in enumerate(chosen):
            tracks, side, _ = trk.get(f)
            counts.append(len(tracks))
            lost = max(lost, int(tracks["lost_count"].max()) if len(tracks) else 0)
            want = debug_view_host(c.binary(f), None, None, lists[f][0], dst, VIEW_ARMOURS)
            plain = want.copy()
            view_labels_host(want, geometry, scale, tracks=tracks, last_vertices=side, origin=eff[f])
            assert (want != plain).any() == (len(tracks) > 0), f
            assert np.array_equal(got[k], want), (f, windowed)
        # stream 3 saw nothing, stream 2 saw five armours and holds none (its steps overflowed track_cap 4); a track of stream 0 was lost once
        assert counts[chosen.index(3)] == 0 and counts[chosen.index(2)] == 0 and sum(counts) >= 2
        if not windowed:   # (a window follows its target: what it shows of a moved one is not this test's to predict)
            assert counts[chosen.index(0)] >= 2 and lost > 0
        assert c.check_guards()[0] == 0
    finally:
        c.set_windows(None, 0, 0)
        trk.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx):
    c, dst, chosen = ctx, (K.VW, K.VH), [2, 0]
    c.upload(batch())
    c.run(default_params(), FULL)
    buf = device_buffer(len(chosen) * 3 * dst[0] * dst[1], fill=0xC3)
    good = Tracker(device=0, n_streams=N, track_cap=4, frame_w=FW, frame_h=FH)
    other = Tracker(device=0, n_streams=N + 1, track_cap=4, frame_w=FW, frame_h=FH)
    launches = abi.lib().rmcv_view_text_launches()

    def refused(call, text):
        with pytest.raises(RmcvError) as e:
            call()
        assert e.value.code == abi.ERR_BAD_ARG and text in str(e.value), str(e.value)

    try:
        for scale in (0, 9):
            refused(lambda: c.batch_view_labels(chosen, buf.data_ptr(), dst, scale), "scale")
            refused(lambda: c.batch_view_tracks(good, chosen, buf.data_ptr(), dst, scale), "scale")
        refused(lambda: c.batch_view_tracks(other, chosen, buf.data_ptr(), dst, 1), "streams")
        refused(lambda: c.batch_view_labels([2, 2], buf.data_ptr(), dst, 1), "repeated")
        refused(lambda: c.batch_view_labels([2, N], buf.data_ptr(), dst, 1), "outside")
        refused(lambda: c.batch_view_labels(chosen, buf.data_ptr(), dst, 1, stride=3 * dst[0] - 1), "stride")
        refused(lambda: c.batch_view_labels(chosen, buf.data_ptr(), dst, 1, pitch=3 * dst[0] * dst[1] - 1), "pitch")
        c.run(default_params(), STAGE_BINARY | STAGE_CONTOURS | STAGE_BLOBS)
        refused(lambda: c.batch_view_labels(chosen, buf.data_ptr(), dst, 1), "RMCV_STAGE_ARMOURS")
        refused(lambda: c.batch_view_tracks(good, chosen, buf.data_ptr(), dst, 1), "RMCV_STAGE_ARMOURS")
        c.sync()
        assert abi.lib().rmcv_view_text_launches() == launches
        assert (buf.cpu().numpy() == 0xC3).all()
    finally:
        good.close()
        other.close()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_labels(ctx):
    import torch
    c, dst, chosen, p = ctx, (K.VW, K.VH), [2, 0], default_params()
    sets = [batch(), batch(shift0=28), batch()]
    eye = np.tile(np.eye(4), (N, 1, 1))

    def context_path(frames):
        """(the plain views, the frames' lists) through the context: equal to the restatement by the tests above"""
        c.upload(frames)
        c.set_base2gripper(eye)
        c.run(p, FULL)
        lists = lists_of(c, FULL)
        return [debug_view_host(c.binary(f), None, None, lists[f][0], dst, VIEW_ARMOURS) for f in chosen], lists

    paths = [context_path(fr) for fr in sets]
    dev = [torch.from_numpy(fr).cuda() for fr in sets]
    pl = Pipeline(device=0, depth=2, **LIMITS)
    trk = Tracker(device=0, n_streams=N, track_cap=4, frame_w=FW, frame_h=FH)
    text_launches = abi.lib().rmcv_view_text_launches
    try:
        for pc in pl.contexts:
            pc.svm_load(*synth.svm_weights())
            pc.pnp_load()
            pc.set_base2gripper(eye)
        with pytest.raises(RmcvError):   # labels are drawn over views: none are set yet
            pl.set_view_labels(abi.LABEL_ARMOURS, 2)
        pl.set_views(chosen, dst, flags=VIEW_ARMOURS)
        for bad in ((abi.LABEL_ARMOURS, 0), (abi.LABEL_ARMOURS, 9), (4, 1)):
            with pytest.raises(RmcvError):
                pl.set_view_labels(*bad)
        pl.set_view_labels(abi.LABEL_ARMOURS, 2)

        def labelled(k, what, scale, tracks_of=None):
            views, lists = paths[k]
            out = []
            for v, f in zip(views, chosen):
                v = v.copy()
                tr, side = tracks_of(f) if tracks_of else (None, None)
                arm = lists[f] if what & abi.LABEL_ARMOURS else (None, None, None)
                out.append(view_labels_host(v, (FW, FH), scale, *arm, tracks=tr, last_vertices=side))
            return np.stack(out)

        n0, tickets = text_launches(), []
        for k in range(3):
            tickets.append(pl.submit(dev[k].data_ptr(), N, FH, FW, p, FULL))
            if k >= 1:   # ticket k - 1: its views live until ticket k + 1 is submitted
                pl.wait(tickets[k - 1])
                assert np.array_equal(pl.views(tickets[k - 1]).cpu().numpy(), labelled(k - 1, abi.LABEL_ARMOURS, 2)), k - 1
        pl.wait(tickets[2])
        assert np.array_equal(pl.views(tickets[2]).cpu().numpy(), labelled(2, abi.LABEL_ARMOURS, 2))
        assert (labelled(0, abi.LABEL_ARMOURS, 2) != np.stack(paths[0][0])).any()
        assert pl.get_info().host_blocking_calls == 0 and text_launches() - n0 == 3
        with pytest.raises(RmcvError):   # a labelled submit needs the armours
            pl.submit(dev[0].data_ptr(), N, FH, FW, p, STAGE_BINARY | STAGE_CONTOURS | STAGE_BLOBS)
        # off: the views are today's, and no label kernel is launched
        pl.set_view_labels(0, 0)
        n0 = text_launches()
        t = pl.submit(dev[1].data_ptr(), N, FH, FW, p, FULL)
        pl.wait(t)
        assert np.array_equal(pl.views(t).cpu().numpy(), np.stack(paths[1][0])) and text_launches() == n0
        # the tracker's targets behind the tracker step of the same submit, under the armours' lines
        pl.set_view_labels(abi.LABEL_ARMOURS | abi.LABEL_TRACKS, 1)
        with pytest.raises(RmcvError) as e:   # an untracked submit is refused before anything is enqueued
            pl.submit(dev[0].data_ptr(), N, FH, FW, p, FULL)
        assert e.value.code == abi.ERR_BAD_ARG and "tracker" in str(e.value)
        for k in (0, 1):
            t = pl.submit(dev[k].data_ptr(), N, FH, FW, p, FULL, tracker=trk, timestamp=(k + 1) * 8 * MS)
            pl.wait(t)
            got = pl.views(t).cpu().numpy()
            want = labelled(k, abi.LABEL_ARMOURS | abi.LABEL_TRACKS, 1, lambda f: trk.get(f)[:2])
            assert np.array_equal(got, want), k
        assert len(trk.get(0)[0]) >= 2 and int(trk.get(0)[0]["lost_count"].max()) > 0
        assert (want != labelled(1, abi.LABEL_ARMOURS, 1)).any()
        pl.set_view_labels(abi.LABEL_TRACKS, 1)
        t = pl.submit(dev[0].data_ptr(), N, FH, FW, p, FULL, tracker=trk, timestamp=3 * 8 * MS)
        pl.wait(t)
        assert np.array_equal(pl.views(t).cpu().numpy(), labelled(0, abi.LABEL_TRACKS, 1, lambda f: trk.get(f)[:2]))
        assert pl.get_info().host_blocking_calls == 0
        # turning the views off turns the labels off
        pl.set_views(None)
        t = pl.submit(dev[0].data_ptr(), N, FH, FW, p, FULL)
        pl.wait(t)
        assert all(pc.check_guards()[0] == 0 for pc in pl.contexts)
    finally:
        pl.close()
        trk.close()
