"""Per-frame detection keys (rmcv_batch_set_frame_camps / rmcv_pipeline_submit_camps / rmcv_tracker_set_camps) on the GPU.  The contract:
everything frame f produces equals, bit for bit, what the CPU oracle gives for that frame with camp = camps[f] and lower_bound =
lower_bounds[f].  Nothing has a tolerance.  The inputs are chosen so that a key applied to the wrong frame, or one key applied to all,
cannot pass: synthetic frames generated with alternating camps (under the other camp their armours are gone or different), frames dimmed
so that two bounds separate completely, random bytes for the pixel stage alone."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import track_ref as T
import window_ref as W
from rmcv_amd import (MORPH_CLOSE, MORPH_DILATE, MORPH_NONE, STAGE_ALL, STAGE_BINARY, STAGE_CONTOURS, STAGE_IDENTITY, STAGE_NO_IMAGE, STAGE_POSE,
                      Context, LegacyParams, Pipeline, RmcvError, Tracker, default_params, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu

N, FW, FH = 16, 512, 384
CAMPS = np.array([i & 1 for i in range(N)], np.int32)
MS = 1_000_000


def detect_all(oracle, frames, camps, lbs=None, morph=MORPH_CLOSE):
    def one(i):
        return oracle.detect_frame(frames[i], oracle.default_params(camp=int(camps[i]), lower_bound=80 if lbs is None else int(lbs[i]), morph=morph))
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, range(len(frames))))


@pytest.fixture(scope="module")
def mixed(oracle):
    """16 synthetic frames of 512 x 384, frame i generated with camp i & 1, and the oracle's results under the frame's own camp and under
    the other one (computed once, shared, never written)"""
    frames = np.stack([synth.frame(i, FW, FH, int(CAMPS[i])) for i in range(N)])
    return frames, detect_all(oracle, frames, CAMPS), detect_all(oracle, frames, 1 - CAMPS)


def check_frames(c, refs, image=True):
    """the context's batch (already run and synced) against per-frame oracle results: binary, contours, blobs as bytes (target too), armours"""
    arm, aoffs = c.armours()
    assert not (c.counts()["status"] & 15).any()
    for f, ref in enumerate(refs):
        if image:
            assert np.array_equal(c.binary(f), ref["binary"]), f
        pts, offs = c.contours(f)
        assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), f
        assert c.blobs(f)[0].tobytes() == ref["blobs"].tobytes(), f
        assert arm[aoffs[f]:aoffs[f + 1]].tobytes() == ref["armours"].tobytes(), f


def expected_keys(camps, lbs):
    return np.array([abi.frame_key(int(a), int(b)) for a, b in zip(camps, lbs)], np.int32)


# ---------------------------------------------------------------- 1. a mixed fleet's batch through the whole path
def test_mixed_camps_full_path(oracle, mixed):
    frames, own, other = mixed
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.upload(frames)
    c.set_frame_camps(CAMPS)
    c.run(default_params(), STAGE_ALL)                      # (params.camp is BLUE: a run that used it for every frame fails below)
    c.sync()
    check_frames(c, own)
    assert np.array_equal(c.frame_keys(), expected_keys(CAMPS, [80] * N))
    assert all(len(r["armours"]) for r in own)
    assert all((r["blobs"]["target"] == CAMPS[f]).all() and len(r["blobs"]) for f, r in enumerate(own))
    differ = sum(own[f]["armours"].tobytes() != other[f]["armours"].tobytes() for f in range(N))
    assert differ >= 8, differ
    assert all(not np.array_equal(own[f]["binary"], other[f]["binary"]) for f in range(N))
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 2. the bound per frame
def test_per_frame_lower_bound_on_dimmed_frames(oracle, mixed):
    frames = ((mixed[0].astype(np.uint16) * 112) >> 8).astype(np.uint8)
    lbs = np.array([60 if (i >> 1) & 1 else 140 for i in range(N)], np.int32)      # period 4 against the camps' 2
    refs = detect_all(oracle, frames, CAMPS, lbs)
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.upload(frames)
    c.set_frame_camps(CAMPS, lbs)
    c.run(default_params(lower_bound=99), STAGE_ALL)
    c.sync()
    check_frames(c, refs)
    assert np.array_equal(c.frame_keys(), expected_keys(CAMPS, lbs))
    for f in range(N):
        assert (len(refs[f]["armours"]) > 0) == (lbs[f] == 60), f
    # lower_bounds None: the run's bound for every frame, the camps still per frame
    c.set_frame_camps(CAMPS)
    c.run(default_params(lower_bound=60), STAGE_ALL)
    c.sync()
    check_frames(c, detect_all(oracle, frames, CAMPS, [60] * N))
    assert np.array_equal(c.frame_keys(), expected_keys(CAMPS, [60] * N))
    c.close()


# ---------------------------------------------------------------- 3. every pair, every loader, the pixel stage
CAMP_CYCLE, BOUND_CYCLE = (1, 0, 2, -1, 7), (0, 1, 37, 128, 255, 256, -5)
SHAPES = [("linear", 256, 96, None), ("row quads", 256, 96, 3 * 256 + 64), ("byte-wise", 200, 100, None)]


def bind(c, frames, stride):
    n, h, w, _ = frames.shape
    if stride is None:
        c.upload(frames)
        return None
    import torch
    buf = np.full((n, h, stride), 99, np.uint8)
    buf[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    t = torch.from_numpy(buf).cuda()
    c.bind_device_frames(t.data_ptr(), n, h, w, stride, stride * h, keepalive=t)
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_every_pair_and_bound_in_every_loader(oracle, shape):
    _, w, h, stride = shape
    n = 24
    rng = np.random.default_rng(w * 1000 + h + (stride or 0))
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    camps = np.array([CAMP_CYCLE[i % 5] for i in range(n)], np.int32)
    lbs = np.array([BOUND_CYCLE[i % 7] for i in range(n)], np.int32)
    c = Context(device=0, max_frames=n, max_width=256, max_height=128)
    keep = bind(c, frames, stride)
    c.set_frame_camps(camps, lbs)
    seen = set()
    for morph in (MORPH_NONE, MORPH_DILATE, MORPH_CLOSE):
        c.run(default_params(camp=2, lower_bound=11, morph=morph), STAGE_BINARY)
        c.sync()
        for f in range(n):
            want = oracle.extract_binary(frames[f], int(camps[f]), int(lbs[f]), morph)
            assert np.array_equal(c.binary(f), want), (morph, f, int(camps[f]), int(lbs[f]))
            seen.add(want.tobytes())
        assert np.array_equal(c.frame_keys(), expected_keys(camps, lbs))
    assert len(seen) > n                                    # the frames' images differ from one another and from morph to morph
    # the bit planes, through the contours of a sparse variant: the random image masked to a few blocks, no byte image
    sparse = np.zeros_like(frames)
    for f in range(n):
        for k in range(3):
            x, y = int(rng.integers(2, w - 20)), 3 + 32 * k + int(rng.integers(0, 12))
            sparse[f, y:y + 10, x:x + 14] = frames[f, y:y + 10, x:x + 14]
    keep = bind(c, sparse, stride)
    c.set_frame_camps(camps, lbs)
    c.run(default_params(morph=MORPH_CLOSE), STAGE_BINARY | STAGE_CONTOURS | STAGE_NO_IMAGE)
    c.sync()
    assert not (c.counts()["status"] & 15).any()
    total = 0
    for f in range(n):
        opts, ooffs = oracle.find_contours(oracle.extract_binary(sparse[f], int(camps[f]), int(lbs[f]), MORPH_CLOSE))
        pts, offs = c.contours(f)
        assert np.array_equal(offs, ooffs) and np.array_equal(pts, opts), f
        total += len(ooffs) - 1
    assert total >= n
    assert c.check_guards()[0] == 0
    del keep
    c.close()


# ---------------------------------------------------------------- 4. device tables are read again by every run
def test_device_tables_are_read_by_every_run(oracle, mixed):
    import torch
    frames, own, other = mixed
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.upload(frames)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_camps = torch.from_numpy(CAMPS).cuda()
        d_lbs = torch.full((N,), 80, dtype=torch.int32, device="cuda")
    s.synchronize()
    c.set_frame_camps(d_camps.data_ptr(), d_lbs.data_ptr(), keepalive=(d_camps, d_lbs))
    c.run(default_params(), STAGE_ALL, stream=s.cuda_stream)
    c.sync()
    check_frames(c, own)
    # new contents on the same stream, no second set call: the other camp for every frame
    with torch.cuda.stream(s):
        d_camps.copy_(1 - d_camps)
    c.run(default_params(), STAGE_ALL, stream=s.cuda_stream)
    c.sync()
    check_frames(c, other)
    assert np.array_equal(c.frame_keys(), expected_keys(1 - CAMPS, [80] * N))
    c.close()


# ---------------------------------------------------------------- 5. windows and keys together
def test_windows_and_keys_together(oracle):
    n, fw, fh, ww, wh = 8, 640, 512, 256, 192
    camps = np.array([i & 1 for i in range(n)], np.int32)
    frames = np.stack([synth.frame(200 + i, fw, fh, int(camps[i])) for i in range(n)])
    whole = detect_all(oracle, frames, camps)
    assert all(len(r["armours"]) for r in whole)
    origins = np.array([W.window_origin(W.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (fw, fh)), ww, wh) for r in whole], np.int32)
    eff = W.effective_origins(origins, fw, fh, ww, wh)
    crops = np.stack([W.crop(frames[f], eff[f], ww, wh) for f in range(n)])
    refs, refs_other = detect_all(oracle, crops, camps), detect_all(oracle, crops, 1 - camps)
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    c.upload(frames)
    c.set_frame_camps(camps)                                # keys first, windows second: neither undoes the other
    c.set_windows(origins, ww, wh)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert np.array_equal(c.windows()[0], eff)
    check_frames(c, refs)
    assert sum(len(r["armours"]) > 0 for r in refs) >= n - 1
    assert sum(refs[f]["armours"].tobytes() != refs_other[f]["armours"].tobytes() for f in range(n)) >= n // 2
    # ... and the byte-wise loader (a window width that is no multiple of 64)
    c.set_windows(origins, 200, 150)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    eff2 = W.effective_origins(origins, fw, fh, 200, 150)
    check_frames(c, detect_all(oracle, np.stack([W.crop(frames[f], eff2[f], 200, 150) for f in range(n)]), camps))
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 6. the pipeline
def test_pipeline_submits_with_keys(oracle, mixed):
    import torch
    frames, own, other = mixed
    ww, wh = 256, 192
    origins = np.array([W.window_origin(W.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (FW, FH)), ww, wh) for r in own], np.int32)
    p = default_params()
    # the context path's records: whole frames with keys, windows with keys, whole frames without (params.camp = BLUE for every frame)
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.upload(frames)
    c.set_frame_camps(CAMPS)
    c.run(p, STAGE_ALL)
    c.sync()
    want_keys = tuple(x.tobytes() for x in c.armours())
    c.set_windows(origins, ww, wh)
    c.run(p, STAGE_ALL)
    c.sync()
    want_win = tuple(x.tobytes() for x in c.armours())
    c.upload(frames)
    c.run(p, STAGE_ALL)
    c.sync()
    want_plain = tuple(x.tobytes() for x in c.armours())
    c.close()
    assert len({want_keys, want_win, want_plain}) == 3
    assert want_keys[0] == np.concatenate([r["armours"] for r in own]).tobytes()
    dev, d_camps, d_orig = torch.from_numpy(frames).cuda(), torch.from_numpy(CAMPS).cuda(), torch.from_numpy(origins).cuda()
    pl = Pipeline(device=0, max_frames=N, max_width=FW, max_height=FH)
    kinds = ["plain"] * 5 + ["keys", "win", "plain"] * 3 + ["plain"] * 2
    want = dict(plain=want_plain, keys=want_keys, win=want_win)
    tickets, hot = [], []
    for kind in kinds:
        before = pl.get_info().hot_batches
        if kind == "plain":
            tickets.append(pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL))
        elif kind == "keys":
            tickets.append(pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL, camps=(d_camps.data_ptr(), None)))
        else:
            tickets.append(pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL, camps=(d_camps.data_ptr(), None), windows=(d_orig.data_ptr(), ww, wh)))
        hot.append((kind, pl.get_info().hot_batches - before))
        if len(tickets) > pl.depth - 1:
            i = len(tickets) - pl.depth
            arm, offs = pl.collect(tickets[i])
            assert (arm.tobytes(), offs.tobytes()) == want[kinds[i]], (i, kinds[i])
    pl.drain()
    for i in range(max(0, len(kinds) - pl.depth + 1), len(kinds)):
        arm, offs = pl.collect(tickets[i])
        assert (arm.tobytes(), offs.tobytes()) == want[kinds[i]], (i, kinds[i])
    assert pl.get_info().host_blocking_calls == 0
    assert all(grew == 0 for kind, grew in hot if kind != "plain")      # batches with keys stay out of the hot rotation
    # the per-stage getters of a ticket with keys
    t = pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL, camps=(d_camps.data_ptr(), None))
    pl.wait(t)
    cx = pl.context_of(t)
    assert np.array_equal(cx.frame_keys(), expected_keys(CAMPS, [80] * N))
    for f in (0, 1, N - 1):
        assert np.array_equal(cx.binary(f), own[f]["binary"]) and cx.blobs(f)[0].tobytes() == own[f]["blobs"].tobytes()
    # refused before anything is enqueued; the pipeline stays usable
    with pytest.raises(RmcvError) as e:
        pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL, camps=(0, None))
    assert e.value.code == abi.ERR_BAD_ARG and "null camps" in str(e.value)
    arm, offs = pl.collect(pl.submit(dev.data_ptr(), N, FH, FW, p, STAGE_ALL))
    assert (arm.tobytes(), offs.tobytes()) == want_plain
    assert pl.get_info().host_blocking_calls == 0
    pl.close()


# ---------------------------------------------------------------- 7. behind a tracker
@pytest.mark.parametrize("win", [(0, 0), (256, 192)], ids=["whole frames", "windows"])
def test_tracked_submits_with_per_stream_camps(oracle, win):
    import torch
    from test_gpu_tracker import same
    n, steps = 8, 4
    ww, wh = win
    camps = np.array([i & 1 for i in range(n)], np.int32)
    base = np.stack([synth.frame(300 + i, FW, FH, int(camps[i])) for i in range(n)])
    scene = []
    for k in range(steps):                                  # four consecutive frames per stream: the stream's frame moved (5, 3) a step
        f = np.zeros_like(base)
        f[:, 3 * k:, 5 * k:] = base[:, :FH - 3 * k, :FW - 5 * k]
        scene.append(f)
    first = detect_all(oracle, scene[0], camps)
    assert all(len(r["armours"]) for r in first)
    origins = np.zeros((n, 2), np.int32)
    if ww:
        origins = np.array([W.window_origin(W.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (FW, FH)), ww, wh) for r in first], np.int32)
    trk = Tracker(device=0, n_streams=n, frame_w=FW, frame_h=FH, win_w=ww, win_h=wh)
    if ww:
        trk.set_origins(origins)
    trk.set_camps(camps)
    refs = [T.RefStream(T.lib(), cap=64, frame=(FW, FH), win=(ww, wh), origin=tuple(int(v) for v in origins[f])) for f in range(n)]
    dev = [torch.from_numpy(f).cuda() for f in scene]
    pl = Pipeline(device=0, hot_contexts=-1, max_frames=n, max_width=FW, max_height=FH)
    p = default_params()
    tracked = 0
    for k in range(steps):
        ts = (k + 1) * 8 * MS
        t = pl.submit(dev[k].data_ptr(), n, FH, FW, p, STAGE_ALL, tracker=trk, timestamp=ts)
        arm, offs = pl.collect(t)
        assert pl.get_info().host_blocking_calls == 0
        # the reference: every stream's tracker stepped with the ORACLE's detections of the stream's frame (its window) under the stream's camp
        req = np.array([r.origin for r in refs], np.int32)
        eff = W.effective_origins(req, FW, FH, ww, wh) if ww else np.zeros((n, 2), np.int32)
        imgs = np.stack([W.crop(scene[k][f], eff[f], ww, wh) for f in range(n)]) if ww else scene[k]
        det = detect_all(oracle, imgs, camps)
        assert arm.tobytes() == np.concatenate([r["armours"] for r in det]).tobytes(), k
        for f, r in enumerate(refs):
            assert r.step(abi.armours_to_frame(det[f]["armours"], int(eff[f][0]), int(eff[f][1])), None, None, ts), (k, f)
        same(trk, refs)
        tracked += sum(len(r.tracks) for r in refs)
    assert all(len(r.tracks) for r in refs) and tracked >= n * steps
    # the tracker's tables are what a context borrows too
    d_camps, d_lbs = trk.device_camps()
    assert d_camps and d_lbs
    c = Context(device=0, max_frames=n, max_width=FW, max_height=FH)
    c.upload(scene[0])
    c.set_frame_camps(d_camps)
    c.run(p, STAGE_ALL)
    c.sync()
    check_frames(c, first)
    c.close()
    # set_camps(None): off again -- the next tracked submit is detected with params.camp
    pl.drain()
    trk.set_camps(None)
    t = pl.submit(dev[0].data_ptr(), n, FH, FW, p, STAGE_ALL, tracker=trk, timestamp=99 * MS)
    pl.wait(t)
    assert np.array_equal(pl.context_of(t).frame_keys(), expected_keys([p.camp] * n, [p.lower_bound] * n))
    pl.close()
    trk.close()


# ---------------------------------------------------------------- 8. identity and pose ride along
def test_identity_and_pose_ride_along(oracle, mixed):
    frames, own, other = mixed
    svm = synth.svm_weights()
    stages = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)
    c.svm_load(*svm)
    c.pnp_load()
    c.upload(frames)
    c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))

    def results():
        c.sync()
        arm, offs = c.armours()
        ident = c.identities()
        r, t, p = c.poses()
        return [(arm[offs[f]:offs[f + 1]].tobytes(), ident[offs[f]:offs[f + 1]].tobytes(), c.icons(f).tobytes(), r[offs[f]:offs[f + 1]].tobytes(),
                 t[offs[f]:offs[f + 1]].tobytes(), p[offs[f]:offs[f + 1]].tobytes()) for f in range(N)]
    uniform = {}
    for camp in (0, 1):                                     # the path without keys, one colour for the whole batch
        c.run(default_params(camp=camp), stages)
        uniform[camp] = results()
    c.set_frame_camps(CAMPS)
    c.run(default_params(), stages)
    got = results()
    for f in range(N):
        assert got[f] == uniform[int(CAMPS[f])][f], f
        # ... and the oracle's: the classifier clamps an armour's icon in place (affine_correction), so the armours are the classified ones
        ri, ra, ricons = oracle.classify_armours(frames[f], own[f]["armours"], svm)
        assert got[f][0] == ra.tobytes() and got[f][1] == ri.tobytes() and got[f][2] == ricons.tobytes(), f
        assert np.array_equal(c.binary(f), own[f]["binary"]) and c.blobs(f)[0].tobytes() == own[f]["blobs"].tobytes(), f
    assert sum(len(g[1]) > 0 for g in got) == N and sum(got[f] != uniform[1 - int(CAMPS[f])][f] for f in range(N)) >= 8
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 9. refusals, and the way back
def test_refusals_and_return_to_per_run_keys(oracle, mixed):
    frames, own, other = mixed
    blue = [own[f] if CAMPS[f] == 1 else other[f] for f in range(N)]     # every frame under params.camp = BLUE
    c = Context(device=0, max_frames=N, max_width=FW, max_height=FH)

    def refused(call, word):
        with pytest.raises(RmcvError) as e:
            call()
        assert e.value.code == abi.ERR_BAD_ARG and word in str(e.value), str(e.value)

    def c_set(camps):
        a = np.ascontiguousarray(camps, np.int32)
        c._chk(abi.lib().rmcv_batch_set_frame_camps(c._h, abi.ptr(a), None))
    refused(lambda: c_set(CAMPS), "no frames bound")
    # a Bayer input format
    c.set_input_format(abi.BAYER_RG)
    c.upload(np.zeros((N, FH, FW), np.uint8))
    refused(lambda: c.set_frame_camps(CAMPS), "Bayer")
    c.set_input_format(abi.INPUT_BGR)
    # RMCV_OPT_ENHANCE
    c.set_enhance(True)
    c.upload(frames)
    refused(lambda: c.set_frame_camps(CAMPS), "ENHANCE")
    c.set_enhance(False)
    # the legacy matcher
    c.upload(frames)
    c.set_frame_camps(CAMPS)
    refused(lambda: c.run_legacy(LegacyParams(1.5, 80, 70, 10, 99999, 1), default_params(), STAGE_ALL), "legacy matcher")
    # ... and the context is usable: the keyed run, then back to per-run keys by set_frame_camps(None)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_frames(c, own)
    c.set_frame_camps(None)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_frames(c, blue)
    assert np.array_equal(c.frame_keys(), expected_keys([1] * N, [80] * N))
    # ... and by a new binding
    c.set_frame_camps(CAMPS)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_frames(c, blue)
    # a batch that takes k_binary_ws without keys does not with them, and does again after
    ws = abi.lib().rmcv_pixel_ws_launches
    c.set_option(abi.OPT_PIXEL_SHAPE, 1)
    n0 = ws()
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert ws() == n0 + 1                                   # (16 x 12 strips: more than half the CUs, contiguous rows -- the wave-specialised kernel)
    c.set_frame_camps(CAMPS)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert ws() == n0 + 1
    check_frames(c, own)
    c.set_frame_camps(None)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert ws() == n0 + 2
    check_frames(c, blue)
    assert c.check_guards()[0] == 0
    c.close()
