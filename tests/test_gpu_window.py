"""Windowed detection (rmcv_batch_set_windows / rmcv_pipeline_submit_windows) on the GPU.  The contract: every result for frame f equals,
bit for bit, what the CPU oracle gives for the cropped image frame[y_eff : y_eff + win_h, x_eff : x_eff + win_w] -- what the reference
computes on image(roi) -- with the effective origin of tests/window_ref.py (clamped into the frame, x snapped down to a multiple of 16).
Nothing has a tolerance.  NOT checked, because it does not hold: equality with whole-frame detection translated into the window."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import window_ref as R
from rmcv_amd import (CAMP_BLUE, CAMP_GUIDELIGHT, CAMP_RED, MORPH_CLOSE, MORPH_DILATE, MORPH_NONE, STAGE_ALL, STAGE_BINARY, STAGE_IDENTITY,
                      STAGE_NO_IMAGE, STAGE_POSE, Context, LegacyParams, Pipeline, RmcvError, default_params, synth)
from rmcv_amd import abi

pytestmark = pytest.mark.gpu


def oparams(oracle, p):
    return oracle.default_params(camp=p.camp, lower_bound=p.lower_bound, morph=p.morph)


def whole_frame_refs(oracle, frames, p=None):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda f: oracle.detect_frame(f, p or oracle.default_params()), frames))


def centred_origin(armour, fw, fh, win_w, win_h):
    """the requested origin of a window centred on an armour: GetROI of its vertices (scale 1), then rect centre minus half the window"""
    return R.window_origin(R.get_roi(armour["vertices"], (1.0, 1.0), (fw, fh)), win_w, win_h)


def first_armour_origins(oracle, frames, win_w, win_h):
    n, fh, fw, _ = frames.shape
    refs = whole_frame_refs(oracle, frames)
    assert all(len(r["armours"]) for r in refs)
    return np.array([centred_origin(r["armours"][0], fw, fh, win_w, win_h) for r in refs], np.int32), refs


def mixed_origins(rng, centres, fw, fh, win_w, win_h):
    """a third anywhere from far left / above to far right / below the frame (negative, past the edge), the others around a target;
    none aligned on purpose"""
    out = []
    for i, (cx, cy) in enumerate(centres):
        if i % 3 == 0:
            out.append((int(rng.integers(-400, fw + 400)), int(rng.integers(-400, fh + 400))))
        else:
            out.append((cx - win_w // 2 + int(rng.integers(-120, 121)), cy - win_h // 2 + int(rng.integers(-90, 91))))
    return np.array(out, np.int32)


def crops_of(frames, eff, win_w, win_h):
    return [R.crop(frames[f], eff[f], win_w, win_h) for f in range(len(frames))]


def check_windows(c, frames, origins, win_w, win_h, oracle, p=None, image=True):
    """the context's batch (already run and synced) against the oracle on every frame's crop; returns (crops, refs, effective origins)"""
    n, fh, fw, _ = frames.shape
    eff = R.effective_origins(origins, fw, fh, win_w, win_h)
    got_eff, gw, gh = c.windows()
    assert (gw, gh) == (win_w, win_h) and np.array_equal(got_eff, eff), (got_eff.tolist(), eff.tolist())
    assert not (eff[:, 0] % 16).any() and (eff >= 0).all() and (eff[:, 0] <= fw - win_w).all() and (eff[:, 1] <= fh - win_h).all()
    crops = crops_of(frames, eff, win_w, win_h)
    op = oparams(oracle, p) if p is not None else oracle.default_params()
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda img: oracle.detect_frame(img, op), crops))
    arm, aoffs = c.armours()
    assert not (c.counts()["status"] & 15).any()
    for f, ref in enumerate(refs):
        if image:
            b = c.binary(f)
            assert b.shape == (win_h, win_w) and np.array_equal(b, ref["binary"]), f
        pts, offs = c.contours(f)
        assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), f
        assert c.blobs(f)[0].tobytes() == ref["blobs"].tobytes(), f
        assert arm[aoffs[f]:aoffs[f + 1]].tobytes() == ref["armours"].tobytes(), f
    return crops, refs, eff


def edge_foreground(binary):
    return bool(binary[0].any() or binary[-1].any() or binary[:, 0].any() or binary[:, -1].any())


def bind(c, frames, stride):
    """frames in HBM: uploaded, or -- with a stride -- a torch buffer with padded rows"""
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


# ---------------------------------------------------------------- 1. the tracked-ROI batch
def test_windows_centred_on_the_first_armour(oracle):
    n, fw, fh, ww, wh = 64, 1280, 1024, 512, 384
    frames = synth.batch(0, n, fw, fh, CAMP_BLUE, 0, threads=16)
    origins, whole = first_armour_origins(oracle, frames, ww, wh)
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    assert c.shape == (n, wh, ww)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    crops, refs, eff = check_windows(c, frames, origins, ww, wh, oracle)
    # not vacuous: every window holds an armour, and a good number of them cut foreground at a window edge
    assert sum(len(r["armours"]) > 0 for r in refs) >= 64
    assert sum(edge_foreground(r["binary"]) for r in refs) >= 8
    # the origins really are per frame, and the snap really acts
    assert len({tuple(e) for e in eff.tolist()}) > 8 and (origins[:, 0] % 16 != 0).any()
    # frame coordinates are a convenience: one f32 add, equal to numpy's
    arm, aoffs = c.armours()
    for f in (0, 17, 63):
        a = arm[aoffs[f]:aoffs[f + 1]]
        moved = c.armours_to_frame(a, eff[f][0], eff[f][1])
        assert np.array_equal(moved["vertices"], a["vertices"] + eff[f].astype(np.float32))
    # back to whole frames on the same binding
    c.set_windows(None, 0, 0)
    assert c.shape == (n, fh, fw) and c.windows()[1:] == (0, 0)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    arm, aoffs = c.armours()
    for f in (0, 31, 63):
        assert np.array_equal(c.binary(f), whole[f]["binary"]) and arm[aoffs[f]:aoffs[f + 1]].tobytes() == whole[f]["armours"].tobytes()
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 2. origins of any value, window sizes, frame geometries
GEOMS = [("1920x1200", 1920, 1200, None, [(640, 512), (384, 256), (64, 32), (200, 150), (1920, 1200)]),
         ("1280x1024 padded stride", 1280, 1024, 3 * 1280 + 64, [(640, 512), (384, 256), (64, 32), (200, 150), (1280, 1024)])]


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_random_origins_window_sizes_and_geometries(oracle, geom):
    _, fw, fh, stride, sizes = geom
    n = 12
    frames = synth.batch(700, n, fw, fh, CAMP_BLUE, 0, threads=16)
    whole = whole_frame_refs(oracle, frames)
    centres = []
    for r in whole:
        x, y, w, h = R.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (fw, fh)) if len(r["armours"]) else (fw // 2, fh // 2, 0, 0)
        centres.append((x + w // 2, y + h // 2))
    rng = np.random.default_rng(fw)
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    keep = bind(c, frames, stride)
    found = 0
    for k, (ww, wh) in enumerate(sizes):
        origins = mixed_origins(rng, centres, fw, fh, ww, wh)
        origins[1] = (-7, -3)                           # negative: clamps to (0, 0)
        origins[2] = (fw + 5, fh + 5)                   # past the edge: clamps to the last position, then snaps
        origins[4] = (fw - ww - 1 if fw > ww else 0, 9)  # one short of the last position: unaligned unless the window is the frame
        if k % 2 == 0:
            c.set_windows(origins, ww, wh)
            dev = None
        else:                                           # the origins in device memory, borrowed
            import torch
            dev = torch.from_numpy(origins).cuda()
            c.set_windows(dev.data_ptr(), ww, wh, keepalive=dev)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        crops, refs, eff = check_windows(c, frames, origins, ww, wh, oracle)
        assert tuple(eff[1]) == (0, 0) and tuple(eff[2]) == ((fw - ww) & ~15, fh - wh)
        found += sum(len(r["armours"]) for r in refs)
        if dev is not None:                             # rewritten on the device behind the host's back: the next run reads them again
            dev += 48
            torch.cuda.synchronize()
            c.run(default_params(), STAGE_ALL)
            c.sync()
            check_windows(c, frames, origins + 48, ww, wh, oracle)
        assert c.check_guards()[0] == 0
    assert found > 0
    c.close()
    del keep


# ---------------------------------------------------------------- 3. every morph, camp, bound; no byte image
@pytest.mark.parametrize("size", [(384, 256), (200, 150)], ids=["row quads", "byte-wise"])
def test_every_morph_camp_bound_and_no_image(oracle, size):
    ww, wh = size
    n, fw, fh = 8, 1280, 1024
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    rng = np.random.default_rng(31)
    for camp in (CAMP_BLUE, CAMP_RED, CAMP_GUIDELIGHT):
        frames = synth.batch(800 + camp, n, fw, fh, CAMP_RED if camp == CAMP_RED else CAMP_BLUE, 0, threads=16)
        whole = whole_frame_refs(oracle, frames, oracle.default_params(camp=CAMP_RED if camp == CAMP_RED else CAMP_BLUE))
        centres = []
        for r in whole:
            assert len(r["armours"])
            x, y, w, h = R.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (fw, fh))
            centres.append((x + w // 2, y + h // 2))
        c.upload(frames)
        for morph in (MORPH_NONE, MORPH_DILATE, MORPH_CLOSE):
            origins = mixed_origins(rng, centres, fw, fh, ww, wh)
            c.set_windows(origins, ww, wh)
            p = default_params(camp=camp, lower_bound=80, morph=morph)
            c.run(p, STAGE_ALL)
            c.sync()
            crops, refs, eff = check_windows(c, frames, origins, ww, wh, oracle, p)
            if camp != CAMP_GUIDELIGHT:
                assert sum(r["binary"].any() for r in refs) >= 4, (camp, morph)
            # without the byte image: the same contours, blobs and armours
            c.run(p, STAGE_ALL | STAGE_NO_IMAGE)
            c.sync()
            check_windows(c, frames, origins, ww, wh, oracle, p, image=False)
            # lower_bound <= 0: everything passes (the pixel stage alone: the window is one blob)
            for lb in (0, -1):
                c.run(default_params(camp=camp, lower_bound=lb, morph=morph), STAGE_BINARY)
                c.sync()
                for f in (0, n - 1):
                    want = oracle.extract_binary(crops[f], camp, lb, morph)
                    assert want.all() and np.array_equal(c.binary(f), want), (camp, morph, lb, f)
        assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 4. + 5. identity and pose
def test_identity_and_pose_on_windows(oracle):
    n, fw, fh, ww, wh = 16, 1920, 1200, 512, 384
    svm = synth.svm_weights()
    frames = synth.batch(400, n, fw, fh, CAMP_BLUE, 0, threads=16)
    origins, _ = first_armour_origins(oracle, frames, ww, wh)
    origins[::4] += (37, -140)        # some windows cut their armour: icons that leave the window are clamped to win_w - 1, win_h - 1
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    c.svm_load(*svm)
    c.pnp_load()
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    c.sync()
    eff = R.effective_origins(origins, fw, fh, ww, wh)
    assert np.array_equal(c.windows()[0], eff)
    crops = crops_of(frames, eff, ww, wh)
    arm, offs = c.armours()
    ident = c.identities()
    r, t, p = c.poses()
    assert len(arm) >= n // 2
    ocfg = oracle.default_pnp_config()
    clamped = 0
    for f in range(n):
        a0 = oracle.detect_frame(crops[f], oracle.default_params())["armours"]
        ri, ra, ricons = oracle.classify_armours(crops[f], a0, svm)       # affine_correction on the crop: clamps to ITS size
        sl = slice(offs[f], offs[f + 1])
        assert arm[sl].tobytes() == ra.tobytes(), f
        assert np.array_equal(ident[sl], ri) and np.array_equal(c.icons(f), ricons), f
        clamped += int((ra["icon"] != a0["icon"]).any()) if len(a0) else 0
        # mobility.cpp:172, 182-185: every image point + ((float)roi.x, (float)roi.y), added in float
        moved = a0.copy()
        moved["vertices"] = a0["vertices"] + eff[f].astype(np.float32)
        wr, wt, wp = oracle.locate_armours(moved, ocfg, np.eye(4))
        assert r[sl].tobytes() == wr.tobytes() and t[sl].tobytes() == wt.tobytes() and p[sl].tobytes() == wp.tobytes(), f
        if len(a0) and eff[f].any():                                      # ... and the offset matters
            assert oracle.locate_armours(a0, ocfg, np.eye(4))[1].tobytes() != wt.tobytes()
    assert clamped >= 1                                                   # some icon did leave its window
    # the stage-wise pose call keeps the default ROI whatever windows the context has
    a0 = oracle.detect_frame(crops[1], oracle.default_params())["armours"]
    gr, gt, gp = c.locate_armours(a0)
    wr, wt, wp = oracle.locate_armours(a0, ocfg, None)
    assert gr.tobytes() == wr.tobytes() and gt.tobytes() == wt.tobytes()
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 6. the legacy matcher
@pytest.mark.parametrize("fit_ellipse", [True, False])
def test_legacy_run_on_windows(oracle, fit_ellipse):
    n, fw, fh, ww, wh = 8, 1280, 1024, 512, 384
    frames = synth.batch(300, n, fw, fh, CAMP_BLUE, 1, threads=16)
    origins, _ = first_armour_origins(oracle, frames, ww, wh)
    origins[1::2] += (-61, 33)
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    c.upload(frames)
    c.set_windows(origins, ww, wh)
    lp = LegacyParams(1.5, 80, 70, 10, 99999, int(fit_ellipse))
    c.run_legacy(lp, default_params(), STAGE_ALL)
    c.sync()
    eff = R.effective_origins(origins, fw, fh, ww, wh)
    assert np.array_equal(c.windows()[0], eff)
    arm, aoffs = c.armours()
    total, camps = 0, set()
    for f in range(n):
        crop = R.crop(frames[f], eff[f], ww, wh)
        ref = oracle.detect_frame(crop, oracle.default_params())
        ob, _, _ = oracle.find_lightblobs(crop, ref["pts"], ref["offs"], 1.5, 80, 70, 10, 99999, fit_ellipse)   # the camp voted from the CROP's means
        gb, _ = c.blobs(f)
        assert gb.tobytes() == ob.tobytes(), f
        oa = oracle.filter_armours(ob, oracle.default_params())                        # pairs the blobs of the enemy camp
        assert arm[aoffs[f]:aoffs[f + 1]].tobytes() == oa.tobytes(), f
        total += len(ob)
        camps |= set(int(v) for v in ob["target"])
    assert total >= n and len(camps) >= 1
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 7. the pipeline
def test_pipeline_interleaves_windowed_and_whole_frame_batches(oracle):
    import torch
    n, fw, fh = 32, 1280, 1024
    p = default_params()
    frames = synth.batch(100, n, fw, fh, CAMP_BLUE, 0, threads=16)
    whole = whole_frame_refs(oracle, frames)
    want_whole = np.concatenate([r["armours"] for r in whole]).tobytes()
    sizes = [(512, 384), (256, 192), (200, 150)]
    rng = np.random.default_rng(77)
    centres = []
    for r in whole:
        x, y, w, h = R.get_roi(r["armours"][0]["vertices"], (1.0, 1.0), (fw, fh))
        centres.append((x + w // 2, y + h // 2))
    sets = {}
    for k, (ww, wh) in enumerate(sizes):
        o = mixed_origins(rng, centres, fw, fh, ww, wh)
        eff = R.effective_origins(o, fw, fh, ww, wh)
        with ThreadPoolExecutor(16) as ex:
            refs = list(ex.map(lambda img: oracle.detect_frame(img, oracle.default_params()), crops_of(frames, eff, ww, wh)))
        sets[k] = (torch.from_numpy(o).cuda(), eff, refs)
    assert sum(len(r["armours"]) for r in sets[0][2]) >= n // 2
    dev = torch.from_numpy(frames).cuda()
    pl = Pipeline(device=0, max_frames=n, max_width=fw, max_height=fh)
    # whole-frame batches long enough for the hot rotation to start, windows in between, sizes changing from batch to batch
    order = [None] * 6 + [0] * 4 + [None, 1, None, 2, 0, 1] + [None] * 4 + [0, 0]
    tickets, got, hot_seen = [], {}, []
    lag = pl.depth - 1

    def check(i):
        arm, offs = got[i]
        k = order[i]
        if k is None:
            assert arm.tobytes() == want_whole, i
            return
        refs = sets[k][2]
        assert arm.tobytes() == np.concatenate([r["armours"] for r in refs]).tobytes(), (i, k)
        assert list(np.diff(offs)) == [len(r["armours"]) for r in refs], (i, k)

    for i, k in enumerate(order):
        before = pl.get_info().hot_batches
        if k is None:
            tickets.append(pl.submit(dev.data_ptr(), n, fh, fw, p, STAGE_ALL))
        else:
            tickets.append(pl.submit(dev.data_ptr(), n, fh, fw, p, STAGE_ALL, windows=(sets[k][0].data_ptr(), sizes[k][0], sizes[k][1])))
        hot_seen.append((k, pl.get_info().hot_batches - before))
        if i >= lag:
            got[i - lag] = pl.collect(tickets[i - lag])
    pl.drain()
    for i in range(max(0, len(order) - lag), len(order)):
        got[i] = pl.collect(tickets[i])
    for i in range(len(order)):
        check(i)
    info = pl.get_info()
    assert info.host_blocking_calls == 0
    assert all(grew == 0 for k, grew in hot_seen if k is not None)      # windowed batches stay out of the hot rotation
    # the per-stage getters of a windowed ticket: window-sized images, the effective origins
    t = pl.submit(dev.data_ptr(), n, fh, fw, p, STAGE_ALL, windows=(sets[0][0].data_ptr(), 512, 384))
    pl.wait(t)
    cx = pl.context_of(t)
    assert np.array_equal(cx.windows()[0], sets[0][1]) and cx.windows()[1:] == (512, 384)
    for f in (0, n - 1):
        assert np.array_equal(cx.binary(f), sets[0][2][f]["binary"])
        pts, offs = cx.contours(f)
        assert np.array_equal(pts, sets[0][2][f]["pts"]) and np.array_equal(offs, sets[0][2][f]["offs"])
    # refusals leave the pipeline usable: a window larger than the frames, null origins
    for bad in ((sets[0][0].data_ptr(), fw + 16, 64), (sets[0][0].data_ptr(), 64, fh + 1), (sets[0][0].data_ptr(), 0, 0), (0, 64, 64)):
        with pytest.raises(RmcvError) as e:
            pl.submit(dev.data_ptr(), n, fh, fw, p, STAGE_ALL, windows=bad)
        assert e.value.code == abi.ERR_BAD_ARG
    arm, offs = pl.collect(pl.submit(dev.data_ptr(), n, fh, fw, p, STAGE_ALL))
    assert arm.tobytes() == want_whole
    assert pl.get_info().host_blocking_calls == 0
    for c in pl.contexts:
        assert c.check_guards()[0] == 0
    pl.close()


# ---------------------------------------------------------------- 8. the locked-target loop
def test_closed_loop_on_a_moving_target(oracle):
    fw, fh, ww, wh = 1280, 1024, 512, 384
    src = synth.frame(5, fw, fh)
    a = oracle.detect_frame(src, oracle.default_params())["armours"]
    assert len(a)
    x, y, w, h = R.get_roi(a[0]["icon"], (1.0, 1.0), (fw, fh))
    pad = 24
    patch = src[max(0, y - pad):y + h + pad, max(0, x - pad):x + w + pad].copy()
    ph, pw, _ = patch.shape
    steps = [(100, 80), (163, 131), (259, 167), (371, 252)]            # where the target's patch sits, frame by frame
    frames = np.zeros((len(steps), fh, fw, 3), np.uint8)
    for k, (px, py) in enumerate(steps):
        frames[k, py:py + ph, px:px + pw] = patch
    c = Context(device=0, max_frames=1, max_width=fw, max_height=fh)
    # step 0: the whole frame
    c.upload(frames[:1])
    c.run(default_params(), STAGE_ALL)
    c.sync()
    arm, _ = c.armours()
    ref = oracle.detect_frame(frames[0], oracle.default_params())
    assert len(arm) and arm.tobytes() == ref["armours"].tobytes()
    prev = (0, 0, 0, 0)
    for k in range(1, len(steps)):
        # detect -> GetROI (scale 2, relative to the window the armour was found in) -> window -> detect
        rect = c.get_roi(arm[0]["vertices"], 2.0, (fw, fh), prev)
        assert rect == R.get_roi(arm[0]["vertices"], (2.0, 2.0), (fw, fh), prev) and rect[2] > 0
        origin = c.window_origin(rect, ww, wh)
        assert origin == R.window_origin(rect, ww, wh)
        c.upload(frames[k:k + 1])
        c.set_windows([origin], ww, wh)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        crops, refs, eff = check_windows(c, frames[k:k + 1], [origin], ww, wh, oracle)
        arm, _ = c.armours()
        assert len(arm) >= 1, k                                         # the target stays locked
        prev = (int(eff[0][0]), int(eff[0][1]), ww, wh)
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_context_usable(oracle):
    n, fw, fh = 2, 1280, 1024
    frames = synth.batch(0, n, fw, fh, CAMP_BLUE, 0)
    origins = np.array([[300, 200], [555, 444]], np.int32)
    c = Context(device=0, max_frames=n, max_width=fw, max_height=fh)

    def usable():
        c.upload(frames)
        c.set_windows(origins, 512, 384)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        check_windows(c, frames, origins, 512, 384, oracle)

    def refused(call, word):
        with pytest.raises(RmcvError) as e:
            call()
        assert e.value.code == abi.ERR_BAD_ARG and word in str(e.value), str(e.value)
    fresh = Context(device=0, max_frames=n, max_width=fw, max_height=fh)
    refused(lambda: abi_set(fresh, origins, 512, 384), "no frames bound")
    fresh.close()
    usable()
    # a Bayer input format
    c.set_input_format(abi.BAYER_RG)
    c.upload(np.zeros((n, fh, fw), np.uint8))
    refused(lambda: c.set_windows(origins, 512, 384), "Bayer")
    c.set_input_format(abi.INPUT_BGR)
    usable()
    # RMCV_OPT_ENHANCE
    c.set_enhance(True)
    c.upload(frames)
    refused(lambda: c.set_windows(origins, 512, 384), "ENHANCE")
    c.set_enhance(False)
    usable()
    # sizes: below 1, larger than the frames (which the context's limits bound in turn)
    c.upload(frames)
    for ww, wh in ((-1, 64), (64, 0), (fw + 1, 64), (64, fh + 1), (1 << 20, 1 << 20)):
        refused(lambda: c.set_windows(origins, ww, wh), "window size")
    assert c.windows()[1:] == (0, 0)                                   # nothing moved: still whole frames
    big = Context(device=0, max_frames=n, max_width=1920, max_height=1200)
    big.upload(frames)
    refused(lambda: big.set_windows(origins, 1920, 1200), "larger than the frames")
    big.close()
    L = abi.lib()
    assert L.rmcv_batch_set_windows(c._h, None, 64, 64) == abi.ERR_BAD_ARG and L.rmcv_batch_set_device_windows(c._h, None, 64, 64) == abi.ERR_BAD_ARG
    usable()
    assert c.check_guards()[0] == 0
    c.close()


def abi_set(c, origins, ww, wh):
    o = np.ascontiguousarray(origins, np.int32)
    c._chk(abi.lib().rmcv_batch_set_windows(c._h, abi.ptr(o), ww, wh))


# ---------------------------------------------------------------- the shim: GetROI -> extract_color(image(roi)) -> solve_PnP(..., roi)
def test_shim_locked_target_step(tmp_path, oracle):
    from test_window_cpu import build_shim_window
    import subprocess
    _, exe = build_shim_window(str(tmp_path))
    fw, fh = 1280, 1024
    ocfg = oracle.default_pnp_config()
    for index in (0, 5):
        out = subprocess.run([exe, str(index)], check=True, capture_output=True, text=True, timeout=180).stdout.strip().splitlines()
        frame = synth.frame(index, fw, fh)
        whole = oracle.detect_frame(frame, oracle.default_params())["armours"]
        v = whole[0]["vertices"]
        rects = [int(t) for t in out[0].split() if t.lstrip("-").isdigit()]
        assert tuple(rects[0:4]) == R.get_roi(v) == (0, 0, 0, 0)
        assert tuple(rects[4:8]) == R.get_roi(v, (1.0, 1.0), (fw, fh))
        roi = R.get_roi(v, (2.0, 2.0), (fw, fh))
        assert tuple(rects[8:12]) == roi and roi[2] > 0 and roi[3] > 0
        x, y, w, h = roi                                          # the reference's ROI: no clamp, no snap -- a sub-view is any rectangle
        crop = np.ascontiguousarray(frame[y:y + h, x:x + w])
        ref = oracle.detect_frame(crop, oracle.default_params())
        head = dict(zip(out[1].split()[0::2], map(int, out[1].split()[1::2])))
        assert head["contours"] == len(ref["offs"]) - 1 and head["points"] == len(ref["pts"]) and head["binary_on"] == int(np.count_nonzero(ref["binary"]))
        assert head["positive"] == len(ref["blobs"]) and head["armours"] == len(ref["armours"]) and len(ref["armours"]) > 0
        got = [[float.fromhex(t) for t in ln.split()[1:]] for ln in out if ln.startswith("armour")]
        moved = ref["armours"].copy()
        moved["vertices"] = ref["armours"]["vertices"] + np.array([x, y], np.float32)
        wr, wt, _ = oracle.locate_armours(moved, ocfg, None)
        for k, a in enumerate(ref["armours"]):
            assert got[k][:8] == [float(t) for t in a["vertices"].reshape(-1)], (index, k)       # window coordinates
            assert got[k][8:11] == list(wr[k]) and got[k][11:14] == list(wt[k]), (index, k)      # the pose of the frame-coordinate points
