"""Exposure-adaptive detection (RMCV_OPT_ENHANCE: rm::AutoEnhance fused into the pixel pass) on the GPU.  The contract: with the option
on, every result for a frame f equals, bit for bit, what the same call gives for E(f) (tests/enhance_ref.py: numpy + the host libm) with
the option off -- so the CPU oracle, run on E(f), checks every stage, and so does the same context's plain call on E(f).  The inputs
that tell a working implementation from one that merely accepts the option are the dimmed frames (tests/test_enhance_cpu.py
test_dimmed_frames_tell_the_paths_apart: at 80/256 the plain path finds no armour on any of them)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import enhance_ref as R
from rmcv_amd import (CAMP_BLUE, CAMP_GUIDELIGHT, CAMP_RED, MORPH_CLOSE, MORPH_DILATE, MORPH_NONE, OPT_CONTOUR_TIER, OPT_FRAME_UPLOAD,
                      OPT_RUN_AHEAD, STAGE_ALL, STAGE_BINARY, STAGE_IDENTITY, STAGE_NO_IMAGE, STAGE_POSE, Context, LegacyParams,
                      Pipeline, RmcvError, default_params, synth)
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "rmcv_amd", "lib")


def bright(frame):
    """a frame whose meanC3 is above 50: gamma > 1 with the default gains"""
    return np.minimum(frame.astype(np.uint16) + 70, 255).astype(np.uint8)


def mixed(first, n, w, h, camp=CAMP_BLUE):
    """n frames of mixed exposure: dimmed to 80/256 and 96/256, as they are, brightened (gamma > 1), one all black (gamma 0.5) and one
    all 255 (gamma 9.2)"""
    fr = synth.batch(first, n, w, h, camp, 0, threads=16)
    out = np.empty_like(fr)
    for f in range(n):
        k = f % 6
        out[f] = R.dim(fr[f], 80) if k in (0, 4) else R.dim(fr[f], 96) if k == 1 else fr[f] if k == 2 else bright(fr[f]) if k == 3 else fr[f]
    if n > 5:
        out[5] = 0
    if n > 6:
        out[n - 1] = 255
    return out


def enhanced(frames, gains=(100.0, 50.0)):
    with ThreadPoolExecutor(16) as ex:
        r = list(ex.map(lambda f: R.E(f, *gains), frames))
    return np.stack([x[0] for x in r]), np.array([x[1] for x in r], np.float32)


def chain(ctx, img, camp=CAMP_BLUE, lb=80, morph=MORPH_CLOSE):
    pts, offs, binary = ctx.extract_color_csr(img, camp, lb, morph)
    blobs, src, neg = ctx.filter_lightblobs(pts, offs, enemy=camp)
    arm = ctx.filter_armours(blobs, enemy=camp)
    return binary, pts, offs, blobs, src, neg, arm


def frame_results(c, n, image=True):
    """everything a batch run left, as bytes: per frame (binary, points, offsets, blobs), then armours and their frame offsets"""
    out = []
    for f in range(n):
        pts, offs = c.contours(f)
        out.append(((c.binary(f).tobytes() if image else b""), pts.tobytes(), offs.tobytes(), c.blobs(f)[0].tobytes()))
    arm, aoffs = c.armours()
    return out, arm.tobytes(), aoffs.tobytes()


def check_against_oracle(c, frames_e, oracle, p=None, image=True):
    arm, aoffs = c.armours()
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda f: oracle.detect_frame(f, p or oracle.default_params()), frames_e))
    for f, ref in enumerate(refs):
        if image:
            assert np.array_equal(c.binary(f), ref["binary"]), f
        pts, offs = c.contours(f)
        assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), f
        assert c.blobs(f)[0].tobytes() == ref["blobs"].tobytes(), f
        assert arm[aoffs[f]:aoffs[f + 1]].tobytes() == ref["armours"].tobytes(), f
    return refs


# ---------------------------------------------------------------- 1. the stand-alone calls
def test_auto_enhance_and_calc_gamma_bytes():
    c = Context(device=0, max_frames=1, max_width=1920, max_height=1200)
    L = lib()
    rng = np.random.default_rng(5)
    f0 = synth.frame(0)
    cases = [("dim80", R.dim(f0, 80), 3840), ("dim96 padded", R.dim(f0, 96), 3840 + 52), ("as it is", f0, 3840), ("bright", bright(f0), 3840),
             ("black", np.zeros((40, 64, 3), np.uint8), 192), ("white", np.full((33, 64, 3), 255, np.uint8), 200),
             ("odd 1283x3", rng.integers(0, 90, (3, 1283, 3), dtype=np.uint8), 3 * 1283), ("odd padded", rng.integers(0, 256, (3, 1283, 3), dtype=np.uint8), 3 * 1283 + 7),
             ("1x1", np.array([[[7, 9, 200]]], np.uint8), 3), ("noise 1920x1200", rng.integers(0, 256, (1200, 1920, 3), dtype=np.uint8), 5760)]
    for name, img, stride in cases:
        h, w, _ = img.shape
        for gains in ((100.0, 50.0), (30.0, 5.0), (2.0, 1.0)):  # (2, 1): gammas up to 509, far beyond where pow(1 / 255, g) is a normal double
            want, g = R.E(img, *gains)
            src = np.full((h, stride), 77, np.uint8)
            src[:, :3 * w] = img.reshape(h, 3 * w)
            out = np.full((h, stride + 5), 7, np.uint8)
            gout = C.c_float(-1)
            rc = L.rmcv_auto_enhance(c._h, ptr(src), w, h, stride, C.c_float(gains[0]), C.c_float(gains[1]), ptr(out), stride + 5, C.byref(gout))
            assert rc == 0, (name, L.rmcv_last_error(c._h))
            assert np.float32(gout.value).tobytes() == np.float32(g).tobytes(), (name, gains, gout.value, g)
            assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), want), (name, gains)
            assert np.all(out[:, 3 * w:] == 7)            # the row padding of the output is left alone
            assert np.array_equal(src[:, :3 * w].reshape(h, w, 3), img) and np.all(src[:, 3 * w:] == 77)
            # in place
            rc = L.rmcv_auto_enhance(c._h, ptr(src), w, h, stride, C.c_float(gains[0]), C.c_float(gains[1]), ptr(src), stride, None)
            assert rc == 0 and np.array_equal(src[:, :3 * w].reshape(h, w, 3), want) and np.all(src[:, 3 * w:] == 77), (name, gains)
        # rm::CalcGamma: any channel count (the table acts on bytes)
        for gamma in (0.0, 0.5, 0.5713445, 1.0, 2.2, 9.2, 129.0, 400.0, 1000.0, 1e30):
            want = R.calc_gamma(img, gamma)
            assert np.array_equal(c.calc_gamma(img, gamma), want), (name, gamma)
            one = np.ascontiguousarray(img[:, :, 1])
            assert np.array_equal(c.calc_gamma(one, gamma), R.calc_gamma(one, gamma)), (name, gamma)
        src = np.full((h, stride), 77, np.uint8)
        src[:, :3 * w] = img.reshape(h, 3 * w)
        assert L.rmcv_calc_gamma(c._h, ptr(src), 3 * w, h, stride, C.c_float(2.2), ptr(src), stride) == 0
        assert np.array_equal(src[:, :3 * w].reshape(h, w, 3), R.calc_gamma(img, 2.2)) and np.all(src[:, 3 * w:] == 77), name
    e, g = c.auto_enhance(R.dim(f0, 80))
    assert np.array_equal(e, R.E(R.dim(f0, 80))[0]) and 0.56 < g < 0.58
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 2. the per-frame chain
@pytest.mark.parametrize("run_ahead", [0, 1])
@pytest.mark.parametrize("upload", [0, 1, 2])
def test_chain_equals_plain_chain_on_enhanced_frame(oracle, run_ahead, upload):
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    c.set_option(OPT_RUN_AHEAD, run_ahead)
    c.set_option(OPT_FRAME_UPLOAD, upload)
    fr = synth.batch(0, 4, 1280, 1024, CAMP_BLUE, 0)
    inputs = [R.dim(fr[0], 80), R.dim(fr[1], 80), R.dim(fr[2], 80), R.dim(fr[3], 96), fr[0], bright(fr[1]), np.zeros_like(fr[0]), np.full_like(fr[0], 255)]
    keep = []  # upload mode 2 pins the caller's buffers in place: they must outlive the context
    found = 0
    for i, img in enumerate(inputs):
        e, g = R.E(img)
        keep += [img, e]
        c.set_enhance(True)
        got = chain(c, img)
        assert c.gammas()[0].tobytes() == np.float32(g).tobytes(), i
        c.set_enhance(False)
        plain = chain(c, e)
        assert c.gammas()[0] == 1.0
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes(), i
        ref = oracle.detect_frame(e, oracle.default_params())
        assert np.array_equal(got[0], ref["binary"]) and np.array_equal(got[2], ref["offs"]) and np.array_equal(got[1], ref["pts"]), i
        assert got[3].tobytes() == ref["blobs"].tobytes() and got[6].tobytes() == ref["armours"].tobytes(), i
        if i < 3:  # the discriminating inputs: the plain path finds nothing on the frame itself
            assert len(chain(c, img)[6]) == 0 and len(got[6]) > 0, i
            found += len(got[6])
    assert found == 4 + 1 + 1
    assert c.check_guards()[0] == 0
    c.close()
    del keep


# ---------------------------------------------------------------- 3. batches
GEOMS = [("linear", 1280, 1024, None), ("row quads", 1280, 1024, 3 * 1280 + 64), ("byte-wise", 1283, 1021, None), ("linear 1920", 1920, 1200, None)]


def bind(c, frames, stride):
    """frames in HBM: uploaded (rows 3 w rounded up to 16 bytes apart), or -- with a stride -- a torch buffer with padded rows"""
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


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_batch_mixed_brightness(oracle, geom):
    _, w, h, stride = geom
    n = 14
    frames = mixed(100, n, w, h)
    fe, gam = enhanced(frames)
    assert gam.min() == 0.5 and 9.19 < gam.max() < 9.21 and (gam > 1).sum() >= 3 and len(set(gam.tolist())) >= 8  # each frame its own gamma
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.set_enhance(True)
    keep = bind(c, frames, stride)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert c.gammas().tobytes() == gam.tobytes()
    refs = check_against_oracle(c, fe, oracle)
    on = frame_results(c, n)
    # the dimmed frames are the ones that tell: the plain path on the frames themselves finds fewer armours
    c.set_enhance(False)
    keep = bind(c, frames, stride)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    plain_arm, plain_offs = c.armours()
    assert np.all(c.gammas() == 1.0)
    for f in (0, 4, 6, 10):
        assert plain_offs[f + 1] - plain_offs[f] == 0
    assert sum(len(refs[f]["armours"]) for f in (0, 4, 6, 10)) > 0
    # ... and the plain path on E(f) is the enhanced path on f
    keep = bind(c, fe, stride)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert frame_results(c, n) == on
    assert c.check_guards()[0] == 0
    c.close()
    del keep


@pytest.mark.parametrize("geom", GEOMS[:3], ids=[g[0] for g in GEOMS[:3]])
def test_batch_every_morph_bound_camp_tier_and_no_image(geom):
    """the same context, option on over f against option off over E(f): every morph, lb in {-1, 1, 80, 255}, the three camps, the
    three forms of findContours, with and without the byte image"""
    _, w, h, stride = geom
    n = 8
    c = Context(device=0, max_frames=n, max_width=w, max_height=h, max_contours=1 << 15, max_points=1 << 19, max_blobs=1 << 12)
    for camp in (CAMP_BLUE, CAMP_RED, CAMP_GUIDELIGHT):
        frames = mixed(200 + camp, n, w, h, CAMP_RED if camp == CAMP_RED else CAMP_BLUE)
        fe, gam = enhanced(frames)
        for morph in (MORPH_NONE, MORPH_DILATE, MORPH_CLOSE):
            for lb in (-1, 1, 80, 255):
                p = default_params(camp=camp, lower_bound=lb, morph=morph)
                # (lb -1 and 1 light most of the frame, tens of thousands of specks: the pixel stage alone, which is where the bound acts)
                stages = STAGE_ALL if lb >= 80 else STAGE_BINARY
                tiers = (0, 1, 2) if (lb == 80 and morph == MORPH_CLOSE) else (0,)
                for tier in tiers:
                    for no_image in ((0, STAGE_NO_IMAGE) if lb == 80 else (0,)):
                        res = []
                        for on, src in ((True, frames), (False, fe)):
                            c.set_option(OPT_CONTOUR_TIER, tier)
                            c.set_enhance(on)
                            keep = bind(c, src, stride)
                            c.run(p, stages | no_image)
                            c.sync()
                            r = [] if no_image else [c.binary(f).tobytes() for f in range(n)]
                            if stages == STAGE_ALL:
                                cnt = c.counts()
                                assert not (cnt["status"] & 15).any()
                                r += [cnt["n_contours"].tobytes(), cnt["n_points"].tobytes(), frame_results(c, n, image=False)]
                            res.append(r)
                            if on:
                                assert c.gammas().tobytes() == gam.tobytes()
                        assert res[0] == res[1], (camp, morph, lb, tier, no_image)
    c.set_option(OPT_CONTOUR_TIER, 0)
    assert c.check_guards()[0] == 0
    c.close()


def test_batch_gains_of_the_context():
    n, w, h = 8, 1280, 1024
    frames = mixed(300, n, w, h)
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.set_enhance(True, 30.0, 5.0)
    c.upload(frames)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    fe, gam = enhanced(frames, (30.0, 5.0))
    assert c.gammas().tobytes() == gam.tobytes()
    on = frame_results(c, n)
    c.set_enhance(False)
    c.upload(fe)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert frame_results(c, n) == on
    c.close()


def test_batch_identity_and_pose(oracle):
    n, w, h = 8, 1920, 1200
    svm = synth.svm_weights()
    frames = R.dim(synth.batch(400, n, w, h, CAMP_BLUE, 0, threads=16), 80)
    frames[3] = R.dim(synth.frame(403, w, h), 96)
    fe, gam = enhanced(frames)
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.svm_load(*svm)
    c.pnp_load()
    c.set_enhance(True)
    c.upload(frames)
    c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    c.sync()
    arm, offs = c.armours()
    ident = c.identities()
    r, t, p = c.poses()
    assert len(arm) > 0
    ocfg = oracle.default_pnp_config()

    def ref(f):
        a = oracle.detect_frame(fe[f], oracle.default_params())["armours"]
        return oracle.classify_armours(fe[f], a, svm), a
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(ref, range(n)))
    for f in range(n):
        (ri, ra, ricons), a0 = refs[f]
        sl = slice(offs[f], offs[f + 1])
        assert arm[sl].tobytes() == ra.tobytes(), f
        assert np.array_equal(ident[sl], ri), f
        assert np.array_equal(c.icons(f), ricons), f
        wr, wt, wp = oracle.locate_armours(a0, ocfg, np.eye(4))
        assert r[sl].tobytes() == wr.tobytes() and t[sl].tobytes() == wt.tobytes() and p[sl].tobytes() == wp.tobytes(), f
    # the icons come from E(f), not from f
    f = int(np.argmax(np.diff(offs)))
    a0 = refs[f][1]
    assert not np.array_equal(oracle.classify_armours(frames[f], a0, svm)[2], refs[f][0][2])
    # per frame: rmcv_classify_armours with the option on
    gi, ga, gicons = c.classify_armours(frames[f], a0)
    ri, ra, ricons = refs[f][0]
    assert np.array_equal(gi, ri) and ga.tobytes() == ra.tobytes() and np.array_equal(gicons, ricons)
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 4. the pipeline
def test_pipeline_switches_between_plain_and_enhanced_batches():
    import torch
    dev = torch.device("cuda", 0)
    p = default_params()
    geoms = [(48, 1280, 1024), (24, 640, 512), (16, 1920, 1200)]
    frames, want = [], {}
    for i, (n, w, h) in enumerate(geoms):
        fr = mixed(500 + 100 * i, n, w, h)
        frames.append(fr)
        for on in (False, True):
            ctx = Context(device=0, max_frames=n, max_width=w, max_height=h)
            ctx.set_enhance(on)
            ctx.upload(fr)
            ctx.run(p, STAGE_ALL)
            ctx.sync()
            want[(i, on)] = ctx.armours()
            ctx.close()
        assert want[(i, True)][0].tobytes() != want[(i, False)][0].tobytes()
    pl = Pipeline(device=0, max_frames=48, max_width=1920, max_height=1200)
    devf = [torch.from_numpy(f).to(dev) for f in frames]
    # (geometry, enhancement) per batch: runs of plain batches long enough for the hot rotation to start, enhancement switched on and off
    order = [(0, False)] * 6 + [(0, True)] * 4 + [(1, True), (2, True), (0, False), (0, False), (1, False), (2, True), (0, True)] + [(0, False)] * 5
    tickets, got = [], {}
    lag = pl.depth - 1
    hot_seen, now = [], None
    for i, (k, on) in enumerate(order):
        if on != now:
            pl.set_enhance(on)
            now = on
        n, h, w, _ = frames[k].shape
        before = pl.get_info().hot_batches
        tickets.append(pl.submit(devf[k].data_ptr(), n, h, w, p, STAGE_ALL))
        hot_seen.append((on, pl.get_info().hot_batches - before))
        if i >= lag:
            got[i - lag] = pl.collect(tickets[i - lag])
    pl.drain()
    for i in range(max(0, len(order) - lag), len(order)):
        got[i] = pl.collect(tickets[i])
    for i, (k, on) in enumerate(order):
        arm, offs = got[i]
        assert arm.tobytes() == want[(k, on)][0].tobytes() and list(offs) == list(want[(k, on)][1]), (i, k, on)
    info = pl.get_info()
    assert info.host_blocking_calls == 0
    assert all(grew == 0 for on, grew in hot_seen if on)       # enhancement batches stay out of the hot rotation
    # the legacy matcher is refused while the option is on, and the pipeline goes on
    pl.set_enhance(True)
    with pytest.raises(RmcvError) as e:
        pl.submit(devf[0].data_ptr(), 48, 1024, 1280, p, STAGE_ALL, legacy=LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1))
    assert e.value.code == abi.ERR_BAD_ARG
    t = pl.submit(devf[0].data_ptr(), 48, 1024, 1280, p, STAGE_ALL)
    arm, offs = pl.collect(t)
    assert arm.tobytes() == want[(0, True)][0].tobytes()
    # a ring whose contexts disagree about the option is refused at submit (whichever slot the batch would take), and goes on once they agree
    pl.set_enhance(False)
    pl.contexts[0].set_enhance(True)
    pl.contexts[pl.depth - 1].set_enhance(True)
    seen = 0
    for _ in range(pl.depth):
        try:
            pl.collect(pl.submit(devf[0].data_ptr(), 48, 1024, 1280, p, STAGE_ALL))
        except RmcvError as err:
            assert err.code == abi.ERR_BAD_ARG and "EVERY slot" in str(err)
            seen += 1
            break
    assert seen == 1
    pl.set_enhance(False)
    arm, offs = pl.collect(pl.submit(devf[0].data_ptr(), 48, 1024, 1280, p, STAGE_ALL))
    assert arm.tobytes() == want[(0, False)][0].tobytes()
    for c in pl.contexts:
        assert c.check_guards()[0] == 0
    pl.close()


def test_pipeline_enhance_argument():
    import torch
    n, w, h = 16, 1280, 1024
    fr = mixed(900, n, w, h)
    ctx = Context(device=0, max_frames=n, max_width=w, max_height=h)
    ctx.set_enhance(True, 30.0, 5.0)
    ctx.upload(fr)
    ctx.run(default_params(), STAGE_ALL)
    ctx.sync()
    want = ctx.armours()
    ctx.close()
    t = torch.from_numpy(fr).cuda()
    pl = Pipeline(device=0, depth=3, max_frames=n, max_width=w, max_height=h, enhance=(30.0, 5.0))
    ts = [pl.submit(t.data_ptr(), n, h, w, default_params(), STAGE_ALL) for _ in range(3)]
    for tk in ts:
        arm, offs = pl.collect(tk)
        assert arm.tobytes() == want[0].tobytes() and list(offs) == list(want[1])
    assert pl.get_info().host_blocking_calls == 0 and pl.get_info().hot_batches == 0
    pl.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_context_usable(oracle):
    n, w, h = 2, 1280, 1024
    fr = R.dim(synth.batch(0, n, w, h, CAMP_BLUE, 0), 80)
    fe, gam = enhanced(fr)
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    L = lib()

    def usable():
        c.set_enhance(True)
        c.upload(fr)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        check_against_oracle(c, fe, oracle)
        assert c.gammas().tobytes() == gam.tobytes()
    fresh = Context(device=0, max_frames=n, max_width=w, max_height=h)
    assert fresh.get_enhance() == (False, 100.0, 50.0)
    fresh.set_enhance(True, 30.0, 5.0)
    assert fresh.get_enhance() == (True, 30.0, 5.0)
    fresh.upload(fr)                                    # the option is bound, no run has built a table yet: every frame reads 1
    assert np.all(fresh.gammas() == 1.0)
    fresh.close()
    usable()
    # enhancement together with a Bayer input format: binding and the per-frame call are refused
    c.set_input_format(abi.BAYER_RG)
    mos = np.zeros((n, h, w), np.uint8)
    for call in (lambda: c.upload(mos), lambda: c.extract_color_csr(mos[0])):
        with pytest.raises(RmcvError) as e:
            call()
        assert e.value.code == abi.ERR_BAD_ARG and "Bayer" in str(e.value)
    c.set_input_format(abi.INPUT_BGR)
    usable()
    # the legacy matcher
    lp = LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1)
    with pytest.raises(RmcvError) as e:
        c.run_legacy(lp)
    assert e.value.code == abi.ERR_BAD_ARG and "legacy" in str(e.value)
    pts, offs, blobs, nb = np.zeros(1, abi.POINT), np.array([0, 1], np.int32), np.zeros(4, abi.LIGHTBLOB), C.c_int32(0)
    small = np.zeros((16, 16, 3), np.uint8)
    assert L.rmcv_find_lightblobs(c._h, ptr(small), 16, 16, 48, ptr(pts), ptr(offs), 1, C.byref(lp), ptr(blobs), 4, C.byref(nb), None, None) == abi.ERR_BAD_ARG
    assert "legacy" in L.rmcv_last_error(c._h).decode()
    usable()
    assert c.get_enhance() == (True, 100.0, 50.0)
    # gains that are not finite or equal: refused, the gains stay
    for hi, lo in ((50.0, 50.0), (float("nan"), 50.0), (100.0, float("-inf"))):
        assert L.rmcv_ctx_set_enhance_gains(c._h, C.c_float(hi), C.c_float(lo)) == abi.ERR_BAD_ARG
        out = np.zeros_like(fr[0])
        assert L.rmcv_auto_enhance(c._h, ptr(fr[0]), w, h, 3 * w, C.c_float(hi), C.c_float(lo), ptr(out), 3 * w, None) == abi.ERR_BAD_ARG
    assert c.get_enhance() == (True, 100.0, 50.0)
    usable()
    # a gamma that is negative or not finite
    out = np.full_like(fr[0], 7)
    for g in (-0.25, float("nan"), float("inf")):
        assert L.rmcv_calc_gamma(c._h, ptr(fr[0]), 3 * w, h, 3 * w, C.c_float(g), ptr(out), 3 * w) == abi.ERR_BAD_ARG
        assert "gamma" in L.rmcv_last_error(c._h).decode()
    assert np.all(out == 7)
    # unknown option values are refused and leave the option as it was
    assert L.rmcv_ctx_set_option(c._h, abi.OPT_ENHANCE, 2) == abi.ERR_BAD_ARG and L.rmcv_ctx_set_option(c._h, abi.OPT_ENHANCE, -1) == abi.ERR_BAD_ARG
    usable()
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 6. the shim
def test_shim_auto_enhance_matches_python_path(tmp_path, oracle):
    tmp = str(tmp_path)
    objs = []
    for unit in ("shim_enhance/backend_enhance", "shim/core_stub", "shim_enhance/caller_enhance"):
        o = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "cv_mock"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(HERE, "shim"),
                        "-I", os.path.join(HERE, "shim_enhance"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", o], check=True)
        objs.append(o)
    exe = os.path.join(tmp, "shim_enhance_main")
    subprocess.run(["g++"] + objs + ["-o", exe, "-L", LIBDIR, "-lrmcv_hip", "-Wl,-rpath," + LIBDIR, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)

    def fnv(a):  # caller_enhance.cpp's position-weighted byte sum, modulo 2^64
        a = np.ascontiguousarray(a).reshape(-1).astype(np.uint64)
        with np.errstate(over="ignore"):
            return int(((a + np.uint64(1)) * (np.arange(len(a), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1))).sum(dtype=np.uint64))
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    for index, num in ((0, 80), (3, 96)):
        out = subprocess.run([exe, str(index), str(num)], check=True, capture_output=True, text=True, timeout=180).stdout.strip().splitlines()
        d = R.dim(synth.frame(index), num)
        e, _ = c.auto_enhance(d)
        assert np.array_equal(e, R.E(d)[0])
        line = {l.split()[0]: l.split()[1:] for l in out if not l.startswith("armour")}
        assert int(line["enhanced"][0], 16) == fnv(e)
        binary, pts, offs, blobs, src, neg, arm = chain(c, e)
        head = dict(zip(out[1].split()[0::2], map(int, out[1].split()[1::2])))
        assert head["contours"] == len(offs) - 1 and head["points"] == len(pts) and head["binary_on"] == int(np.count_nonzero(binary))
        assert head["positive"] == len(blobs) and head["negative"] == len(neg) and head["armours"] == len(arm) and len(arm) > 0
        got = [[float.fromhex(t) for t in l.split()[1:]] for l in out if l.startswith("armour")]
        assert got == [[float(v) for v in a["vertices"].reshape(-1)] for a in arm]
        ref = oracle.detect_frame(e, oracle.default_params())
        assert arm.tobytes() == ref["armours"].tobytes()
        assert line["fused_same"][:2] == ["1", "plain_contours"] and int(line["fused_same"][2]) == len(oracle.detect_frame(d, oracle.default_params())["offs"]) - 1
        assert int(line["gamma22"][0], 16) == fnv(R.calc_gamma(d, 2.2)) and int(line["gamma05"][0], 16) == fnv(R.calc_gamma(d, 0.5))
    c.close()
