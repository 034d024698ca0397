"""Raw Bayer frames (RMCV_OPT_INPUT_FORMAT) on the GPU.  The contract: every output for a mosaic m equals, bit for bit, what the BGR
path gives for D(m) (tests/bayer_ref.py) -- so the CPU oracle, run on D(m), checks every stage, and so does the same context's
BGR call on D(m)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bayer_ref as BR
from rmcv_amd import (CAMP_BLUE, CAMP_GUIDELIGHT, CAMP_RED, MORPH_CLOSE, MORPH_DILATE, MORPH_NONE, OPT_CONTOUR_TIER, OPT_FRAME_UPLOAD,
                      OPT_IMAGE_EXPORT, OPT_TEST_SLOW_US, STAGE_ALL, STAGE_IDENTITY, STAGE_NO_IMAGE, STAGE_POSE, Context, LegacyParams, Pipeline, RmcvError,
                      default_params, synth)
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu


def scene(seed, w, h, camp=CAMP_BLUE, pattern=BR.RG):
    """a synthetic camera frame's mosaic and D of it"""
    m = BR.mosaic(synth.frame(seed, w, h, camp), pattern)
    return m, BR.demosaic(m, pattern)


def ref_frame(oracle, d, p=None):
    return oracle.detect_frame(d, p or oracle.default_params())


def check_frame(ctx, f, ref, image=True):
    if image:
        assert np.array_equal(ctx.binary(f), ref["binary"]), f
    pts, offs = ctx.contours(f)
    assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), f
    blobs, _ = ctx.blobs(f)
    assert blobs.tobytes() == ref["blobs"].tobytes(), f


# ---------------------------------------------------------------- 1. rmcv_demosaic
@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_demosaic_equals_d(pattern):
    c = Context(device=0, max_frames=1, max_width=1920, max_height=1200)
    rng = np.random.default_rng(pattern)
    for (w, h, stride) in [(3, 3, 3), (5, 4, 5), (1283, 1021, 1300), (1280, 1024, 1280), (1920, 1200, 1920)]:
        raw = rng.integers(0, 256, (h, stride), dtype=np.uint8)
        out = np.full((h, 3 * w + 5), 7, np.uint8)
        rc = lib().rmcv_demosaic(c._h, ptr(raw), w, h, stride, pattern, ptr(out), 3 * w + 5)
        assert rc == 0, lib().rmcv_last_error(c._h)
        want = BR.demosaic(raw[:, :w], pattern)
        assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), want), (w, h)
        assert np.all(out[:, 3 * w:] == 7)  # the row padding of the output is left alone
    assert np.array_equal(c.demosaic(raw[:, :1920], pattern), BR.demosaic(raw[:, :1920], pattern))
    assert c.check_guards()[0] == 0
    c.close()


def test_demosaic_refuses_bad_arguments():
    """every argument check of rmcv_demosaic, with a real context: each refusal names its reason, nothing is written"""
    c = Context(device=0, max_frames=1, max_width=64, max_height=64)
    raw = np.zeros((8, 8), np.uint8)
    out = np.full((8, 24), 7, np.uint8)
    L = lib()
    cases = [((ptr(raw), 8, 8, 8, BR.RG, None, 24), "null buffer"), ((None, 8, 8, 8, BR.RG, ptr(out), 24), "null buffer"),
             ((ptr(raw), 2, 8, 8, BR.RG, ptr(out), 24), "w >= 3"), ((ptr(raw), 8, 2, 8, BR.RG, ptr(out), 24), "w >= 3"),
             ((ptr(raw), 8, 8, 7, BR.RG, ptr(out), 24), "stride < w"), ((ptr(raw), 8, 8, 8, BR.RG, ptr(out), 23), "out_stride"),
             ((ptr(raw), 8, 8, 8, 0, ptr(out), 24), "unknown Bayer pattern"), ((ptr(raw), 8, 8, 8, 5, ptr(out), 24), "unknown Bayer pattern")]
    for args, why in cases:
        assert L.rmcv_demosaic(c._h, *args) == abi.ERR_BAD_ARG, (args, why)
        assert why in L.rmcv_last_error(c._h).decode(), why
    assert np.all(out == 7)
    assert L.rmcv_demosaic(c._h, ptr(raw), 8, 8, 8, BR.RG, ptr(out), 24) == 0 and np.all(out == 0)
    c.close()


# ---------------------------------------------------------------- 2. the per-frame chain
def chain(ctx, img, camp, lb, morph):
    pts, offs, binary = ctx.extract_color_csr(img, camp, lb, morph)
    blobs, src, neg = ctx.filter_lightblobs(pts, offs, enemy=camp)
    arm = ctx.filter_armours(blobs, enemy=camp)
    return binary, pts, offs, blobs, src, neg, arm


def test_chain_every_pattern_camp_morph_bound(oracle):
    # (lower_bound 1 on the demosaiced noise: tens of thousands of specks -- room for all of them)
    c = Context(device=0, max_frames=1, max_width=640, max_height=512, max_contours=1 << 16, max_points=1 << 20, max_blobs=1 << 14)
    for pattern in BR.PATTERNS:
        for camp in (CAMP_BLUE, CAMP_RED):
            m, d = scene(7000 + pattern * 10 + camp, 640, 512, camp, pattern)
            for morph in (MORPH_NONE, MORPH_DILATE, MORPH_CLOSE):
                for lb in (0, 1, 80, 256):
                    c.set_input_format(pattern)
                    got = chain(c, m, camp, lb, morph)
                    c.set_input_format(0)
                    bgr = chain(c, d, camp, lb, morph)  # the same context's BGR call on D(m)
                    for g, b in zip(got, bgr):
                        assert g.tobytes() == b.tobytes(), (pattern, camp, morph, lb)
                    p = oracle.default_params(camp=camp, lower_bound=lb, morph=morph)
                    ref = oracle.detect_frame(d, p, cap_pts=1 << 20, cap_contours=1 << 16, cap_blobs=1 << 14)
                    assert np.array_equal(got[0], ref["binary"]), (pattern, camp, morph, lb)
                    assert np.array_equal(got[2], ref["offs"]) and np.array_equal(got[1], ref["pts"]), (pattern, camp, morph, lb)
                    assert got[3].tobytes() == ref["blobs"].tobytes() and got[6].tobytes() == ref["armours"].tobytes(), (pattern, camp, morph, lb)
    # the guide-light camp (G - R) too
    m, d = scene(7100, 640, 512, CAMP_BLUE, BR.GR)
    c.set_input_format(BR.GR)
    _, _, binary = c.extract_color_csr(m, CAMP_GUIDELIGHT, 30, MORPH_CLOSE)
    assert np.array_equal(binary, oracle.extract_binary(d, CAMP_GUIDELIGHT, 30, MORPH_CLOSE))
    c.close()


@pytest.mark.parametrize("upload", [0, 1, 2, 3])
@pytest.mark.parametrize("export", [0, 1])
def test_chain_upload_and_export_modes(oracle, upload, export):
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    c.set_option(OPT_FRAME_UPLOAD, upload)
    c.set_option(OPT_IMAGE_EXPORT, export)
    c.set_input_format(BR.BG)
    keep = []  # mode 2 pins the caller's buffers in place: they must outlive the context
    for i in range(3):  # (the second and third frames run ahead: the filters ride with extract_color)
        m, d = scene(7200 + i, 1280, 1024, CAMP_BLUE, BR.BG)
        keep.append(m)
        binary, pts, offs, blobs, src, neg, arm = chain(c, m, CAMP_BLUE, 80, MORPH_CLOSE)
        ref = ref_frame(oracle, d)
        assert np.array_equal(binary, ref["binary"]) and np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"])
        assert blobs.tobytes() == ref["blobs"].tobytes() and arm.tobytes() == ref["armours"].tobytes()
    # a mosaic with padded rows, straight through the C-ABI
    m, d = scene(7210, 1280, 1024, CAMP_BLUE, BR.BG)
    padded = np.zeros((1024, 1300), np.uint8)
    padded[:, :1280] = m
    keep.append(padded)
    binary = np.empty((1024, 1280), np.uint8)
    pts = np.empty(c.limits.max_points, abi.POINT)
    offs = np.empty(c.limits.max_contours + 1, np.int32)
    nc, npt = C.c_int32(0), C.c_int32(0)
    rc = lib().rmcv_extract_color(c._h, ptr(padded), 1280, 1024, 1300, CAMP_BLUE, 80, MORPH_CLOSE, ptr(binary), ptr(pts), len(pts), ptr(offs),
                                  len(offs) - 1, C.byref(nc), C.byref(npt))
    assert rc == 0
    assert np.array_equal(binary, oracle.extract_binary(d, CAMP_BLUE, 80, MORPH_CLOSE))
    c.close()
    del keep


def test_chain_leaves_a_slow_runtime_copy_for_a_mosaic(oracle):
    """RMCV_OPT_FRAME_UPLOAD 3: the upload of a mosaic is judged by its own 1 B/px (1280x1024: slow above 1.3 MB / 45 GB/s + 100 us =
    129 us, where a BGR frame's 3.9 MB would allow 187 us).  With 150 us added to what the library measures, three frames in a row are
    slow and the chain moves to the pinned staging buffer; the results never change."""
    L = abi.lib()
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    c.set_option(OPT_IMAGE_EXPORT, 0)                # (the image path stays put: only the upload is judged here)
    c.set_input_format(BR.GR)
    m, d = scene(7250, 1280, 1024, CAMP_BLUE, BR.GR)
    ref = ref_frame(oracle, d)

    def one():
        binary, pts, offs, blobs, src, neg, arm = chain(c, m, CAMP_BLUE, 80, MORPH_CLOSE)
        assert np.array_equal(binary, ref["binary"]) and np.array_equal(pts, ref["pts"]) and arm.tobytes() == ref["armours"].tobytes()
        us = (C.c_double * 9)()
        assert L.rmcv_ctx_frame_timing(c._h, us, 9) == 0
        return int(us[7])
    one()
    c.set_option(OPT_FRAME_UPLOAD, 3)                # (set again: the counters start over whatever the first frame met)
    c.set_option(OPT_TEST_SLOW_US, 150)
    seen = [one() for _ in range(5)]
    assert seen[0] == 0 and seen[3:] == [1, 1], seen  # the runtime's copy first; three slow frames, then pinned staging
    c.close()


# ---------------------------------------------------------------- 3. batches
@pytest.fixture(scope="module")
def batch256(oracle):
    """256 x 1280x1024 mosaics (pattern RG, camp BLUE) and the oracle's results on D of each"""
    n, w, h = 256, 1280, 1024
    bgr = synth.batch(7300, n, w, h, CAMP_BLUE, 0, threads=16)
    mos = BR.mosaic(bgr, BR.RG)
    with ThreadPoolExecutor(16) as ex:
        d = list(ex.map(lambda f: BR.demosaic(mos[f], BR.RG), range(n)))
        refs = list(ex.map(lambda f: ref_frame(oracle, d[f]), range(n)))
    return mos, d, refs


def check_batch(c, refs, image=True):
    arm, offs = c.armours()
    for f in range(len(refs)):
        check_frame(c, f, refs[f], image)
        assert arm[offs[f]:offs[f + 1]].tobytes() == refs[f]["armours"].tobytes(), f


def test_batch_upload_256(batch256):
    mos, d, refs = batch256
    c = Context(device=0, max_frames=256, max_width=1280, max_height=1024)
    c.set_input_format(BR.RG)
    c.upload(mos)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    st_bayer = c.counts()["status"]
    # the same context, BGR path, on D(m): same status words
    c.set_input_format(0)
    c.upload(np.stack(d[:16]))
    c.run(default_params(), STAGE_ALL)
    c.sync()
    assert np.array_equal(c.counts()["status"], st_bayer[:16])
    c.close()


def test_batch_torch_strided_pitched_no_image(batch256):
    import torch
    mos, d, refs = batch256
    n, h, w = mos.shape
    stride, pitch = 1344, 1344 * 1024 + 4096
    buf = np.zeros(n * pitch, np.uint8)
    for f in range(n):
        buf[f * pitch:f * pitch + h * stride].reshape(h, stride)[:, :w] = mos[f]
    t = torch.from_numpy(buf).cuda()
    c = Context(device=0, max_frames=256, max_width=1280, max_height=1024)
    c.set_input_format(BR.RG)
    c.bind_device_frames(t.data_ptr(), n, h, w, stride, pitch, keepalive=t)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    c.run(default_params(), STAGE_ALL | STAGE_NO_IMAGE)
    c.sync()
    check_batch(c, refs, image=False)
    # contiguous tensor, default stride (w under a Bayer format)
    t2 = torch.from_numpy(mos).cuda()
    c.bind_device_frames(t2.data_ptr(), n, h, w, keepalive=t2)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    c.close()


def test_batch_dense_mid_tier(oracle):
    """hundreds of specks per frame: the contour stage's mid tier behind the Bayer pixel kernel"""
    n, w, h = 24, 1280, 1024
    bgr = synth.batch(7400, n, w, h, CAMP_BLUE, 0, threads=16)
    rng = np.random.default_rng(3)
    for f in range(n):
        ys, xs = rng.integers(2, h - 4, 600), rng.integers(2, w - 4, 600)
        for y, x in zip(ys, xs):
            bgr[f, y:y + 3, x:x + 3] = (255, 90, 10)
    mos = BR.mosaic(bgr, BR.GB)
    d = [BR.demosaic(mos[f], BR.GB) for f in range(n)]
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda f: ref_frame(oracle, d[f]), range(n)))
    assert max(len(r["offs"]) for r in refs) > 300
    c = Context(device=0, max_frames=n, max_width=w, max_height=h, max_contours=4096)
    c.set_input_format(BR.GB)
    for tier in (0, 2):
        c.set_option(OPT_CONTOUR_TIER, tier)
        c.upload(mos)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        check_batch(c, refs)
    c.close()


# ---------------------------------------------------------------- 4. C5: identities, icons, poses
def test_c5_identity_pose_and_per_frame_classify(oracle):
    n, w, h = 24, 1920, 1200
    svm = synth.svm_weights()
    bgr = synth.batch(7500, n, w, h, CAMP_BLUE, 0, threads=16)
    mos = BR.mosaic(bgr, BR.BG)
    d = [BR.demosaic(mos[f], BR.BG) for f in range(n)]
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.svm_load(*svm)
    c.pnp_load()
    c.set_input_format(BR.BG)
    c.upload(mos)
    c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    c.sync()
    arm, offs = c.armours()
    ident = c.identities()
    r, t, p = c.poses()
    assert len(arm) > 0
    ocfg = oracle.default_pnp_config()

    def ref(f):
        a = ref_frame(oracle, d[f])["armours"]
        return oracle.classify_armours(d[f], a, svm), a
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
    # per frame: rmcv_classify_armours on the mosaic
    f = int(np.argmax(np.diff(offs)))
    a0 = refs[f][1]
    gi, ga, gicons = c.classify_armours(mos[f], a0)
    ri, ra, ricons = oracle.classify_armours(d[f], a0, svm)
    assert np.array_equal(gi, ri) and ga.tobytes() == ra.tobytes() and np.array_equal(gicons, ricons)
    c.close()


# ---------------------------------------------------------------- 5. the pipeline
def test_pipeline_bayer_slots_and_bgr_beside(oracle):
    import torch
    dev = torch.device("cuda", 0)
    p = default_params()
    geoms = [(64, 1280, 1024), (32, 640, 512), (64, 1280, 1024)]
    mos, want = [], []
    for i, (n, w, h) in enumerate(geoms):
        m = BR.mosaic(synth.batch(7600 + 100 * i, n, w, h, CAMP_BLUE, i % 2, threads=16), BR.GR)
        mos.append(m)
        ctx = Context(device=0, max_frames=n, max_width=w, max_height=h)
        ctx.set_input_format(BR.GR)
        ctx.upload(m)
        ctx.run(p, STAGE_ALL)
        ctx.sync()
        want.append(ctx.armours())
        ctx.close()
    # the context results above are the oracle's (test_batch_*); spot-check one frame here as well
    ref = ref_frame(oracle, BR.demosaic(mos[1][0], BR.GR))
    assert want[1][0][want[1][1][0]:want[1][1][1]].tobytes() == ref["armours"].tobytes()

    bgr = synth.batch(7700, 32, 1280, 1024, CAMP_BLUE, 0, threads=16)
    tb = torch.from_numpy(bgr).to(dev)

    def bgr_lists():
        q = Pipeline(device=0, max_frames=64, max_width=1280, max_height=1024)
        ts = [q.submit(tb.data_ptr(), 32, 1024, 1280, p, STAGE_ALL) for _ in range(3)]
        out = [q.collect(t) for t in ts]
        q.close()
        return out
    before = bgr_lists()

    ws0 = lib().rmcv_pixel_ws_launches()
    pl = Pipeline(device=0, max_frames=64, max_width=1280, max_height=1024, input_format=BR.GR)
    devm = [torch.from_numpy(m).to(dev) for m in mos]
    order = [0, 0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 0, 2, 2, 1, 0]
    tickets, got = [], {}
    lag = pl.depth - 1  # a ticket is collected before its slot comes round again
    for i, k in enumerate(order):
        n, h, w = mos[k].shape
        tickets.append(pl.submit(devm[k].data_ptr(), n, h, w, p, STAGE_ALL))
        if i >= lag:
            got[i - lag] = pl.collect(tickets[i - lag])
    pl.drain()
    for i in range(max(0, len(order) - lag), len(order)):
        got[i] = pl.collect(tickets[i])
    for i, k in enumerate(order):
        arm, offs = got[i]
        assert arm.tobytes() == want[k][0].tobytes() and list(offs) == list(want[k][1]), (i, k)
    info = pl.get_info()
    assert info.host_blocking_calls == 0
    assert lib().rmcv_pixel_ws_launches() == ws0  # a Bayer batch never runs k_binary_ws
    # the legacy matcher is not for mosaics
    with pytest.raises(RmcvError) as e:
        pl.submit(devm[0].data_ptr(), 64, 1024, 1280, p, STAGE_ALL, legacy=LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1))
    assert e.value.code == abi.ERR_BAD_ARG
    pl.close()

    after = bgr_lists()
    for (a0, o0), (a1, o1) in zip(before, after):
        assert a0.tobytes() == a1.tobytes() and list(o0) == list(o1)


# ---------------------------------------------------------------- 6. back to BGR, guards, legacy entry points
def test_back_to_bgr_guards_and_legacy(oracle):
    n, w, h = 4, 1280, 1024
    bgr = synth.batch(7800, n, w, h, CAMP_BLUE, 0)
    c = Context(device=0, max_frames=n, max_width=1448, max_height=h)
    # odd sizes through every path of the Bayer kernel: unaligned rows and ragged last words (3 .. 1283), h % 32 != 0, w = 1 (mod 16)
    # (the last column is a lane's pixel 0 and takes its bit from the lane before -- for 1025 from another wave: recomputed), and the
    # dwordx4 loader with w a multiple of 16 but not of 64 (1440: lanes beyond the row read the next row's bytes)
    c.set_input_format(BR.RG)
    for (ww, hh) in [(3, 3), (5, 4), (17, 9), (67, 45), (1025, 700), (1283, 1021), (1001, 999), (1440, 1024)]:
        big = synth.frame(7850 + ww, max(ww, 256), max(hh, 256), CAMP_BLUE)[:hh, :ww].copy()  # (the generator wants room for its scene)
        big[hh // 4:hh // 2, -3:] = (255, 60, 0)   # lit last columns in some rows: the border bits are 1 there, 0 elsewhere
        big[:hh // 8, :2] = (255, 60, 0)           # ... and the first columns
        m = BR.mosaic(big, BR.RG)
        dd = BR.demosaic(m, BR.RG)
        for morph in (MORPH_NONE, MORPH_CLOSE):
            _, _, binary = c.extract_color_csr(m, CAMP_BLUE, 60, morph)
            assert np.array_equal(binary, oracle.extract_binary(dd, CAMP_BLUE, 60, morph)), (ww, hh, morph)
        c.upload(np.stack([m, m]))
        c.run(default_params(), STAGE_ALL)
        c.sync()
        check_frame(c, 1, ref_frame(oracle, dd))
    assert c.check_guards()[0] == 0
    # legacy: refused under a Bayer format
    lp = LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1)
    with pytest.raises(RmcvError) as e:
        c.run_legacy(lp)
    assert e.value.code == abi.ERR_BAD_ARG
    pts = np.zeros(1, abi.POINT)
    offs = np.array([0, 1], np.int32)
    blobs = np.zeros(4, abi.LIGHTBLOB)
    nb = C.c_int32(0)
    m = np.zeros((16, 16), np.uint8)
    assert lib().rmcv_find_lightblobs(c._h, ptr(m), 16, 16, 16, ptr(pts), ptr(offs), 1, C.byref(lp), ptr(blobs), 4, C.byref(nb),
                                      None, None) == abi.ERR_BAD_ARG
    assert "legacy" in lib().rmcv_last_error(c._h).decode()
    # unknown values are refused, the format stays
    assert lib().rmcv_ctx_set_option(c._h, abi.OPT_INPUT_FORMAT, 5) == abi.ERR_BAD_ARG
    assert lib().rmcv_ctx_set_option(c._h, abi.OPT_INPUT_FORMAT, -1) == abi.ERR_BAD_ARG
    # back to BGR: identical to a fresh context
    c.set_input_format(0)
    c.upload(bgr)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    fresh = Context(device=0, max_frames=n, max_width=1448, max_height=h)
    fresh.upload(bgr)
    fresh.run(default_params(), STAGE_ALL)
    fresh.sync()
    a1, o1 = c.armours()
    a2, o2 = fresh.armours()
    assert a1.tobytes() == a2.tobytes() and list(o1) == list(o2)
    for f in range(n):
        assert np.array_equal(c.binary(f), fresh.binary(f))
        assert all(np.array_equal(x, y) for x, y in zip(c.contours(f), fresh.contours(f)))
    pc, oc, bc = c.extract_color_csr(bgr[0])
    pf, of, bf = fresh.extract_color_csr(bgr[0])
    assert np.array_equal(pc, pf) and np.array_equal(oc, of) and np.array_equal(bc, bf)
    assert c.check_guards()[0] == 0 and fresh.check_guards()[0] == 0
    c.close()
    fresh.close()
