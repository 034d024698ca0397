"""The sensor's frame as delivered (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT) on the GPU.  The contract: every output for a
delivered buffer r equals, bit for bit, what the 8-bit Bayer path gives for the oriented mosaic T(r) with the derived pattern
(tests/raw_ref.py) -- hence what the oracle gives for D(T(r)) (tests/bayer_ref.py).  Nothing here has a tolerance."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bayer_ref as BR
import raw_ref as RR
from rmcv_amd import (CAMP_BLUE, CAMP_GUIDELIGHT, CAMP_RED, MORPH_CLOSE, MORPH_DILATE, MORPH_NONE, OPT_CONTOUR_TIER, OPT_FRAME_UPLOAD,
                      OPT_IMAGE_EXPORT, OPT_TEST_SLOW_US, STAGE_ALL, STAGE_IDENTITY, STAGE_NO_IMAGE, STAGE_POSE, Context, LegacyParams, Pipeline,
                      RmcvError, default_params, synth)
from rmcv_amd import abi
from rmcv_amd.abi import lib, ptr

pytestmark = pytest.mark.gpu

SAMPLES = [(8, 0), (16, 0), (16, 2), (16, 4)]  # (sample bits, valid bit)


def scene(seed, w, h, pattern, bits, vbit, mirror, flip, camp=CAMP_BLUE, n=None, variant=0):
    """a delivered buffer r of pattern `pattern` whose oriented reading is a synthetic camera frame's mosaic: (r, T(r), the derived
    pattern, D(T(r))); n: a batch"""
    dp = RR.derived_pattern(pattern, w, h, mirror, flip)
    bgr = synth.frame(seed, w, h, camp, variant) if n is None else synth.batch(seed, n, w, h, camp, variant, threads=16)
    m = BR.mosaic(bgr, dp)
    r = synth.raw_frame(m, bits, vbit, mirror, flip, np.random.default_rng(seed))
    assert np.array_equal(RR.T(r, vbit, mirror, flip), m)
    if n is None:
        return r, m, dp, BR.demosaic(m, dp)
    with ThreadPoolExecutor(16) as ex:
        d = list(ex.map(lambda f: BR.demosaic(m[f], dp), range(n)))
    return r, m, dp, d


def use(ctx, pattern, bits=8, vbit=0, mirror=False, flip=False):
    ctx.set_input_format(pattern)
    ctx.set_input_layout(bits, vbit, mirror, flip)


def ref_frame(oracle, d, p=None):
    return oracle.detect_frame(d, p or oracle.default_params())


def check_frame(ctx, f, ref, image=True):
    if image:
        assert np.array_equal(ctx.binary(f), ref["binary"]), f
    pts, offs = ctx.contours(f)
    assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), f
    blobs, _ = ctx.blobs(f)
    assert blobs.tobytes() == ref["blobs"].tobytes(), f


def check_batch(c, refs, image=True):
    arm, offs = c.armours()
    for f in range(len(refs)):
        check_frame(c, f, refs[f], image)
        assert arm[offs[f]:offs[f + 1]].tobytes() == refs[f]["armours"].tobytes(), f


def chain(ctx, img, camp, lb, morph):
    pts, offs, binary = ctx.extract_color_csr(img, camp, lb, morph)
    blobs, src, neg = ctx.filter_lightblobs(pts, offs, enemy=camp)
    arm = ctx.filter_armours(blobs, enemy=camp)
    return binary, pts, offs, blobs, src, neg, arm


# ---------------------------------------------------------------- 1. rmcv_demosaic_raw
@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_demosaic_raw_equals_d_of_t(pattern):
    c = Context(device=0, max_frames=1, max_width=1920, max_height=1200)
    rng = np.random.default_rng(40 + pattern)
    for (w, h, pad) in [(3, 3, 0), (5, 4, 0), (1283, 1021, 17), (1280, 1024, 0), (1920, 1200, 0)]:
        for bits, vbit in SAMPLES:
            sb = bits // 8
            r = rng.integers(0, 1 << bits, (h, w + pad), dtype=np.uint16 if sb == 2 else np.uint8)
            for mirror, flip in RR.ORIENTATIONS:
                out = np.full((h, 3 * w + 5), 7, np.uint8)
                orient = (abi.ORIENT_MIRROR if mirror else 0) | (abi.ORIENT_FLIP if flip else 0)
                rc = lib().rmcv_demosaic_raw(c._h, ptr(r), w, h, (w + pad) * sb, pattern, bits, vbit, orient, ptr(out), 3 * w + 5)
                assert rc == 0, lib().rmcv_last_error(c._h)
                want = BR.demosaic(RR.T(r[:, :w], vbit, mirror, flip), RR.derived_pattern(pattern, w, h, mirror, flip))
                assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), want), (w, h, bits, vbit, mirror, flip)
                assert np.all(out[:, 3 * w:] == 7)  # the row padding of the output is left alone
    r = rng.integers(0, 1 << 16, (64, 80), dtype=np.uint16)
    assert np.array_equal(c.demosaic_raw(r, pattern, 3, True, True), BR.demosaic(RR.T(r, 3, True, True), RR.derived_pattern(pattern, 80, 64, True, True)))
    assert np.array_equal(c.demosaic_raw(r.astype(np.uint8), pattern), c.demosaic(r.astype(np.uint8), pattern))
    assert c.check_guards()[0] == 0
    c.close()


def test_demosaic_raw_refuses_bad_arguments():
    c = Context(device=0, max_frames=1, max_width=64, max_height=64)
    raw = np.zeros((8, 9), np.uint16)
    out = np.full((8, 24), 7, np.uint8)
    odd = C.c_void_p(raw.ctypes.data + 1)
    f = lib().rmcv_demosaic_raw
    cases = [((None, 8, 8, 16, 1, 16, 4, 3, ptr(out), 24), "null buffer"), ((ptr(raw), 8, 8, 16, 1, 16, 4, 3, None, 24), "null buffer"),
             ((ptr(raw), 2, 8, 16, 1, 16, 4, 3, ptr(out), 24), "w >= 3"), ((ptr(raw), 8, 8, 14, 1, 16, 4, 3, ptr(out), 24), "stride < 2 w"),
             ((ptr(raw), 8, 8, 7, 1, 8, 0, 3, ptr(out), 24), "stride < w"), ((ptr(raw), 8, 8, 17, 1, 16, 4, 3, ptr(out), 24), "odd stride"),
             ((odd, 8, 8, 16, 1, 16, 4, 3, ptr(out), 24), "2-byte aligned"), ((ptr(raw), 8, 8, 16, 1, 16, 5, 3, ptr(out), 24), "valid_bit"),
             ((ptr(raw), 8, 8, 16, 1, 16, -1, 3, ptr(out), 24), "valid_bit"), ((ptr(raw), 8, 8, 16, 1, 16, 4, 4, ptr(out), 24), "orientation"),
             ((ptr(raw), 8, 8, 16, 1, 12, 4, 3, ptr(out), 24), "sample_bits"), ((ptr(raw), 8, 8, 16, 1, 16, 4, 3, ptr(out), 23), "out_stride"),
             ((ptr(raw), 8, 8, 16, 0, 16, 4, 3, ptr(out), 24), "unknown Bayer pattern")]
    for args, why in cases:
        assert f(c._h, *args) == abi.ERR_BAD_ARG, (args, why)
        assert why in lib().rmcv_last_error(c._h).decode(), why
    assert np.all(out == 7)
    assert f(c._h, ptr(raw), 8, 8, 18, 1, 16, 4, 3, ptr(out), 24) == 0 and np.all(out == 0)
    c.close()


# ---------------------------------------------------------------- 2. the per-frame chain
def test_chain_every_orientation_pattern_sample_morph(oracle):
    """640x512.  Thinned from the full product so that the run stays short: every (pattern, orientation, sample layout) triple runs
    -- 48 of them -- each with two (morph, lower bound) pairs and one camp, rotated so that every orientation meets every pattern,
    both sample sizes, all three morphs, all four bounds and both camps."""
    c = Context(device=0, max_frames=1, max_width=640, max_height=512, max_contours=1 << 16, max_points=1 << 20, max_blobs=1 << 14)
    morphs, lbs = (MORPH_NONE, MORPH_DILATE, MORPH_CLOSE), (0, 1, 80, 256)
    seen = set()
    i = 0
    for oi, (mirror, flip) in enumerate(RR.ORIENTATIONS):
        for pi, pattern in enumerate(BR.PATTERNS):
            for si, (bits, vbit) in enumerate([(8, 0), (16, 2), (16, 4)]):
                camp = (CAMP_BLUE, CAMP_RED)[(pi + si + oi) % 2]
                r, m, dp, d = scene(7000 + i, 640, 512, pattern, bits, vbit, mirror, flip, camp)
                for k in range(2):
                    morph, lb = morphs[(pi + si + k) % 3], lbs[(i + 2 * k + oi) % 4]
                    what = (pattern, mirror, flip, bits, vbit, camp, morph, lb)
                    seen.add((oi, morph)); seen.add((oi, bits)); seen.add((oi, pattern)); seen.add(("lb", lb)); seen.add(("camp", camp))
                    use(c, pattern, bits, vbit, mirror, flip)
                    got = chain(c, r, camp, lb, morph)
                    use(c, dp)  # the same context, default layout, on T(r) with the derived pattern
                    plain = chain(c, m, camp, lb, morph)
                    for g, b in zip(got, plain):
                        assert g.tobytes() == b.tobytes(), what
                    p = oracle.default_params(camp=camp, lower_bound=lb, morph=morph)
                    ref = oracle.detect_frame(d, p, cap_pts=1 << 20, cap_contours=1 << 16, cap_blobs=1 << 14)
                    assert np.array_equal(got[0], ref["binary"]), what
                    assert np.array_equal(got[2], ref["offs"]) and np.array_equal(got[1], ref["pts"]), what
                    assert got[3].tobytes() == ref["blobs"].tobytes() and got[6].tobytes() == ref["armours"].tobytes(), what
                i += 1
    for oi in range(4):
        assert all((oi, x) in seen for x in morphs + (8, 16) + BR.PATTERNS)
    assert all(("lb", x) in seen for x in lbs) and ("camp", CAMP_BLUE) in seen and ("camp", CAMP_RED) in seen
    # the guide-light camp (G - R) once
    r, m, dp, d = scene(7100, 640, 512, BR.GR, 16, 2, True, True)
    use(c, BR.GR, 16, 2, True, True)
    _, _, binary = c.extract_color_csr(r, CAMP_GUIDELIGHT, 30, MORPH_CLOSE)
    assert np.array_equal(binary, oracle.extract_binary(d, CAMP_GUIDELIGHT, 30, MORPH_CLOSE))
    c.close()


# ---------------------------------------------------------------- 3. odd geometry
def extract_binary_strided(c, r, w, h, pad_samples, camp, lb, morph):
    """rmcv_extract_color straight through the C-ABI on a buffer whose rows are `pad_samples` samples longer than w"""
    buf = np.zeros((h, w + pad_samples), r.dtype)
    buf[:, :w] = r
    binary = np.empty((h, w), np.uint8)
    pts = np.empty(c.limits.max_points, abi.POINT)
    offs = np.empty(c.limits.max_contours + 1, np.int32)
    nc, npt = C.c_int32(0), C.c_int32(0)
    rc = lib().rmcv_extract_color(c._h, ptr(buf), w, h, (w + pad_samples) * buf.itemsize, camp, lb, morph, ptr(binary), ptr(pts), len(pts),
                                  ptr(offs), len(offs) - 1, C.byref(nc), C.byref(npt))
    assert rc == 0, lib().rmcv_last_error(c._h)
    return binary


@pytest.mark.parametrize("mirror", [False, True])
def test_odd_geometry(oracle, mirror):
    """unaligned rows and ragged words through the byte-wise loader (with mirror the ragged end of a row sits in the first lane), the
    last column taking its bit from another wave (1025), the dwordx4 loaders with w a multiple of 16 but not of 64 (1440)"""
    c = Context(device=0, max_frames=2, max_width=1448, max_height=1024)
    for gi, (ww, hh) in enumerate([(3, 3), (5, 4), (17, 9), (67, 45), (1025, 700), (1283, 1021), (1001, 999), (1440, 1024)]):
        flip = bool(gi & 1)
        big = synth.frame(7850 + ww, max(ww, 256), max(hh, 256), CAMP_BLUE)[:hh, :ww].copy()
        big[hh // 4:hh // 2, -3:] = (255, 60, 0)   # lit last columns in some rows
        big[:hh // 8, :2] = (255, 60, 0)           # ... and the first columns
        for bits, vbit in ((8, 0), (16, 3)):
            pattern = BR.PATTERNS[(gi + bits // 8) % 4]
            dp = RR.derived_pattern(pattern, ww, hh, mirror, flip)
            m = BR.mosaic(big, dp)
            dd = BR.demosaic(m, dp)
            r = synth.raw_frame(m, bits, vbit, mirror, flip, np.random.default_rng(gi))
            use(c, pattern, bits, vbit, mirror, flip)
            for morph in (MORPH_NONE, MORPH_CLOSE):
                want = oracle.extract_binary(dd, CAMP_BLUE, 60, morph)
                _, _, binary = c.extract_color_csr(r, CAMP_BLUE, 60, morph)  # rows back to back: unaligned for odd w
                assert np.array_equal(binary, want), (ww, hh, bits, morph, "dense")
                assert np.array_equal(extract_binary_strided(c, r, ww, hh, 13, CAMP_BLUE, 60, morph), want), (ww, hh, bits, morph, "padded")
            c.upload(np.stack([r, r]))
            c.run(default_params(), STAGE_ALL)
            c.sync()
            check_frame(c, 1, ref_frame(oracle, dd))
            # a device batch with rows and frames that are NOT 16-byte aligned: the byte-wise loader for every width
            import torch
            stride = (ww + 3) * (bits // 8)
            pitch = stride * hh + 2 * (bits // 8)
            buf = np.zeros(2 * pitch, np.uint8)
            for f in range(2):
                buf[f * pitch:f * pitch + hh * stride].view(r.dtype).reshape(hh, ww + 3)[:, :ww] = r
            t = torch.from_numpy(buf).cuda()
            c.bind_device_frames(t.data_ptr(), 2, hh, ww, stride, pitch, keepalive=t)
            c.run(default_params(), STAGE_ALL)
            c.sync()
            check_frame(c, 1, ref_frame(oracle, dd))
    assert c.check_guards()[0] == 0
    c.close()


# ---------------------------------------------------------------- 4. upload and export modes, the slow-copy rule
@pytest.mark.parametrize("upload", [0, 1, 2, 3])
@pytest.mark.parametrize("export", [0, 1])
def test_chain_upload_and_export_modes(oracle, upload, export):
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    c.set_option(OPT_FRAME_UPLOAD, upload)
    c.set_option(OPT_IMAGE_EXPORT, export)
    use(c, BR.BG, 16, 4, True, True)
    keep = []  # mode 2 pins the caller's buffers in place: they must outlive the context
    for i in range(3):  # (the second and third frames run ahead: the filters ride with extract_color)
        r, m, dp, d = scene(7200 + i, 1280, 1024, BR.BG, 16, 4, True, True)
        keep.append(r)
        binary, pts, offs, blobs, src, neg, arm = chain(c, r, CAMP_BLUE, 80, MORPH_CLOSE)
        ref = ref_frame(oracle, d)
        assert np.array_equal(binary, ref["binary"]) and np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"])
        assert blobs.tobytes() == ref["blobs"].tobytes() and arm.tobytes() == ref["armours"].tobytes()
    r, m, dp, d = scene(7210, 1280, 1024, BR.BG, 16, 4, True, True)
    assert np.array_equal(extract_binary_strided(c, r, 1280, 1024, 10, CAMP_BLUE, 80, MORPH_CLOSE), oracle.extract_binary(d, CAMP_BLUE, 80, MORPH_CLOSE))
    c.close()
    del keep


def test_chain_judges_a_slow_runtime_copy_by_two_bytes_per_pixel(oracle):
    """RMCV_OPT_FRAME_UPLOAD 3: the upload of a 16-bit mosaic is judged by its own 2 B/px (1280x1024: slow above 2.6 MB / 45 GB/s + 100 us
    = 158 us; a BGR frame's 3.9 MB would allow 187 us).  With 170 us added to what the library measures every frame is slow by that
    rule whatever the copy really took: three in a row and the chain moves to the pinned staging buffer; the results never change."""
    L = abi.lib()
    c = Context(device=0, max_frames=1, max_width=1280, max_height=1024)
    c.set_option(OPT_IMAGE_EXPORT, 0)
    use(c, BR.GR, 16, 2, True, True)
    r, m, dp, d = scene(7250, 1280, 1024, BR.GR, 16, 2, True, True)
    ref = ref_frame(oracle, d)

    def one():
        binary, pts, offs, blobs, src, neg, arm = chain(c, r, CAMP_BLUE, 80, MORPH_CLOSE)
        assert np.array_equal(binary, ref["binary"]) and np.array_equal(pts, ref["pts"]) and arm.tobytes() == ref["armours"].tobytes()
        us = (C.c_double * 9)()
        assert L.rmcv_ctx_frame_timing(c._h, us, 9) == 0
        return int(us[7])
    one()
    c.set_option(OPT_FRAME_UPLOAD, 3)
    c.set_option(OPT_TEST_SLOW_US, 170)
    seen = [one() for _ in range(5)]
    assert seen[0] == 0 and seen[3:] == [1, 1], seen
    c.close()


# ---------------------------------------------------------------- 5. batches
@pytest.fixture(scope="module")
def batch256(oracle):
    """256 x 1280x1024 delivered buffers (BG sensor, 16-bit samples with the pixel at bits 4..11, to be mirrored and flipped) and the
    oracle's results on D(T(r)) of each"""
    r, m, dp, d = scene(7300, 1280, 1024, BR.BG, 16, 4, True, True, n=256)
    assert dp == BR.RG
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda f: ref_frame(oracle, d[f]), range(256)))
    return r, refs


def test_batch_upload_256(batch256):
    r, refs = batch256
    c = Context(device=0, max_frames=256, max_width=1280, max_height=1024)
    use(c, BR.BG, 16, 4, True, True)
    c.upload(r)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    c.close()


def test_batch_torch_strided_pitched_no_image(batch256):
    import torch
    r, refs = batch256
    n, h, w = r.shape
    stride, pitch = 2 * 1344, 2 * 1344 * 1024 + 4096
    buf = np.zeros(n * pitch, np.uint8)
    for f in range(n):
        buf[f * pitch:f * pitch + h * stride].view(np.uint16).reshape(h, stride // 2)[:, :w] = r[f]
    t = torch.from_numpy(buf).cuda()
    c = Context(device=0, max_frames=256, max_width=1280, max_height=1024)
    use(c, BR.BG, 16, 4, True, True)
    c.bind_device_frames(t.data_ptr(), n, h, w, stride, pitch, keepalive=t)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    c.run(default_params(), STAGE_ALL | STAGE_NO_IMAGE)
    c.sync()
    check_batch(c, refs, image=False)
    # contiguous tensor, default stride (2 w with 16-bit samples)
    t2 = torch.from_numpy(r.view(np.uint8)).cuda()
    c.bind_device_frames(t2.data_ptr(), n, h, w, keepalive=t2)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    check_batch(c, refs)
    c.close()


def test_batch_dense_mid_tier(oracle):
    """hundreds of specks per frame: the contour stage's mid tier behind the oriented 16-bit loader"""
    n, w, h = 24, 1280, 1024
    mirror, flip, pattern = True, False, BR.GR
    dp = RR.derived_pattern(pattern, w, h, mirror, flip)
    bgr = synth.batch(7400, n, w, h, CAMP_BLUE, 0, threads=16)
    rng = np.random.default_rng(3)
    for f in range(n):
        ys, xs = rng.integers(2, h - 4, 600), rng.integers(2, w - 4, 600)
        for y, x in zip(ys, xs):
            bgr[f, y:y + 3, x:x + 3] = (255, 90, 10)
    m = BR.mosaic(bgr, dp)
    r = synth.raw_frame(m, 16, 2, mirror, flip, rng)
    d = [BR.demosaic(m[f], dp) for f in range(n)]
    with ThreadPoolExecutor(16) as ex:
        refs = list(ex.map(lambda f: ref_frame(oracle, d[f]), range(n)))
    assert max(len(x["offs"]) for x in refs) > 300
    c = Context(device=0, max_frames=n, max_width=w, max_height=h, max_contours=4096)
    use(c, pattern, 16, 2, mirror, flip)
    for tier in (0, 2):
        c.set_option(OPT_CONTOUR_TIER, tier)
        c.upload(r)
        c.run(default_params(), STAGE_ALL)
        c.sync()
        check_batch(c, refs)
    c.close()


# ---------------------------------------------------------------- 6. C5: identities, icons, poses
def test_c5_identity_pose_and_per_frame_classify(oracle):
    n, w, h = 24, 1920, 1200
    svm = synth.svm_weights()
    r, m, dp, d = scene(7500, w, h, BR.GB, 16, 4, True, True, n=n)
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    c.svm_load(*svm)
    c.pnp_load()
    use(c, BR.GB, 16, 4, True, True)
    c.upload(r)
    c.set_base2gripper(np.tile(np.eye(4), (n, 1, 1)))
    c.run(default_params(), STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    c.sync()
    arm, offs = c.armours()
    ident = c.identities()
    rv, tv, pv = c.poses()
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
        assert rv[sl].tobytes() == wr.tobytes() and tv[sl].tobytes() == wt.tobytes() and pv[sl].tobytes() == wp.tobytes(), f
    # per frame: rmcv_classify_armours on the delivered buffer, flipped only and 8-bit too
    f = int(np.argmax(np.diff(offs)))
    a0 = refs[f][1]
    ri, ra, ricons = oracle.classify_armours(d[f], a0, svm)
    gi, ga, gicons = c.classify_armours(r[f], a0)
    assert np.array_equal(gi, ri) and ga.tobytes() == ra.tobytes() and np.array_equal(gicons, ricons)
    use(c, RR.delivered_pattern(dp, w, h, False, True), 8, 0, False, True)
    gi, ga, gicons = c.classify_armours(RR.delivered(m[f], 8, 0, False, True), a0)
    assert np.array_equal(gi, ri) and ga.tobytes() == ra.tobytes() and np.array_equal(gicons, ricons)
    c.close()


# ---------------------------------------------------------------- 7. the pipeline
def test_pipeline_oriented_slots_and_bgr_beside(oracle):
    import torch
    dev = torch.device("cuda", 0)
    p = default_params()
    lay = dict(sample_bits=16, valid_bit=2, mirror=True, flip=True)
    geoms = [(64, 1280, 1024), (32, 640, 512), (48, 1024, 768)]
    raws, want = [], []
    for i, (n, w, h) in enumerate(geoms):
        r, m, dp, d = scene(7600 + 100 * i, w, h, BR.GR, 16, 2, True, True, n=n, variant=i % 2)
        raws.append(r)
        ctx = Context(device=0, max_frames=n, max_width=w, max_height=h)
        use(ctx, BR.GR, 16, 2, True, True)
        ctx.upload(r)
        ctx.run(p, STAGE_ALL)
        ctx.sync()
        want.append(ctx.armours())
        ctx.close()
        ref = ref_frame(oracle, d[0])  # (the contexts' results are the oracle's: test_batch_*; one frame of each here as well)
        assert want[i][0][want[i][1][0]:want[i][1][1]].tobytes() == ref["armours"].tobytes()

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
    pl = Pipeline(device=0, max_frames=64, max_width=1280, max_height=1024, input_format=BR.GR, **lay)
    devm = [torch.from_numpy(r.view(np.uint8)).to(dev) for r in raws]
    order = [0, 0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 0, 2, 2, 1, 0]
    tickets, got = [], {}
    lag = pl.depth - 1
    for i, k in enumerate(order):
        n, h, w = raws[k].shape
        tickets.append(pl.submit(devm[k].data_ptr(), n, h, w, p, STAGE_ALL))
        if i >= lag:
            got[i - lag] = pl.collect(tickets[i - lag])
    pl.drain()
    for i in range(max(0, len(order) - lag), len(order)):
        got[i] = pl.collect(tickets[i])
    for i, k in enumerate(order):
        arm, offs = got[i]
        assert arm.tobytes() == want[k][0].tobytes() and list(offs) == list(want[k][1]), (i, k)
    assert pl.get_info().host_blocking_calls == 0
    assert lib().rmcv_pixel_ws_launches() == ws0  # a Bayer batch never runs k_binary_ws
    with pytest.raises(RmcvError) as e:  # odd strides are refused at submit
        pl.submit(devm[0].data_ptr(), 64, 1024, 1280, p, STAGE_ALL, stride=2 * 1280 + 1, frame_pitch=(2 * 1280 + 1) * 1024 + 1)
    assert e.value.code == abi.ERR_BAD_ARG
    with pytest.raises(RmcvError) as e:
        pl.submit(devm[0].data_ptr(), 64, 1024, 1280, p, STAGE_ALL, legacy=LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1))
    assert e.value.code == abi.ERR_BAD_ARG
    pl.close()

    after = bgr_lists()
    for (a0, o0), (a1, o1) in zip(before, after):
        assert a0.tobytes() == a1.tobytes() and list(o0) == list(o1)


# ---------------------------------------------------------------- 8. refusals and the way back
def test_refusals_and_back_to_defaults(oracle):
    n, w, h = 4, 1280, 1024
    L = lib()
    bgr = synth.batch(7800, n, w, h, CAMP_BLUE, 0)
    c = Context(device=0, max_frames=n, max_width=w, max_height=h)
    r, m, dp, d = scene(7810, w, h, BR.RG, 16, 3, True, False)
    use(c, BR.RG, 16, 3, True, False)
    # unknown values are refused and the options stay: the frame still reads right afterwards
    for opt, bad in ((abi.OPT_INPUT_SAMPLE_BITS, 12), (abi.OPT_INPUT_SAMPLE_BITS, 0), (abi.OPT_INPUT_VALID_BIT, 5), (abi.OPT_INPUT_VALID_BIT, -1),
                     (abi.OPT_INPUT_ORIENT, 4), (abi.OPT_INPUT_ORIENT, -1), (abi.OPT_INPUT_FORMAT, 5)):
        assert L.rmcv_ctx_set_option(c._h, opt, bad) == abi.ERR_BAD_ARG, (opt, bad)
    _, _, binary = c.extract_color_csr(r, CAMP_BLUE, 80, MORPH_CLOSE)
    assert np.array_equal(binary, oracle.extract_binary(d, CAMP_BLUE, 80, MORPH_CLOSE))
    # 16-bit samples: strides are bytes and even, pointers 2-byte aligned
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.stack([r, r])).view(np.uint8)).cuda()
    for args, why in (((t.data_ptr(), 2, h, w, 2 * w + 1, (2 * w + 1) * h + 1), "even"), ((t.data_ptr(), 2, h, w, 2 * w, 2 * w * h - 1), "stride/pitch"),
                      ((t.data_ptr(), 2, h, w, 2 * w - 2, 2 * w * h), "stride/pitch"), ((t.data_ptr() + 1, 1, h, w, 2 * w, 2 * w * h), "aligned")):
        with pytest.raises(RmcvError) as e:
            c.bind_device_frames(*args)
        assert e.value.code == abi.ERR_BAD_ARG and why in str(e.value), (why, str(e.value))
    binary = np.empty((h, w), np.uint8)
    nc, npt = C.c_int32(0), C.c_int32(0)
    pts, offs = np.empty(c.limits.max_points, abi.POINT), np.empty(c.limits.max_contours + 1, np.int32)
    assert L.rmcv_extract_color(c._h, ptr(r), w, h, 2 * w + 1, CAMP_BLUE, 80, MORPH_CLOSE, ptr(binary), ptr(pts), len(pts), ptr(offs), len(offs) - 1,
                                C.byref(nc), C.byref(npt)) == abi.ERR_BAD_ARG
    assert L.rmcv_batch_upload(c._h, C.c_void_p(r.ctypes.data + 1), 1, w, h, 2 * w, C.c_int64(2 * w * h)) == abi.ERR_BAD_ARG
    # the legacy matcher keeps refusing every Bayer layout
    with pytest.raises(RmcvError) as e:
        c.run_legacy(LegacyParams(1.5, 80.0, 70.0, 10.0, 99999.0, 1))
    assert e.value.code == abi.ERR_BAD_ARG
    # BGR frames with a layout left on: refused by name, at every binding and per-frame call
    c.set_input_format(0)
    for bits, mirror, name in ((16, False, "RMCV_OPT_INPUT_SAMPLE_BITS"), (8, True, "RMCV_OPT_INPUT_ORIENT")):
        c.set_input_layout(bits, 0, mirror, False)
        for call in (lambda: c.upload(bgr), lambda: c.extract_color_csr(bgr[0]),
                     lambda: c.bind_device_frames(t.data_ptr(), 1, 16, 16)):
            with pytest.raises(RmcvError) as e:
                call()
            assert e.value.code == abi.ERR_BAD_ARG and name in str(e.value), (name, str(e.value))
    # defaults restored: identical to a fresh context
    c.set_input_layout()
    c.upload(bgr)
    c.run(default_params(), STAGE_ALL)
    c.sync()
    fresh = Context(device=0, max_frames=n, max_width=w, max_height=h)
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
    # ... and a plain 8-bit mosaic on a context that has read oriented 16-bit frames
    m8 = BR.mosaic(bgr[1], BR.GB)
    for x in (c, fresh):
        use(x, BR.GB)
    assert all(np.array_equal(a, b) for a, b in zip(c.extract_color_csr(m8), fresh.extract_color_csr(m8)))
    assert c.check_guards()[0] == 0 and fresh.check_guards()[0] == 0
    c.close()
    fresh.close()
