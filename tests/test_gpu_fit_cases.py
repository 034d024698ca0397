"""The contour cases of tests/fit_cases.py -- one for every branch of fit_ellipse_wave (rmcv_amd/csrc/wave_detect.h); tests/test_fit_cases_cpu.py
shows on the oracle that each reaches its branch -- through EVERY call site of the fit on the device, against the oracle's bytes:

* rmcv_fit_ellipse, one contour at a time (k_fit);
* rmcv_filter_lightblobs on all point lists as one multi-contour call (k_fit + k_pairs): the positive list, its order and source indices
  and the negative list, with the reference's gates and with every gate open (ratio_hi = +inf: a zero-width ellipse, ratio = inf, is a
  positive; 0 / 0 = NaN is a negative);
* rmcv_match_lightblob with fit_ellipse = 1 (k_match);
* for the cases that are real borders, one frame through rmcv_batch_run with RMCV_OPT_SPARSE_WAVES 8 and 4 (the values the option takes) and
  RMCV_OPT_CONTOUR_TIER 0, 1 and 2 -- both fit sites of the fused sparse kernel (k_contours_kernel.inc: the work list in LDS, and in
  global memory behind the mid tier or the literal scanner) -- comparing the byte image, the contours, the blobs and the armours.  The
  1920 x 1200 comb frame takes the 2^24 branch of the coordinate sums within the default limits.

... and what the entry points refuse: a negative coordinate is RMCV_ERR_BAD_ARG on the host, and the context stays usable."""
import numpy as np
import pytest

import fit_cases as F
from rmcv_amd import MORPH_NONE, OPT_CONTOUR_TIER, OPT_SPARSE_WAVES, STAGE_ALL, Context, RmcvError, default_params

pytestmark = pytest.mark.gpu

CASES = F.point_cases()
IMAGES = F.image_cases()
INF = float("inf")
BAD_ARG = -1


def _finite(box):
    return all(np.isfinite(box[f]) for f in ("cx", "cy", "w", "h", "angle"))


def test_fit_ellipse_every_point_case(ctx, oracle):
    failures, refused = [], 0
    for c in CASES:
        ref, _ = oracle.fit_ellipse_direct(c.pts)
        if _finite(ref):       # RMCV_OK and the oracle's bytes for every finite result, zero width included
            got = ctx.fit_ellipse(c.pts)
            if got.tobytes() != ref.tobytes():
                failures.append((c.name, tuple(got), tuple(ref)))
        else:                  # a NaN result is refused (rmcv_abi.h)
            with pytest.raises(RmcvError) as e:
                ctx.fit_ellipse(c.pts)
            assert e.value.code == BAD_ARG, c.name
            refused += 1
    assert not failures, failures
    by = {c.name: c for c in CASES}
    for name in F.DEGENERATE:  # finite, of zero width: these were refused once
        assert ctx.fit_ellipse(by[name].pts).tobytes() == oracle.fit_ellipse_direct(by[name].pts)[0].tobytes(), name


def _csr():
    pts = np.concatenate([c.pts for c in CASES])
    offs = np.cumsum([0] + [len(c.pts) for c in CASES]).astype(np.int32)
    return pts, offs


@pytest.mark.parametrize("gates", ["reference", "open"])
def test_filter_lightblobs_all_cases_in_one_call(ctx, oracle, gates):
    pts, offs = _csr()
    assert len(pts) <= ctx.limits.max_points and len(CASES) <= ctx.limits.max_contours
    if gates == "reference":
        kw = dict(tilt_max=70.0, ratio_range=(1.5, 80.0), area_range=(10.0, 99999.0))
    else:
        kw = dict(tilt_max=1e30, ratio_range=(0.0, INF), area_range=(0.0, 1e300))
    p = oracle.default_params(tilt_max=kw["tilt_max"], ratio_lo=kw["ratio_range"][0], ratio_hi=kw["ratio_range"][1], area_lo=kw["area_range"][0],
                              area_hi=kw["area_range"][1])
    rb, rs, rn = oracle.filter_lightblobs(pts, offs, p)
    assert len(rb) <= ctx.limits.max_blobs
    blobs, src, neg = ctx.filter_lightblobs(pts, offs, **kw)
    names = [c.name for c in CASES]
    assert src.tolist() == rs.tolist(), ([names[i] for i in src], [names[i] for i in rs])
    assert neg.tolist() == rn.tolist(), ([names[i] for i in neg], [names[i] for i in rn])
    bad = [names[s] for s, a, b in zip(src, blobs, rb) if a.tobytes() != b.tobytes()]
    assert not bad, bad
    if gates == "open":        # every contour is judged; the degenerate ones land where the oracle puts them
        assert len(src) + len(neg) == len(CASES)
        where = {names[i]: "positive" for i in src}
        where.update({names[i]: "negative" for i in neg})
        assert where["direct_none_collinear_horizontal"] == "positive" and where["direct_jittered_two_rows"] == "positive"   # ratio = inf
        assert where["direct_none_all_equal"] == "negative"                                                                  # ratio = NaN


@pytest.mark.parametrize("gates", [(1.5, 80.0, 70.0, 10.0, 99999.0), (0.0, INF, 1e30, -1.0, 3e38)])
def test_match_lightblob_with_fit_ellipse(ctx, oracle, gates):
    failures, matched = [], 0
    for c in CASES:
        ok_o, box_o = oracle.match_lightblob(c.pts, *gates, True)
        ok_g, box_g = ctx.match_lightblob(c.pts, *gates, True)
        if ok_g != ok_o or (ok_o and box_g.tobytes() != box_o.tobytes()):
            failures.append((c.name, ok_g, ok_o, tuple(box_g), tuple(box_o)))
        matched += ok_o
    assert not failures, failures
    assert matched > 0


def test_negative_coordinates_are_refused_and_the_context_stays_usable(ctx, oracle):
    by = {c.name: c for c in CASES}
    good = by["direct_first_n64"].pts
    want = oracle.fit_ellipse_direct(good)[0]
    for field, value in (("x", -1), ("y", -30000), ("x", -(1 << 31))):
        bad = good.copy()
        bad[field][5] = value
        offs = np.array([0, len(bad)], np.int32)
        for call in (lambda: ctx.fit_ellipse(bad), lambda: ctx.filter_lightblobs(bad, offs),
                     lambda: ctx.match_lightblob(bad, 1.5, 80.0, 70.0, 10.0, 99999.0, True)):
            with pytest.raises(RmcvError) as e:
                call()
            assert e.value.code == BAD_ARG and "negative" in str(e.value)
            assert ctx.fit_ellipse(good).tobytes() == want.tobytes()          # the same context, right away
    # a multi-contour list whose LAST contour holds the negative point
    pts = np.concatenate([good, bad])
    offs = np.array([0, len(good), 2 * len(good)], np.int32)
    with pytest.raises(RmcvError) as e:
        ctx.filter_lightblobs(pts, offs)
    assert e.value.code == BAD_ARG
    rb, rs, rn = oracle.filter_lightblobs(good, offs[:2])
    blobs, src, neg = ctx.filter_lightblobs(good, offs[:2])
    assert blobs.tobytes() == rb.tobytes() and src.tolist() == rs.tolist() and neg.tolist() == rn.tolist()
    assert ctx.check_guards()[0] == 0


@pytest.fixture(scope="module")
def frame_ctx():
    c = Context(device=0, max_frames=1)          # the default limits: 1920 x 1200, 65 536 points
    yield c
    c.close()


@pytest.fixture(scope="module")
def image_refs(oracle):
    """the oracle's frames, computed once: {(image, gates): detect_frame}"""
    out = {}
    for ic in IMAGES:
        for gates, kw in (("reference", {}), ("open", dict(tilt_max=1e30, ratio_lo=0.0, ratio_hi=INF, area_hi=1e300))):
            out[ic.name, gates] = (kw, oracle.detect_frame(F.frame_of(ic.mask), oracle.default_params(morph=oracle.MORPH_NONE, area_lo=0.0, **kw)))
    return out


@pytest.mark.parametrize("waves,tier", [(8, 0), (4, 0), (8, 2), (4, 2), (8, 1), (4, 1)])
@pytest.mark.parametrize("image", [ic.name for ic in IMAGES])
def test_batch_run_on_real_borders(frame_ctx, image_refs, image, waves, tier):
    c = frame_ctx
    mask = {ic.name: ic.mask for ic in IMAGES}[image]
    c.set_option(OPT_SPARSE_WAVES, waves)
    c.set_option(OPT_CONTOUR_TIER, tier)
    c.upload(F.frame_of(mask)[None])
    for gates in ("reference", "open"):
        kw, ref = image_refs[image, gates]
        c.run(default_params(morph=MORPH_NONE, area_lo=0.0, **kw), STAGE_ALL)
        c.sync()
        assert not (int(c.counts()["status"][0]) & 15), (gates, c.counts())
        assert np.array_equal(c.binary(0), ref["binary"]), gates
        pts, offs = c.contours(0)
        assert np.array_equal(offs, ref["offs"]) and np.array_equal(pts, ref["pts"]), gates
        blobs, _ = c.blobs(0)
        assert blobs.tobytes() == ref["blobs"].tobytes(), (gates, len(blobs), len(ref["blobs"]))
        arm, aoffs = c.armours()
        assert arm[aoffs[0]:aoffs[1]].tobytes() == ref["armours"].tobytes(), (gates, len(arm), len(ref["armours"]))
    if image == "comb_2p24":
        assert len(ref["blobs"]) == 1                                       # the comb's border was fitted, not skipped
    else:
        assert len(ref["blobs"]) >= 4
