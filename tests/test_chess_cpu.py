"""The chessboard detector on the CPU: rmcv_find_chessboard_host, the sequential form of rmcv_amd/csrc/device_chess.h, against
tests/chess_ref.py (the header's text restated in numpy) byte for byte on every case of tests/chess_cases.py -- candidates with their responses,
corners, status; the response against a direct evaluation in Python integers; what is known of each case beforehand; the accuracy conditions;
every refusal.  No GPU.

Measured on these cases: the coarse corners of the clean boards lie within 1.5 px (max-norm) of the analytic ones (bound 2.5 px, the range
tests/corner_cases.py refines from); after find -> refine the clean affine boards lie within 0.00064 px (bound 0.0081 px)."""
import ctypes as C

import numpy as np
import pytest

import chess_cases as CC
import chess_ref as REF
import rmcv_amd as R
from rmcv_amd import abi

NAMES = [c.name for c in CC.CASES]
COARSE_BOUND = 2.5


def host(c):
    return R.find_chessboard_host(CC.IMAGES[c.image], c.cols, c.rows, c.params)


@pytest.fixture(scope="module")
def results():
    return {c.name: host(c) for c in CC.CASES}


def test_constants_and_defaults():
    assert (R.CHESS_COUNT_MASK, R.CHESS_FOUND, R.CHESS_OVERFLOW, R.CHESS_NO_GRID, R.CHESS_CAND_MAX) == (REF.COUNT_MASK, REF.FOUND, REF.OVERFLOW, REF.NO_GRID, REF.CAND_MAX)
    assert R.chess_defaults() == REF.DEFAULTS == dict(threshold=1000, contrast=10, nms=3, dist_min=6, dist_max=255)
    assert R.chess_params(dict(nms=2), contrast=7).tolist() == [1000, 7, 2, 6, 255]


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_the_restatement(name, results):
    c = CC.BY_NAME[name]
    cor, st, cand = results[name]
    ref, ref_st, ref_cand = REF.find(CC.IMAGES[c.image], c.cols, c.rows, **c.params)
    assert st == ref_st
    assert cand.dtype == ref_cand.dtype and cand.tobytes() == ref_cand.tobytes()
    assert (cor is None) == (ref is None) and (cor is None or (cor.dtype == ref.dtype and cor.tobytes() == ref.tobytes()))


def test_cases_are_what_they_are_said_to_be(results):
    assert len(CC.BY_NAME) == len(CC.CASES)
    worst = 0.0
    for c in CC.CASES:
        cor, st, cand = results[c.name]
        assert (cor is not None) == c.found == bool(st & R.CHESS_FOUND), c.name
        assert bool(st & R.CHESS_NO_GRID) == (not c.found and not st & R.CHESS_OVERFLOW), c.name
        if c.found:
            assert len(cand) == st & R.CHESS_COUNT_MASK
            assert np.array_equal(cor, np.floor(cor)) and cor.shape == (c.cols * c.rows, 2)
            err = np.abs(cor - c.analytic).max()
            print("%-24s candidates %3d coarse error %.3f px" % (c.name, len(cand), err))
            assert not c.clean or err <= COARSE_BOUND, c.name      # (the analytic order: the orientation is the rule's)
            worst = max(worst, err) if c.clean else worst
    print("worst coarse error on the clean boards: %.3f px" % worst)
    n = lambda name: len(results[name][2])
    assert [n(k) for k in ("upright-5x4", "persp1-8x6", "persp1-8x6-noise8", "squares13-11x8", "long-32x2", "upright-2x2")] == [20, 48, 48, 88, 64, 4]   # the analytic count
    assert n("persp2-8x6-cropped") == 47 and n("corner-outside-5x4") == 19 and n("two-boards-3x3") == 18   # one corner lost; both boards seen
    assert results["blank"][1] == R.CHESS_NO_GRID and n("blank") == 0
    st = results["noise-overflow"][1]
    assert st & R.CHESS_OVERFLOW and not st & (R.CHESS_FOUND | R.CHESS_NO_GRID) and st & R.CHESS_COUNT_MASK > R.CHESS_CAND_MAX and n("noise-overflow") == 0
    # the mirror image is found, and what is returned is right-handed
    g = results["mirror-5x4"][0].reshape(4, 5, 2)
    a, b = g[0, 1] - g[0, 0], g[1, 0] - g[0, 0]
    assert a[0] * b[1] - a[1] * b[0] > 0
    # the square pattern starts at the corner with the smallest x + y of its four
    g = results["rot0.7-6x6"][0].reshape(6, 6, 2)
    assert g[0, 0].sum() == min(p.sum() for p in (g[0, 0], g[0, -1], g[-1, 0], g[-1, -1]))


def exact_response(g, x, y):
    """R at (x, y) of a gray image (a list of lists of Python integers), term by term from the rule's text"""
    ring = [g[y + dy][x + dx] for dx, dy in REF.RING]
    sr = sum(abs((ring[n] + ring[n + 8]) - (ring[n + 4] + ring[n + 12])) for n in range(4))
    dr = sum(abs(ring[n] - ring[n + 8]) for n in range(8))
    loc = g[y][x] + g[y][x - 1] + g[y][x + 1] + g[y - 1][x] + g[y + 1][x]
    return 5 * sr - 5 * dr - abs(5 * sum(ring) - 16 * loc)


def test_response_equals_exact_integers():
    """11 x 11 patches: the middle pixel alone lies 5 from every edge, so it is the only candidate, exactly when its R exceeds the threshold"""
    rng = np.random.default_rng(20241022)
    seen_pos = seen_neg = 0
    for k in range(400):
        levels = rng.integers(0, 256, (2, 2))
        if k % 2:
            levels[1, 1], levels[1, 0] = levels[0, 0], levels[0, 1]                  # a chessboard corner
        patch = np.kron(levels, np.ones((6, 6), np.int64))[:11, :11] + rng.integers(-20, 21, (11, 11))
        if k % 5 == 0:
            patch = rng.integers(0, 256, (11, 11))
        bgr = np.clip(patch, 0, 255).astype(np.uint8)[:, :, None].repeat(3, axis=2)
        bgr[..., 0] = rng.integers(0, 256, (11, 11))                                  # (the channels differ: gray is part of what is checked)
        gray = [[(1868 * int(p[0]) + 9617 * int(p[1]) + 4899 * int(p[2]) + 8192) >> 14 for p in row] for row in bgr]
        want = exact_response(gray, 5, 5)
        threshold = int(rng.integers(0, 3000))
        cor, st, cand = R.find_chessboard_host(bgr, 2, 2, threshold=threshold)
        assert cor is None and cand.tolist() == ([[5, 5, want]] if want > threshold else []), (k, want, threshold)
        _, _, zero = R.find_chessboard_host(bgr, 2, 2, threshold=0, nms=7)
        assert zero.tolist() == ([[5, 5, want]] if want > 0 else [])
        seen_pos += want > 0
        seen_neg += want <= 0
    assert seen_pos >= 50 and seen_neg >= 50


def test_threshold_and_ties():
    """an R equal to the threshold is no candidate; of two equal maxima in one neighbourhood the earlier in row-major order stays"""
    c = CC.BY_NAME["upright-5x4"]
    cand = host(c)[2]
    lowest = int(cand[:, 2].min())
    assert len(R.find_chessboard_host(CC.IMAGES[c.image], 5, 4, threshold=lowest)[2]) < len(cand) == len(R.find_chessboard_host(CC.IMAGES[c.image], 5, 4, threshold=lowest - 1)[2])
    img = np.full((40, 40, 3), 215, np.uint8)
    img[:20, :20] = img[20:, 20:] = 40                     # one corner between pixels: R is the same at its four pixels
    r = REF.response(REF.gray(img))
    assert r[19, 19] == r[19, 20] == r[20, 19] == r[20, 20] == r.max()
    assert R.find_chessboard_host(img, 2, 2)[2].tolist() == [[19, 19, int(r.max())]]


def test_padded_rows_and_null_outputs():
    c = CC.BY_NAME["rot0.52-5x4"]
    img = CC.IMAGES[c.image]
    h, w = img.shape[:2]
    want, want_st, want_cand = host(c)
    stride = 3 * w + 13
    padded = np.full(stride * (h - 1) + 3 * w, 0x5A, np.uint8)
    np.lib.stride_tricks.as_strided(padded, (h, 3 * w), (stride, 1))[:] = img.reshape(h, 3 * w)
    L = abi.lib()
    out = abi.chess_outputs(5, 4)
    assert L.rmcv_find_chessboard_host(abi.ptr(padded), w, h, stride, 5, 4, None, *[abi.ptr(a) for a in out]) == 0     # (null parameters: the defaults)
    cor, st, cand = abi.chess_result(out)
    assert cor.tobytes() == want.tobytes() and st == want_st and cand.tobytes() == want_cand.tobytes()
    cor = np.zeros((20, 2), np.float32)
    assert L.rmcv_find_chessboard_host(abi.ptr(img), w, h, 3 * w, 5, 4, None, abi.ptr(cor), None, None, None) == 0
    assert cor.tobytes() == want.tobytes()
    keep = np.full((20, 2), 7.25, np.float32)            # no board: the corner row is not touched
    st = np.zeros(1, np.int32)
    assert L.rmcv_find_chessboard_host(abi.ptr(CC.IMAGES["blank"]), 160, 128, 480, 5, 4, None, abi.ptr(keep), abi.ptr(st), None, None) == 0
    assert (keep == 7.25).all() and st[0] == R.CHESS_NO_GRID


def test_host_refusals():
    img = CC.IMAGES["upright-5x4"]
    L = abi.lib()
    out = abi.chess_outputs(5, 4)
    o = [abi.ptr(a) for a in out]
    ok = R.chess_params()
    call = lambda bgr=abi.ptr(img), w=160, h=128, stride=480, cols=5, rows=4, prm=ok, cor=o[0]: L.rmcv_find_chessboard_host(bgr, w, h, stride, cols, rows, abi.ptr(prm), cor, *o[1:])
    assert call() == 0
    for bad in (dict(bgr=None), dict(cor=None), dict(w=0), dict(h=0), dict(w=32768), dict(h=32768), dict(stride=479), dict(cols=1), dict(rows=1), dict(cols=33), dict(rows=33)):
        assert call(**bad) == abi.ERR_BAD_ARG, bad
    for bad in (dict(threshold=-1), dict(contrast=-1), dict(contrast=256), dict(nms=0), dict(nms=8), dict(dist_min=0), dict(dist_min=30, dist_max=29), dict(dist_max=1024)):
        assert call(prm=R.chess_params(bad)) == abi.ERR_BAD_ARG, bad
        with pytest.raises(R.RmcvError, match="rmcv_find_chessboard_host"):
            R.find_chessboard_host(img, 5, 4, bad)
    for good in (dict(threshold=0), dict(contrast=0), dict(contrast=255), dict(nms=1), dict(nms=7), dict(dist_min=1), dict(dist_min=255), dict(dist_max=1023), dict(cols=32, rows=32),
                 dict(cols=2, rows=2)):
        kw = {k: good.pop(k) for k in ("cols", "rows") if k in good}
        big = np.zeros((1024, 2), np.float32)
        assert call(prm=R.chess_params(good), cor=abi.ptr(big), **kw) == 0, good


def test_accuracy_after_refinement():
    """find -> refine with the two host functions on the clean affine boards: within the refinement's own bound of the analytic corners"""
    worst = 0.0
    for name in CC.ACCURACY:
        c = CC.BY_NAME[name]
        cor, st, _ = host(c)
        assert cor is not None and np.abs(cor - c.analytic).max() <= COARSE_BOUND
        for win in CC.ACCURACY_WINDOWS:
            fine, fst = R.corner_subpix_host(CC.IMAGES[c.image], cor, win)
            err = np.abs(fine - c.analytic).max()
            print("%-16s win %s: %.5f px" % (name, win, err))
            assert (fst & R.CORNER_CONVERGED).all() and err <= CC.ACCURACY_BOUND, (name, win)
            worst = max(worst, err)
    print("worst after refinement: %.5f px" % worst)
