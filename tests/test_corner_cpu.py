"""Corner refinement on the CPU: rmcv_corner_subpix_host, rmcv_corner_mask and rmcv_gray_host against the numpy restatements
of tests/corner_ref.py, mpmath and the analytic corners of synthetic boards.  No GPU.

Measured on restatement (b) (OpenCV's sequential sums), never on the library: on the clean affine boards, windows 3 .. 8 in each axis, guesses
up to +-2.5 px, the refined corner lies within 0.00081 px of the analytic one (every case listed by ACCURACY_CASES); the bound below is ten
times that.  A half-pixel convention error is 0.5 px.  The library's results equal restatement (b) bit for bit on 62 of the 62 cases."""

import mpmath
import numpy as np
import pytest

import corner_cases as CC
import corner_ref as REF
import rmcv_amd as R
from rmcv_amd import abi, synth

ACCURACY_MEASURED_PX = 0.00081
ACCURACY_BOUND_PX = 10 * ACCURACY_MEASURED_PX
ACCURACY_CASES = [c for c in CC.CASES if c.image in CC.ACCURACY_BOARDS and len(c.corners) == 12 and 3 <= min(c.win) and max(c.win) <= 8]
BY_NAME = {c.name: c for c in CC.CASES}


def host(c):
    return R.corner_subpix_host(CC.IMAGES[c.image], c.corners, c.win, c.zero, c.max_iters, c.eps)


@pytest.fixture(scope="module")
def seq():
    """restatement (b) on every case, once"""
    return {c.name: REF.subpix(CC.IMAGES[c.image], c.corners, c.win, c.zero, c.max_iters, c.eps, pinned=False) for c in CC.CASES}


def test_case_list_covers_every_branch():
    assert len(BY_NAME) == len(CC.CASES)
    st = np.concatenate([host(c)[1] for c in CC.CASES])
    for bit in (R.CORNER_DET_ZERO, R.CORNER_LEFT_IMAGE, R.CORNER_REVERTED, R.CORNER_CONVERGED, R.CORNER_BAD_INPUT):
        assert (st & bit).any(), hex(bit)
    iters = st & R.CORNER_ITERS_MASK
    assert (iters == 40).any() and (iters == 1).any() and (iters == 0).any()
    assert {c.win for c in CC.CASES} >= set(CC.WINDOWS) and {c.zero for c in CC.CASES} == set(CC.ZERO_ZONES)
    assert host(BY_NAME["flat-det-zero"])[1].tolist() == [1 | R.CORNER_DET_ZERO]
    far = BY_NAME["far-flat-window"]
    assert host(far)[1].tolist() == [1 | R.CORNER_DET_ZERO] and host(far)[0].tobytes() == far.corners.tobytes()
    assert host(BY_NAME["reverted"])[1][0] & R.CORNER_REVERTED and host(BY_NAME["reverted"])[0].tobytes() == BY_NAME["reverted"].corners.tobytes()
    near = host(BY_NAME["leaves-image-near"])
    assert near[1][0] & R.CORNER_LEFT_IMAGE and not near[1][0] & R.CORNER_REVERTED and near[0][0][1] < 0
    nan = host(BY_NAME["nan"])
    assert nan[1].tolist() == [R.CORNER_BAD_INPUT] * 2 and nan[0].tobytes() == BY_NAME["nan"].corners.tobytes()
    assert host(BY_NAME["max-iters-1"])[1].tolist() == [1]


@pytest.mark.parametrize("name", [c.name for c in CC.CASES])
def test_host_equals_pinned_restatement(name):
    c = BY_NAME[name]
    out, st = host(c)
    ref, ref_st = REF.subpix(CC.IMAGES[c.image], c.corners, c.win, c.zero, c.max_iters, c.eps, pinned=True)
    assert st.tolist() == ref_st.tolist()
    assert out.tobytes() == ref.tobytes()


def test_mask_equals_mpmath():
    cache = {}

    def exp(v):  # the exponential correctly rounded to double
        if v not in cache:
            with mpmath.workprec(200):
                cache[v] = float(mpmath.exp(mpmath.mpf(v)))
        return cache[v]

    differing = []
    for wx in range(1, 16):
        for wy in range(1, 16):
            ref = REF.mask(wx, wy, exp=exp)
            got = R.corner_mask((wx, wy))
            assert got.shape == (2 * wy + 1, 2 * wx + 1) and got.dtype == np.float32
            if got.tobytes() != ref.tobytes():
                differing.append((wx, wy, int((got != ref).sum())))
    assert differing == []   # (pm_exp is within 2 ulp of the true value only: an entry that differed here would be a finding, not a tolerance)


def test_mask_zero_zones_and_refusals():
    for win, zero in (((8, 8), (0, 0)), ((8, 8), (2, 1)), ((3, 5), (2, 4)), ((15, 15), (14, 14))):
        full, m = R.corner_mask(win), R.corner_mask(win, zero)
        ref = full.copy()
        ref[win[1] - zero[1]:win[1] + zero[1] + 1, win[0] - zero[0]:win[0] + zero[0] + 1] = 0
        assert m.tobytes() == ref.tobytes() and (m == 0).sum() == (2 * zero[0] + 1) * (2 * zero[1] + 1)
    for win, zero in (((0, 3), (-1, -1)), ((3, 16), (-1, -1)), ((3, 3), (3, 0)), ((3, 3), (0, 3)), ((3, 3), (-1, 0)), ((3, 3), (0, -1)), ((3, 3), (-2, -2))):
        with pytest.raises(R.RmcvError):
            R.corner_mask(win, zero)


def test_gray_equals_integer_formula():
    rng = np.random.default_rng(20241021)
    cube = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    px = np.concatenate([rng.integers(0, 256, (1 << 20, 3), dtype=np.uint8), cube]).reshape(1, -1, 3)
    got = R.gray_host(px)
    v = px.astype(np.int64)
    ref = (1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14
    assert ref.max() == 255 and ref.min() == 0
    assert np.array_equal(got, ref.astype(np.uint8))
    assert np.array_equal(REF.gray(px), got)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert R.gray_host(grey)[0].tolist() == list(range(256))   # equal channels keep their value


def test_padded_rows_and_null_status():
    c = BY_NAME["edge160-win8x8"]
    img = CC.IMAGES[c.image]
    h, w = img.shape[:2]
    wide = np.full((h, 3 * w + 7), 0xA5, np.uint8)
    wide[:, :3 * w] = img.reshape(h, 3 * w)
    cor = c.corners.copy()
    rc = abi.lib().rmcv_corner_subpix_host(abi.ptr(wide), w, h, wide.shape[1], abi.ptr(cor), len(cor), 8, 8, -1, -1, 40, 0.001, None)
    assert rc == 0 and cor.tobytes() == host(c)[0].tobytes()
    g = np.zeros((h, w + 5), np.uint8)
    assert abi.lib().rmcv_gray_host(abi.ptr(wide), w, h, wide.shape[1], abi.ptr(g), w + 5) == 0
    assert np.array_equal(g[:, :w], R.gray_host(img)) and not g[:, w:].any()


def test_host_refusals():
    img = CC.IMAGES["affine96"]
    cor = np.zeros((2, 2), np.float32)
    st = np.zeros(2, np.int32)
    L = abi.lib()

    def call(bgr=img, w=96, h=80, stride=288, corners=cor, n=2, win=(8, 8), zero=(-1, -1), iters=40, eps=0.001):
        return L.rmcv_corner_subpix_host(abi.ptr(bgr), w, h, stride, abi.ptr(corners), n, win[0], win[1], zero[0], zero[1], iters, eps, abi.ptr(st))

    assert call() == 0 and call(n=0) == 0 and call(n=0, corners=None) == 0
    for kw in (dict(bgr=None), dict(corners=None), dict(w=0), dict(h=0), dict(stride=287), dict(n=-1), dict(win=(0, 8)), dict(win=(8, 16)), dict(zero=(8, 0)),
               dict(zero=(0, -1)), dict(iters=0), dict(iters=101), dict(eps=-1e-9), dict(eps=float("nan")), dict(eps=float("inf"))):
        assert call(**kw) == abi.ERR_BAD_ARG, kw
    assert call(iters=100, eps=0.0, win=(15, 1), zero=(14, 0)) == 0
    assert L.rmcv_gray_host(None, 4, 4, 12, abi.ptr(st), 4) == abi.ERR_BAD_ARG
    assert L.rmcv_gray_host(abi.ptr(img), 96, 80, 288, abi.ptr(np.zeros((80, 96), np.uint8)), 95) == abi.ERR_BAD_ARG
    assert L.rmcv_corner_mask(3, 3, -1, -1, None) == abi.ERR_BAD_ARG


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_against_sequential_sums(seq):
    """restatement (b): every coordinate within 1 float32 ulp, iteration counts equal wherever the coordinates are bit-equal"""
    equal = 0
    for c in CC.CASES:
        out, st = host(c)
        ref, ref_st = seq[c.name]
        fin = np.isfinite(ref).all(axis=1)
        assert np.array_equal(fin, np.isfinite(out).all(axis=1)) and out[~fin].tobytes() == ref[~fin].tobytes()
        assert ulps(out[fin], ref[fin]).max(initial=0) <= 1, c.name
        same = (out.view(np.int32) == ref.view(np.int32)).all(axis=1)
        assert np.array_equal(st[same], ref_st[same]), c.name
        equal += out.tobytes() == ref.tobytes()
    print("bit-equal with the sequential sums: %d of %d cases" % (equal, len(CC.CASES)))
    assert equal >= len(CC.CASES) - 3   # (all, or nearly all: DESIGN.md 4s records the count)


def test_accuracy_on_affine_boards(seq):
    assert len(ACCURACY_CASES) >= 12 and {c.image for c in ACCURACY_CASES} == set(CC.ACCURACY_BOARDS)
    worst_ref = worst = 0.0
    for c in ACCURACY_CASES:
        truth = CC.TRUTH[c.image]
        out, st = host(c)
        assert ((st & R.CORNER_CONVERGED) != 0).all() and not (st & R.CORNER_REVERTED).any(), c.name
        worst_ref = max(worst_ref, float(np.abs(seq[c.name][0] - truth).max()))
        worst = max(worst, float(np.abs(out - truth).max()))
    print("largest distance from the analytic corner: restatement (b) %.6f px, library %.6f px; bound %.5f px" % (worst_ref, worst, ACCURACY_BOUND_PX))
    assert worst_ref <= ACCURACY_MEASURED_PX   # (the measurement the bound was set from still holds for the generator)
    assert worst <= ACCURACY_BOUND_PX


def test_chessboard_generator():
    img, truth = synth.chessboard(96, 80, CC.H_AFFINE_96, 5, 4)
    assert img.shape == (80, 96, 3) and img.dtype == np.uint8 and truth.shape == (12, 2)
    assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
    assert set(np.unique(img)) >= {40, 215} and img.min() == 40 and img.max() == 215
    assert truth[0].tolist() == [14.5 + 14 + 2, 16.0 - 1 + 13] and truth[-1].tolist() == [14.5 + 4 * 14 + 3 * 2, 16.0 - 4 + 3 * 13]
    # pixel centres at integers: about truth[0] = (30.5, 28.0) the board is point-symmetric, so pixel (31 + dx, 28 + dy) equals (30 - dx, 28 - dy)
    g = img[..., 0]
    for dy in range(-5, 6):
        for dx in range(0, 6):
            assert g[28 + dy, 31 + dx] == g[28 - dy, 30 - dx]
    assert g[28, 31] not in (40, 215) and g[22, 36] in (40, 215)   # (an edge pixel is a mixture; the inside of a square is not)
    img8, _ = synth.chessboard(96, 80, CC.H_AFFINE_96, 5, 4, ss=8, lo=0, hi=255)
    assert img8.min() == 0 and img8.max() == 255
    assert np.array_equal(synth.chessboard(96, 80, CC.H_AFFINE_96, 5, 4)[0], img)
