"""rm::AutoEnhance / rm::CalcGamma without a GPU: enhance_math.h (the gamma, the table builder with the pinned pow, the pixel kernel's
threshold table) compiled with gcc, against tests/enhance_ref.py (numpy + the host libm); the host-side ABI entry points; and the test
inputs themselves -- the dimmed synthetic frames on which the plain and the enhanced path disagree."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import enhance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <math.h>
#include "rmcv_amd/csrc/enhance_math.h"
void t_lut(float g, unsigned char* o) { for (int i = 0; i < 256; i++) o[i] = enh_lut_entry(i, g); }
float t_gamma(const uint64_t* s, int64_t n, float hi, float lo) { return enh_gamma(s, n, hi, lo); }
void t_m(const unsigned char* lut, int lb, unsigned short* o) { for (int b = 0; b < 256; b++) o[b] = enh_m_entry(lut, b, lb); }
double t_pow(double x, double g) { return pm_pow(x, g); }
'''
GAINS = [(100.0, 50.0), (30.0, 5.0)]
N_GAMMAS = 3798  # distinct float32 gammas of contract_gammas()
LARGE_GAMMAS = [22.0, 64.0, 127.0, 128.0, 129.0, 133.5, 134.0, 135.0, 254.0, 383.0, 384.0, 385.0, 400.0, 509.0, 1000.0, 1e5, 1e30, 3.4028234e38]


@pytest.fixture(scope="module")
def em(tmp_path_factory):
    d = tmp_path_factory.mktemp("em")
    c = d / "em.c"
    c.write_text(SRC)
    so = d / "em.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", ROOT, str(c), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    L.t_lut.argtypes = [C.c_float, C.c_void_p]
    L.t_gamma.restype = C.c_float
    L.t_gamma.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_float]
    L.t_m.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.t_pow.restype = C.c_double
    L.t_pow.argtypes = [C.c_double, C.c_double]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def contract_gammas():
    """every gamma the contract yields from meanC3 in linspace(0, 255, 1501) and j / 7, j < 400, with both gain pairs, plus five fixed ones
    and LARGE_GAMMAS: 3 798 distinct float32 values"""
    gs = set()
    for gains in GAINS:
        for m in list(np.linspace(0, 255, 1501)) + [j / 7 for j in range(400)]:
            gs.add(float(R.gamma_from_mean(m, *gains)))
    gs |= {0.0, 0.5, 1.0, 2.2, 9.2}
    # ... and gammas far beyond those: every finite gamma >= 0 is accepted (rmcv_calc_gamma, gains such as (2, 1) on a bright frame give
    # 509), and from ~128 on pow(1 / 255, g) leaves the normal range of a double
    gs |= {float(np.float32(g)) for g in LARGE_GAMMAS}
    return sorted(gs)


def pinned_lut(em, g):
    o = np.empty(256, np.uint8)
    em.t_lut(g, _p(o))
    return o


def test_pinned_table_equals_libm_table(em):
    gs = contract_gammas()
    assert len(gs) == N_GAMMAS and min(gs) == 0.0 and max(gs) > 3e38
    for g in gs:
        got, want = pinned_lut(em, g), R.lut(g)
        assert np.array_equal(got, want), (g, np.nonzero(got != want)[0][:8])


def test_pinned_pow_is_close_to_libm(em):
    """the table needs 1e-9 (no entry of the contract's gammas is closer than 3e-7 to a rounding tie); the pinned pow gives ~1e-14"""
    worst = 0.0
    for g in [g for g in contract_gammas() if g <= 21.0][::7] + [9.2, 21.0]:
        for i in range(1, 255, 3):
            want = math.pow(i / 255.0, float(np.float32(g)))
            got = em.t_pow(i / 255.0, float(np.float32(g)))
            if want > 1e-300:
                worst = max(worst, abs(got - want) / want)
    assert worst < 1e-12, worst
    # total: a result below the normal range is 0 (libm: subnormal or 0 -- both far below 0.5 / 255), never a garbage exponent
    for g in LARGE_GAMMAS:
        for i in (1, 2, 100, 200, 254):
            got, want = em.t_pow(i / 255.0, g), math.pow(i / 255.0, g)
            assert 0.0 <= got <= 1.0 and (abs(got - want) <= 1e-12 * want or (got == 0.0 and want < 2.3e-308)), (g, i, got, want)
    assert em.t_pow(0.0, 0.0) == 1.0 and em.t_pow(0.0, 0.5) == 0.0 and em.t_pow(1.0, 7.0) == 1.0 and em.t_pow(0.3, 0.0) == 1.0


def test_tables_are_non_decreasing_and_the_fixed_points(em):
    for g in contract_gammas():
        t = pinned_lut(em, g).astype(int)
        assert (np.diff(t) >= 0).all(), g
        assert t[255] == 255, g
        if g > 0:
            assert t[0] == 0, g
    assert (pinned_lut(em, 0.0) == 255).all()                       # pow(x, 0) = 1, pow(0, 0) = 1
    assert np.array_equal(pinned_lut(em, 1.0), np.arange(256))      # the identity


def test_gamma_from_sums(em):
    rng = np.random.default_rng(11)
    for gains in GAINS:
        for _ in range(4000):
            w, h = int(rng.integers(1, 4000)), int(rng.integers(1, 3000))
            n = w * h
            s = np.array([int(rng.integers(0, 256 * n)) for _ in range(3)], np.uint64)
            s = np.minimum(s, np.uint64(255 * n))
            got = np.float32(em.t_gamma(_p(s), n, *gains))
            want = R.gamma_from_sums(s, n, *gains)
            assert got.tobytes() == np.float32(want).tobytes(), (s, n, gains, got, want)
    # more pixels than 2^32 / 255: the sums pass 32 bits
    n = 5000 * 5000
    s = np.array([255 * n, 200 * n, 3 * n], np.uint64)
    assert np.float32(em.t_gamma(_p(s), n, 100.0, 50.0)).tobytes() == np.float32(R.gamma_from_sums(s, n)).tobytes()


def test_gamma_branch_edges(em):
    """g == 1 (the upper end of the mapped range: stays 1) and g == -3 (the lower end: maps to 0), reached exactly: with gains
    (100, 50) k = 0.04 and b = -1, with (4, 2) k = 1 and b = -1 -- a uniform frame of value v has meanC3 = v and g = v - 1"""
    def uniform(v, n=64):
        return np.array([v * n, v * n, v * n], np.uint64), n
    for v, want in ((2, 1.0), (1, 0.75), (0, 0.5), (3, 2.0), (255, 254.0)):
        s, n = uniform(v)
        assert R.gamma_from_sums(s, n, 4.0, 2.0) == np.float32(want)
        assert np.float32(em.t_gamma(_p(s), n, 4.0, 2.0)) == np.float32(want)
    # g = -3 exactly and just below: gains (2, 4) give k = -1, b = 5, g = 5 - v
    for v, want in ((8, 0.0), (9, 0.0), (7, 0.25), (4, 1.0), (3, 2.0)):
        s, n = uniform(v)
        assert R.gamma_from_sums(s, n, 2.0, 4.0) == np.float32(want), v
        assert np.float32(em.t_gamma(_p(s), n, 2.0, 4.0)) == np.float32(want), v


@pytest.mark.parametrize("lb", [1, 80, 255, 256])
def test_threshold_table_against_brute_force(em, lb):
    """M[b] = min{a : LUT[a] - LUT[b] >= lb}: a >= M[b] must equal the compare through the table for every (a, b)"""
    for g in contract_gammas()[::40] + [0.0, 0.5, 1.0, 2.2, 9.2] + LARGE_GAMMAS:
        t = pinned_lut(em, g)
        m = np.empty(256, np.uint16)
        em.t_m(_p(t), lb, _p(m))
        assert np.array_equal(m, R.m_table(t, lb)), (g, lb)
        a = np.arange(256)
        direct = (t.astype(int)[:, None] - t.astype(int)[None, :]) >= lb  # [a, b]
        assert np.array_equal(a[:, None] >= m[None, :].astype(int), direct), (g, lb)


def test_host_side_abi_entry_points():
    from rmcv_amd import abi
    L = abi.lib()
    for g in (0.0, 0.5713445, 1.0, 2.2, 9.2):
        assert np.array_equal(abi.gamma_lut(g), R.lut(g)), g
    out = np.zeros(256, np.uint8)
    for bad in (-0.5, float("nan"), float("inf")):
        assert L.rmcv_gamma_lut(C.c_float(bad), _p(out)) == abi.ERR_BAD_ARG
    assert L.rmcv_gamma_lut(C.c_float(1.0), None) == abi.ERR_BAD_ARG
    s = np.array([123456789, 98765432, 55555555], np.uint64)
    n = 1280 * 1024
    assert abi.enhance_gamma(s, n).tobytes() == np.float32(R.gamma_from_sums(s, n)).tobytes()
    assert abi.enhance_gamma(s, n, 30.0, 5.0).tobytes() == np.float32(R.gamma_from_sums(s, n, 30.0, 5.0)).tobytes()
    g = C.c_float(0)
    for hi, lo in ((50.0, 50.0), (float("nan"), 50.0), (100.0, float("inf"))):
        assert L.rmcv_enhance_gamma(_p(s), C.c_int64(n), C.c_float(hi), C.c_float(lo), C.byref(g)) == abi.ERR_BAD_ARG
    assert L.rmcv_enhance_gamma(_p(s), C.c_int64(0), C.c_float(100.0), C.c_float(50.0), C.byref(g)) == abi.ERR_BAD_ARG


def test_dimmed_frames_tell_the_paths_apart(oracle):
    """the inputs of the GPU tests: synthetic frames 0..7 (1280x1024, variant 0, blue) as an under-exposed camera sees them.  At
    (v * 80) >> 8 the plain path finds nothing and the enhanced one the armours; at 96 they differ on six frames; at 112 and on the
    undimmed stream they agree (the synthetic lights are saturated)."""
    from rmcv_amd import CAMP_BLUE, synth
    frames = synth.batch(0, 8, 1280, 1024, CAMP_BLUE, 0)
    p = oracle.default_params()

    def counts(img):
        r = oracle.detect_frame(img, p)
        return len(r["offs"]) - 1, len(r["blobs"]), len(r["armours"])
    plain, enh, gam = {}, {}, {}
    for num in (80, 96, 112):
        d = R.dim(frames, num)
        plain[num] = [counts(d[f]) for f in range(8)]
        e = [R.E(d[f]) for f in range(8)]
        enh[num] = [counts(x[0]) for x in e]
        gam[num] = [float(x[1]) for x in e]
    assert plain[80] == [(0, 0, 0)] * 8
    assert enh[80][:3] == [(23, 8, 4), (11, 2, 1), (13, 4, 1)]
    assert [c[2] for c in enh[80]] == [4, 1, 1, 5, 1, 2, 2, 2]
    assert all(0.56 < g < 0.58 for g in gam[80])                     # gamma ~0.57
    assert [c[2] for c in plain[96]] == [3, 0, 1, 2, 0, 0, 0, 2]
    assert [c[2] for c in enh[96]] == [4, 1, 3, 6, 1, 2, 2, 2]
    assert plain[112] == enh[112]
    full = [R.E(frames[f]) for f in range(8)]
    for f in range(8):
        assert oracle.detect_frame(full[f][0], p)["armours"].tobytes() == oracle.detect_frame(frames[f], p)["armours"].tobytes()


def test_shim_defines_the_exposure_functions(tmp_path):
    """the backend object (declarations of include/imgproc.h:23, 35 + the shim) DEFINES rm::CalcGamma, rm::AutoEnhance and the fused
    rm::extract_color_enhanced next to the functions it defined before; a caller that saw declarations only links against it"""
    here = os.path.join(ROOT, "tests")
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in ("shim_enhance/backend_enhance", "shim/core_stub", "shim_enhance/caller_enhance"):
        objs[unit] = os.path.join(str(tmp_path), os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(here, "cv_mock"), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(here, "shim"),
                        "-I", os.path.join(here, "shim_enhance"), "-c", os.path.join(here, unit + ".cpp"), "-o", objs[unit]], check=True)
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_enhance/backend_enhance"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_enhance/caller_enhance"]], check=True, capture_output=True, text=True).stdout
    for sym in ("rm::CalcGamma(", "rm::AutoEnhance(", "rm::extract_color_enhanced(", "rm::extract_color(", "rm::filter_armours("):
        assert any(sym in ln and " T " in ln for ln in defined.splitlines()), sym
        assert any(sym in ln for ln in undefined.splitlines()), sym
    assert "rmcv_auto_enhance" not in undefined  # the caller reaches the C-ABI only through rm::
    exe = os.path.join(str(tmp_path), "shim_enhance_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    assert os.path.exists(exe)
