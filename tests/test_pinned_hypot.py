"""pm_hypot (rmcv_amd/csrc/pinned_math.h: what the device tracker's Jacobi rotation calls, on the GPU and in rmcv_tracker_step_host) and
trk_ref_hypot (tests/track_ref_hypot.c: what the tests' reference calls instead of libm's) are both CORRECTLY ROUNDED: proven here
against exact integer arithmetic -- r is the double nearest to sqrt(a^2 + b^2) iff (r - half ulp below)^2 <= a^2 + b^2 <= (r + half ulp
above)^2 in integers, a tie only with an even r."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "rmcv_amd/csrc/pinned_math.h"
void t_hypot(const double* x, const double* y, double* o, int n) { for (int i = 0; i < n; i++) o[i] = pm_hypot(x[i], y[i]); }
'''


@pytest.fixture(scope="module")
def pm(tmp_path_factory):
    d = tmp_path_factory.mktemp("pmh")
    c = d / "pmh.c"
    c.write_text(SRC)
    so = d / "pmh.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", ROOT, str(c), "-o", str(so), "-lm"], check=True)
    return C.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def both(pm, x, y):
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    o = np.empty_like(x)
    pm.t_hypot(_p(x), _p(y), _p(o), len(x))
    return (("pm_hypot", o), ("trk_ref_hypot", track_ref.hypot_n(x, y)))


def split(v):
    """|v| = m * 2^e exactly, m an integer below 2^53, e >= -1074"""
    m, e = math.frexp(abs(v))
    e = max(e - 53, -1074)
    mi = int(math.ldexp(abs(v), -e))
    assert math.ldexp(mi, e) == abs(v)
    return mi, e


def correctly_rounded(a, b, r):
    if not math.isfinite(r) or r <= 0:
        return False
    (ma, ea), (mb, eb), (mr, er) = split(a), split(b), split(r)
    E = min(ea, eb, er)
    S16 = 16 * ((ma << (ea - E)) ** 2 + (mb << (eb - E)) ** 2)
    X = 4 * (mr << (er - E))
    ulp = 1 << (er - E)
    up = 2 * ulp                                                   # 4 x half an ulp
    dn = ulp if (mr == 1 << 52 and er > -1074) else 2 * ulp        # the spacing below a power of two is half as wide
    lo, hi = (X - dn) ** 2, (X + up) ** 2
    if mr & 1:
        return lo < S16 < hi
    return lo <= S16 <= hi


def check(pm, x, y):
    for name, o in both(pm, x, y):
        bad = [(float(a), float(b), float(r)) for a, b, r in zip(x, y, o) if not correctly_rounded(float(a), float(b), float(r))]
        assert not bad, (name, len(bad), [(a.hex(), b.hex(), r.hex()) for a, b, r in bad[:5]])


# ---- the generators (tests/leaf_cases.py imports them for the device-against-host bit tests, with smaller counts) ----------------------------
def gen_random_pairs(n=1_000_000):
    """seeded pairs, exponent differences 0 .. 60, signs mixed"""
    rng = np.random.default_rng(20240517)
    ea = rng.integers(-20, 21, n)
    d = rng.integers(0, 61, n)
    x = np.ldexp(rng.uniform(1, 2, n), ea) * rng.choice([-1.0, 1.0], n)
    y = np.ldexp(rng.uniform(1, 2, n), ea - d) * rng.choice([-1.0, 1.0], n)
    swap = rng.random(n) < 0.5
    return np.where(swap, y, x), np.where(swap, x, y)


def gen_midpoints_and_ties(n_mid=40000, n_ties=3000):
    """the hard cases: b^2 / (2 a) next to an odd number of half ulps of a (sqrt lands ~2^-53 of an ulp from a rounding boundary), and
    Pythagorean triples whose hypotenuse needs 54 bits (an exact tie: the even neighbour) -> ((x, y) near midpoints, (x, y) ties)"""
    rng = np.random.default_rng(7)
    a = np.ldexp(rng.uniform(1, 2, n_mid), rng.integers(-8, 9, n_mid))
    k = 2 * rng.integers(0, 6, n_mid) + 1
    ulp = np.ldexp(1.0, np.frexp(a)[1] - 53)
    b = np.sqrt(k * a * ulp)
    x = np.concatenate([a, a, a])
    y = np.concatenate([b, np.nextafter(b, 0), np.nextafter(b, np.inf)])
    xs, ys, n_tie = [], [], 0
    while n_tie < n_ties:
        m, n = int(rng.integers(1 << 26, 3 << 25)), int(rng.integers(1, 1 << 26))
        if (m - n) % 2 == 0 or n >= m:
            continue
        h, p, q = m * m + n * n, m * m - n * n, 2 * m * n
        if not (1 << 53) <= h < (1 << 54) or p >= (1 << 53):
            continue
        sc = int(rng.integers(-30, 30))
        xs.append(math.ldexp(p, sc))
        ys.append(math.ldexp(q, sc))
        n_tie += 1
    return (x, y), (np.array(xs), np.array(ys))


TINY, BIG = 5e-324, 1.7976931348623157e308
ZEROS = (np.array([0.0, -0.0, 3.5, -3.5, 0.0, TINY, BIG]), np.array([2.5, -2.5, 0.0, -0.0, -0.0, 0.0, 0.0]))
NON_FINITE = (np.array([math.inf, -math.inf, math.nan, math.nan, 1.0, BIG, BIG]), np.array([1.0, math.nan, math.inf, 1.0, math.nan, BIG, 1e300]))


def gen_extremes(n=20000):
    """finite, non-zero pairs at the ends of the range: a list of (x, y)"""
    rng = np.random.default_rng(3)
    sub = np.ldexp(rng.integers(1, 1 << 52, n).astype(np.float64), -1074)      # subnormals
    sub2 = np.ldexp(rng.integers(1, 1 << 52, n).astype(np.float64), -1074 - rng.integers(0, 30, n)).astype(np.float64)
    near = np.ldexp(rng.uniform(1, 2, n), rng.integers(-1030, -1000, n))  # around the smallest normal
    huge = np.ldexp(rng.uniform(1, 1.41, n), 1022)                            # near overflow (stays finite: below 2^1023.5 each)
    huge2 = np.ldexp(rng.uniform(1, 2, n), 1022 - rng.integers(0, 40, n))
    eq = np.ldexp(rng.uniform(1, 2, n), rng.integers(-1000, 1000, n))
    ok = sub2 > 0
    return [(sub[ok], sub2[ok]), (near, sub), (huge * 0.7, huge2 * 0.7), (eq, eq),
            (np.array([TINY, TINY, 3 * TINY, 2.2250738585072014e-308, 1.0, 1e300]), np.array([TINY, 2 * TINY, 4 * TINY, 2.2250738585072014e-308, 1.0, 1e300]))]


def gen_tracker_pairs():
    """the (p, beta) arguments the Jacobi rotation met in the scenarios of tests/test_tracker_cpu.py (recorded once from the reference,
    tests/golden/track_hypot_pairs.json, doubles as hex): (n, 2)"""
    with open(os.path.join(ROOT, "tests", "golden", "track_hypot_pairs.json")) as f:
        return np.array([[float.fromhex(a), float.fromhex(b)] for a, b in json.load(f)["pairs"]])


def test_random_pairs(pm):
    """10^6 seeded pairs, exponent differences 0 .. 60, signs mixed"""
    x, y = gen_random_pairs(1_000_000)
    assert len(x) == 1_000_000
    check(pm, x, y)


def test_near_midpoints_and_ties(pm):
    (x, y), (xs, ys) = gen_midpoints_and_ties(40000, 3000)
    assert len(x) == 120000 and len(xs) == 3000
    check(pm, x, y)
    check(pm, xs, ys)


def test_extremes(pm):
    tiny, big = TINY, BIG
    groups = gen_extremes(20000)
    assert len(groups) == 5 and all(len(x) >= 6 for x, _ in groups)
    for x, y in groups:
        check(pm, x, y)
    z, w = ZEROS
    for name, o in both(pm, z, w):
        assert o.tolist() == [2.5, 2.5, 3.5, 3.5, 0.0, tiny, big] and not np.signbit(o).any(), name
    inf = math.inf
    for name, o in both(pm, *NON_FINITE):
        assert o[0] == inf and o[1] == inf and o[2] == inf and math.isnan(o[3]) and math.isnan(o[4]) and o[5] == inf, name   # C99 F.9.4.3
        assert o[6] == big, name


def test_pairs_from_the_tracker_scenarios(pm):
    pairs = gen_tracker_pairs()
    assert len(pairs) >= 1000
    fin = np.isfinite(pairs).all(1) & (pairs != 0).any(1)
    check(pm, pairs[fin, 0], pairs[fin, 1])
    for name, o in both(pm, pairs[~fin, 0], pairs[~fin, 1]):   # NaN states (dt = 0) run through
        ref = np.hypot(pairs[~fin, 0], pairs[~fin, 1])
        assert np.array_equal(np.isnan(o), np.isnan(ref)) and np.array_equal(o[~np.isnan(o)], ref[~np.isnan(ref)]), name
