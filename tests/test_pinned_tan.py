"""pm_tan (pinned_math.h: rm::DeltaHeight's tangent, the same source on host and device) against the host libm's tan.  Both promise an
error below 1 ulp, so they can differ by 1 ulp at the most -- the bar tests/test_pinned_math.py sets for sin and cos."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include "rmcv_amd/csrc/pinned_math.h"
void t_tan(const double* x, double* o, int n) { for (int i = 0; i < n; i++) o[i] = pm_tan(x[i]); }
'''


@pytest.fixture(scope="module")
def pm(tmp_path_factory):
    d = tmp_path_factory.mktemp("pmtan")
    c = d / "pm.c"
    c.write_text(SRC)
    so = d / "pm.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", ROOT, str(c), "-o", str(so), "-lm"], check=True)
    return C.CDLL(str(so))


def _tan(pm, x):
    x = np.ascontiguousarray(x, np.float64)
    o = np.empty_like(x)
    pm.t_tan(x.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), len(x))
    return o


def ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_tan_within_one_ulp_of_the_host(pm):
    rng = np.random.default_rng(11)
    near = []
    for k in list(range(1, 9)) + list(range(-8, 0)):   # the doubles next to k pi / 2: the reduction's cancellation at its worst
        c = k * (math.pi / 2)
        near += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    x = np.concatenate([rng.uniform(-7, 7, 400000), rng.uniform(-1e4, 1e4, 200000), [2.0 ** -30, -2.0 ** -30], near])
    o = _tan(pm, x)
    r = np.array([math.tan(v) for v in x])
    d = ulps(o, r)
    worst = int(d.argmax())
    print("pm_tan vs host tan: max %d ulp (at x = %r), %d of %d differ by one" % (d.max(), x[worst], np.count_nonzero(d == 1), len(x)))
    assert np.array_equal(np.signbit(o), np.signbit(r))
    assert d.max() <= 1


def test_tan_special_values(pm):
    o = _tan(pm, [np.nan, np.inf, -np.inf, 0.0, -0.0])
    assert np.isnan(o[:3]).all()
    assert o[3] == 0.0 and not np.signbit(o[3])
    assert o[4] == 0.0 and np.signbit(o[4])
