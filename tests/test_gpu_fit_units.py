"""The scalar tails of the ellipse fit on the device, each alone, against the oracle bit for bit: tests/fit_units/fit_units_main.hip runs
the 3 x 3 eigen-solver (device_eig3.h as the library compiles it), direct_reduce + direct_finish, normal_factor<5> / <3> + normal_apply,
general_centre and general_finish of rmcv_amd/csrc/device_fit.h over the case lists of tests/fit_unit_cases.py -- one wavefront per case,
because the tails keep their matrices across the lanes of a register -- and every result slot must equal the oracle's (two NaNs are equal;
everything else is raw bits, the sign of zero included).  tests/test_fit_units_cpu.py shows that these lists take every branch of the
tails, so a wrong constant subscript in one of the hand-unrolled shapes of device_eig3.h fails here.

A second binary of the same source, built with -DRMCV_EIG3_GENERAL, runs the run-time-subscript form of the eigen-solver that
device_eig3.h claims to equal: it must agree with the specialised build on every case of every function.

The programs are built with the library's Makefile (target fit_units: the library's own flags) and each is run ONCE, as a fresh child
process under a time limit; any non-zero status fails the module and nothing further is started on the GPU.  A missing hipcc is a failure,
not a skip: the library was built with it on this machine."""
import os
import subprocess

import numpy as np
import pytest

import fit_unit_cases as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_fit_units")
    subprocess.run(["make", "-C", os.path.join(ROOT, "rmcv_amd", "csrc"), "-j", "2", "fit_units"], check=True)
    recs = U.records()
    cases = str(d / "cases.bin")
    U.write_case_file(cases, recs)
    out = {}
    for build in ("fit_units_main", "fit_units_main_general"):
        dst = str(d / (build + ".bin"))
        done = subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "tests", "_build", build), cases, dst], capture_output=True, text=True)
        assert done.returncode == 0, (build, done.returncode, done.stderr[-2000:])   # (the second program is not started after a failure)
        out[build] = U.read_result_file(dst, recs)
    return out, [U.oracle_bits(r) for r in recs]


def _report(rec, got, want, what):
    eq = U.same_bits(got, want, U.slot_kinds(rec.fid))
    bad = np.argwhere(~eq)
    return ["%s %s[%s] slot %d: %#018x != %#018x" % (what, U.FUNCS[rec.fid], rec.names[i], j, int(got[i, j]), int(want[i, j])) for i, j in bad[:8]], len(bad)


@pytest.mark.parametrize("fid", range(len(U.FUNCS)), ids=list(U.FUNCS))
def test_device_bits_equal_the_oracle_bits(results, fid):
    device, oracle = results
    rec = U.records()[fid]
    assert rec.fid == fid and len(rec.names) > 0
    lines, n = _report(rec, device["fit_units_main"][fid], oracle[fid], "gfx950 / oracle")
    assert n == 0, (n, lines)


@pytest.mark.parametrize("fid", range(len(U.FUNCS)), ids=list(U.FUNCS))
def test_general_eigen_solver_build_equals_the_specialised_one(results, fid):
    device, oracle = results
    rec = U.records()[fid]
    lines, n = _report(rec, device["fit_units_main_general"][fid], device["fit_units_main"][fid], "RMCV_EIG3_GENERAL / specialised")
    assert n == 0, (n, lines)
    lines, n = _report(rec, device["fit_units_main_general"][fid], oracle[fid], "RMCV_EIG3_GENERAL / oracle")
    assert n == 0, (n, lines)
