"""The sentence every parity assertion of this suite rests on -- the same source gives the same bits on the host and on gfx950
(rmcv_amd/csrc/pinned_math.h) -- checked directly: tests/leaf/leaf_main.hip evaluates every leaf function of pinned_math.h and enhance_math.h,
and the IEEE primitives they take for granted, over the case list of tests/leaf_cases.py in a trivial kernel and in its own (clang) host
pass, and both must equal the gcc build of the same text bit for bit (two NaNs are equal; everything else is raw bits, the sign of zero
included).  The program is built with the library's Makefile (its `leaf` target: the library's own flags) and run ONCE, as a fresh child
process; any non-zero status fails the module and nothing further is started on the GPU.  A missing hipcc is a failure, not a skip: the
library was built with it on this machine."""
import os
import subprocess

import pytest

import leaf_cases as K
from test_leaf_cpu import ROOT, build_gcc_program, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_leaf")
    subprocess.run(["make", "-C", os.path.join(ROOT, "rmcv_amd", "csrc"), "-j", "1", "leaf"], check=True)
    recs = K.records()
    cases, dst, gcc_dst = str(d / "cases.bin"), str(d / "device.bin"), str(d / "gcc.bin")
    K.write_case_file(cases, recs)
    subprocess.run([build_gcc_program(d), cases, gcc_dst], check=True)
    done = subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "tests", "_build", "leaf_main"), cases, dst], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    device_and_clang = K.read_result_file(dst, recs)
    assert all(dev is not None for dev, _ in device_and_clang)
    return device_and_clang, [host for _, host in K.read_result_file(gcc_dst, recs)]


@pytest.mark.parametrize("func", K.functions())
def test_device_bits_equal_the_host_bits(results, func):
    device_and_clang, gcc = results
    failures = []
    for k, r in enumerate(K.records()):
        if r.func == func:
            dev, clang = device_and_clang[k]
            failures += [report(r, dev, gcc[k], "gfx950 / gcc host"), report(r, clang, gcc[k], "clang host / gcc host"), report(r, dev, clang, "gfx950 / clang host")]
    assert not any(failures), [f for f in failures if f]
