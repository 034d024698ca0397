"""The host path of the icon classifier's trainer (rmcv_amd/csrc/svm_plan.h over device_svm.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/svm_san_main.cpp, a stand-alone program with its own main, is compiled with g++
-fsanitize=address,undefined and fed the case list, and what it writes equals the restatement (tests/svm_train_ref.py) byte for byte.
A CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import svm_cases as K
import svm_train_ref as R
from rmcv_amd import svm

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("svm_san") / "svm_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "svm_san_main.cpp"), "-o", exe], check=True)
    return exe


def expected_bytes(case):
    ref = K.reference(case)
    n_c = len(case["params"]["c_grid"])
    held = np.array(ref["labels"], np.int32)[R.predict(ref["W"], ref["rho"], len(ref["labels"]), case["samples"])]
    return (struct.pack("<ii", 0, len(ref["labels"])) + np.array(ref["labels"], "<i4").tobytes() + ref["W"].astype("<f4").tobytes() + ref["rho"].astype("<f8").tobytes() +
            struct.pack("<id", ref["best_index"], ref["best_c"]) + np.array(ref["cv_errors"][:n_c], "<i4").tobytes() + np.array(ref["iterations"], "<i4").tobytes() +
            np.array(ref["converged"], "<i4").tobytes() + np.array(ref["objective"], "<f8").tobytes() + ref["alpha"].astype("<f8").tobytes() + held.astype("<i4").tobytes())


@pytest.mark.parametrize("name", K.NAMES)
def test_host_path_under_sanitizers_equals_the_restatement(program, tmp_path, name):
    case = K.by_name(name)
    K.check(case)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<ii", len(case["samples"]), 0 if case["perm"] is None else 1) + bytes(svm.default_train_params(**case["params"])) +
                case["samples"].tobytes() + case["responses"].tobytes() + (b"" if case["perm"] is None else case["perm"].tobytes()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert open(dst, "rb").read() == expected_bytes(case)
