"""The host path of rmcv_amd/csrc/model_plan.h under AddressSanitizer and UndefinedBehaviorSanitizer: tests/models_san_main.cpp, a
stand-alone program with its own main whose every model array and table is a heap block of exactly its size (1 model of 2 classes and
64 models of 8 among them), is compiled with -fsanitize=address,undefined and fed the cases of tests/model_cases.py; what it prints and
writes equals tests/model_ref.py.  A CPU test: nothing here touches a GPU or loads into python."""
import hashlib
import os
import subprocess

import model_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_pack_rule_and_refusals_under_sanitizers_equal_the_restatement(tmp_path):
    exe = str(tmp_path / "models_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "models_san_main.cpp"), "-o", exe], check=True)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(K.encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    want_lines, want_blob = K.expected()
    assert done.stdout.splitlines() == want_lines
    assert hashlib.sha256(open(dst, "rb").read()).hexdigest() == hashlib.sha256(want_blob).hexdigest()
