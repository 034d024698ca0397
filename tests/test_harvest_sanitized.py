"""The host path of rmcv_amd/csrc/device_harvest.h under AddressSanitizer and UndefinedBehaviorSanitizer: tests/harvest_san_main.cpp, a
stand-alone program with its own main whose every table is a heap block of exactly its size, is compiled with -fsanitize=address,undefined
and fed the case list of tests/test_harvest_plan.py; what it writes equals tests/harvest_ref.py.  A CPU test: nothing here touches a GPU
or loads into python."""
import os
import subprocess

import harvest_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def test_host_rule_under_sanitizers_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "harvest_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "harvest_san_main.cpp"), "-o", exe], check=True)
    cs = K.calls()
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(K.encode(cs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, src, dst], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    K.check(K.decode(open(dst, "rb").read(), cs), cs)
