"""The host side of the recorder's loop records under AddressSanitizer and UndefinedBehaviorSanitizer: tests/loop_san_main.cpp, a stand-alone
program with its own main, is compiled with -fsanitize=address,undefined.  It writes a session of two records WITH loop records and feeds
the session reader every prefix length of it and single altered bytes of the length word, the entry (loop_bytes included) and the fixed
part of each loop record, walking whatever parses; then the trigger rule and the setup extractors meet records with hostile counts.  Every
call returns clean or RMCV_ERR_BAD_ARG and the sanitizers stay silent.  A CPU test: nothing here touches a GPU or loads into python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loop_san") / "loop_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "loop_san_main.cpp"), "-o", exe], check=True)
    return exe


def test_session_reader_and_loop_record_readers_under_sanitizers(program, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, str(tmp_path / "session.rmcv")], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    words = done.stdout.split()
    got = dict(zip(words[0::2], (int(v) for v in words[1::2])))
    assert got["prefixes_ok"] == 3                 # the header alone, one record, both records
    assert got["hostile_refused"] == 12            # four hostile counts x three extractors
    assert got["altered_ok"] > 0                   # most bytes of a fixed part are free to differ; the counts are not
