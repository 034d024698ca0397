"""The host side of the session recorder under AddressSanitizer and UndefinedBehaviorSanitizer: tests/record_san_main.cpp, a stand-alone
program with its own main, is compiled with -fsanitize=address,undefined.  It packs and unpacks the whole case list of tests/pack_ref.py
(what it writes equals the numpy restatement byte for byte), then feeds rmcv_unpack_host's check and the session reader every prefix length
of one tiny packed frame and one tiny session file, and the same with single bytes of header, row table, length word and entry altered:
every call returns clean or RMCV_ERR_BAD_ARG and the sanitizers stay silent.  A CPU test: nothing here touches a GPU or loads into python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pack_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
TINY = ("poisson", 300, 3, 2)        # the frame whose prefixes and altered bytes are tried: two segments a row, both modes


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_san") / "record_san_main")
    subprocess.run(["g++"] + FLAGS + [os.path.join(HERE, "record_san_main.cpp"), "-o", exe], check=True)
    return exe


def test_host_pack_unpack_and_session_reader_under_sanitizers(program, tmp_path):
    cases = R.cases() + [TINY]
    blob, want = struct.pack("<i", len(cases)), b""
    for kind, w, h, lag in cases:
        stride = w + 7                                                   # stride > w_bytes
        rows = np.full((h, stride), 0xEE, np.uint8)
        rows[:, :w] = R.plane(kind, w, h)
        blob += struct.pack("<4i", w, h, stride, lag) + rows.tobytes()
        p = R.packed(kind, w, h, lag)
        want += struct.pack("<q", len(p)) + p.tobytes()
    fin, fout, fses = (str(tmp_path / n) for n in ("in.bin", "out.bin", "session.rmcv"))
    with open(fin, "wb") as f:
        f.write(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([program, fin, fout, fses], capture_output=True, text=True, env=env)
    assert done.returncode == 0, done.stderr
    assert open(fout, "rb").read() == want
    words = done.stdout.split()
    got = dict(zip(words[0::2], (int(v) for v in words[1::2])))
    assert got["frame_prefixes_ok"] == 1                                 # the whole frame and nothing shorter
    assert got["session_prefixes_ok"] == 3                               # the header alone, one record, both records
    # an altered header or row-table byte never passes: a width changes the sizes the table and the length must add up to, a mode bit that
    # is cleared or set leaves them alone -- those (and only those) decode, to other bytes
    p = R.packed(*TINY)
    S, h = R.segments(TINY[1]), TINY[2]
    flips = sum(1 for hb in p[:h * S] if not (hb & 0x10 == 0 and (hb & 15) == 8))   # (raw b = 8 -> predicted b = 8 is no header a packer writes)
    assert got["frame_altered_ok"] == flips
