"""rm::debug::logger on the shim (include/rmcv_shim.hpp): the link contract of tests/shim_record/ -- a backend unit that
DEFINES the member functions of the class the host's debug.h declares, a caller that saw the declaration only -- built like
tests/shim_view/; and what the caller's program leaves behind: a session file in the section's directory holding the frames it wrote, bit
for bit, with their `data` records, and nothing from the second, read-only logger.  Host-side only: no GPU."""
import os
import subprocess

import numpy as np

from rmcv_amd import CAMP_BLUE, synth
from rmcv_amd.recorder import Session

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS = ("shim_record/backend_record", "shim/core_stub", "shim_record/caller_record")


def build(tmp):
    libdir = os.path.join(ROOT, "rmcv_amd", "lib")
    objs = {}
    for unit in UNITS:
        objs[unit] = os.path.join(tmp, os.path.basename(unit) + ".o")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(HERE, "shim_record"), "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(HERE, "shim"), "-c", os.path.join(HERE, unit + ".cpp"), "-o", objs[unit]], check=True)
    exe = os.path.join(tmp, "shim_record_main")
    subprocess.run(["g++"] + list(objs.values()) + ["-o", exe, "-L", libdir, "-lrmcv_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                                                    "-lamdhip64"], check=True)
    return objs, exe


def test_shim_defines_the_logger_and_it_writes_a_session(tmp_path):
    objs, exe = build(str(tmp_path))
    defined = subprocess.run(["nm", "-C", "--defined-only", objs["shim_record/backend_record"]], check=True, capture_output=True, text=True).stdout
    undefined = subprocess.run(["nm", "-C", "--undefined-only", objs["shim_record/caller_record"]], check=True, capture_output=True, text=True).stdout
    for name in ("rm::debug::logger::logger(long long, int, cv::Size const&)", "rm::debug::logger::~logger()", "rm::debug::logger::write(cv::Mat const&, cv::Mat const&)"):
        assert any(name in ln and " T " in ln for ln in defined.splitlines()), name
        assert any(name in ln for ln in undefined.splitlines()), name
    assert "rmcv_pack_host" not in undefined and "rmcv_session_append" not in undefined      # the caller reaches the recorder only through rm::
    work = tmp_path / "run"
    work.mkdir()
    w, h = 200, 136
    out = subprocess.run([exe, "42", str(w), str(h)], check=True, capture_output=True, text=True, cwd=str(work), timeout=120).stdout.split()
    assert out == ["written", "3"]
    assert sorted(os.listdir(str(work / "42"))) == ["session.rmcv"]
    s = Session(str(work / "42" / "session.rmcv"))
    assert len(s) == 3                                                                        # the read-only logger's write was dropped
    a, b = synth.frame(3, w, h, CAMP_BLUE, 0), synth.frame(4, w, h, CAMP_BLUE, 0)
    blob = np.array([1.5, -2.0, 1e9]).tobytes()
    for i, (want, user, fmt, lag) in enumerate(((a, blob, 0, 3), (b, b"", 0, 3), (a[..., 1], blob, -1, 1))):
        e, got_user = s.entry(i)
        assert (e.ticket, e.n_frames, e.w, e.h, e.lag, e.input_format) == (i, 1, w, h, lag, fmt) and got_user == user
        assert np.array_equal(s.frames(i)[0].reshape(want.shape), want)
    s.close()
