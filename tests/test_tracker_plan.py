"""tracker_plan.h (rmcv_amd/csrc) against the code it replaced: compiled with the host C++ compiler into a stand-alone program, what the
header's ONE view of a tracker's state gives its callers is compared, over whole grids, with the expressions as they stood in k_aim.hip,
k_attitude.hip, rmcv_host.hip and rmcv_pipeline.hip before the header, restated in tests/tracker_plan_ref.py (each function there names its
file and lines): the nullable arguments of launch_aim and launch_attitude, the LoopArgs fill, a tracked submit's origins and keys, what
rmcv_batch_track and rmcv_batch_attitude refuse and in which order, the host's offset of a stream's current list, and what a config is
refused for.  The program runs as a child process, once more built with the address and undefined-behaviour sanitizers; nothing is loaded
into Python."""
import itertools
import os
import subprocess

import pytest

import tracker_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fake device addresses (never dereferenced): what the state's pointers hold when "allocated"
P = dict(b_origins=0x1000, b_camps=0x2000, b_lower_bounds=0x3000, aim_cfgs=0x4000, stream_g2c=0x5000, aims=0x6000, aim_inputs=0x7000,
         attitudes=0x8000, packet_errors=0x9000)
# bit i of a state's mask, in this order: the six modes, then which of the six tables with a first use have had it, then win_w != 0
BITS = ("aim_on", "att_on", "camps_on", "lower_bounds_on", "aim_cfgs_on", "stream_g2c_on", "aim_cfgs", "stream_g2c", "aims", "aim_inputs",
        "attitudes", "packet_errors", "win")
TC = (3, 640, 512, 320, 256)     # the refusals' tracker: n_streams, frame_w, frame_h, win_w, win_h

SRC = r'''
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include "rmcv_amd/csrc/tracker_plan.h"
using namespace rmcv;
template <typename T> static T* at(uintptr_t a) { return reinterpret_cast<T*>(a); }
static unsigned long long u(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }
int main()
{
    for (int m = 0; m < (1 << 13); m++) {
        const auto bit = [m](int i) { return ((m >> i) & 1) != 0; };
        TrackerState s;
        s.device = 5;
        s.cfg.n_streams = 3, s.cfg.track_cap = 2, s.cfg.frame_w = 640, s.cfg.frame_h = 512, s.cfg.tick_frequency = 1e9;
        s.cfg.win_w = bit(12) ? 320 : 0, s.cfg.win_h = bit(12) ? 256 : 0;
        s.aim_cfg.max_lost = 7, s.aim_cfg.v0 = 15.5, s.att_cfg.motor_angle_mode = 1, s.att_cfg.gripper2camera[15] = 2.5;
        s.b.tracks = at<rmcv_track>(0x100), s.b.side = at<float>(0x200), s.b.sel = at<int32_t>(0x300), s.b.n_tracking = at<int32_t>(0x400), s.b.status = at<int32_t>(0x500);
        s.b.origins = at<rmcv_point>(0x1000), s.b.camps = at<int32_t>(0x2000), s.b.lower_bounds = at<int32_t>(0x3000);
        s.aim_on = bit(0), s.att_on = bit(1);
        // switched tables: mode and memory are independent bits (the two in TrackerBufs are there from the tracker's creation on)
        s.camps = {s.b.camps, bit(2)}, s.lower_bounds = {s.b.lower_bounds, bit(3)};
        s.aim_cfgs = {bit(6) ? at<rmcv_aim_config>(0x4000) : nullptr, bit(4)}, s.stream_g2c = {bit(7) ? at<double>(0x5000) : nullptr, bit(5)};
        // tables with a first use: on from their allocation on (tracker_plan.h, StreamTable)
        s.aims = {bit(8) ? at<rmcv_aim>(0x6000) : nullptr, bit(8)}, s.aim_inputs = {bit(9) ? at<rmcv_aim_input>(0x7000) : nullptr, bit(9)};
        s.attitudes = {bit(10) ? at<rmcv_attitude>(0x8000) : nullptr, bit(10)}, s.packet_errors = {bit(11) ? at<int32_t>(0x9000) : nullptr, bit(11)};
        const TrackerView v = tracker_view_of(s);
        const int copied = v.device == 5 && !memcmp(&v.cfg, &s.cfg, sizeof(s.cfg)) && !memcmp(&v.aim_cfg, &s.aim_cfg, sizeof(s.aim_cfg)) &&
                           !memcmp(&v.att_cfg, &s.att_cfg, sizeof(s.att_cfg)) && !memcmp(&v.b, &s.b, sizeof(s.b));
        printf("V %d : %d %d %d %d %d %d %llx %llx %llx %llx %llx %llx %llx %llx %llx\n", m, copied, (int)v.aim_on, (int)v.att_on, v.has_aim, v.has_att, v.has_camps, u(v.origins),
               u(v.camps), u(v.lower_bounds), u(v.aim_cfgs), u(v.stream_g2c), u(v.aims), u(v.aim_inputs), u(v.attitudes), u(v.packet_errors));
    }
    // the refusals: a tracker of 3 streams, 640 x 512, windows of 320 x 256
    TrackerView v{};
    v.cfg.n_streams = 3, v.cfg.frame_w = 640, v.cfg.frame_h = 512, v.cfg.win_w = 320, v.cfg.win_h = 256;
    const int dxy[5][2] = {{0, 0}, {1, 0}, {-1, 0}, {0, 1}, {0, -1}}, win[4][3] = {{0, 640, 512}, {1, 320, 256}, {1, 321, 256}, {1, 320, 255}};
    for (int track = 0; track < 2; track++) for (int dev : {0, 1}) for (int att = 0; att < 2; att++) for (int n : {0, 2, 3, 4}) for (int frames = 0; frames < 2; frames++)
        for (auto& d : dxy) for (int stages : {15, 7}) for (auto& w : win) {
            v.device = dev, v.att_on = att != 0;
            const StepBatch g{0, n, frames != 0, 640 + d[0], 512 + d[1], w[0], w[1], w[2]};
            char buf[200];
            const char* no = step_refusal(track ? "rmcv_batch_track" : "rmcv_batch_attitude", track != 0, v, g, stages, buf);
            printf("R %d %d %d %d %d %d %d %d %d %d %d : %s\n", track, dev, att, n, frames, d[0], d[1], stages, w[0], w[1], w[2], no ? no : "-");
        }
    for (int sel : {0, 1, 2, 3, -1}) for (int n_streams : {1, 3, 256}) for (int stream : {0, n_streams / 2, n_streams - 1}) for (int cap : {1, 2, 64})
        printf("A %d %d %d %d : %zu\n", sel, n_streams, stream, cap, current_list_at(sel, n_streams, stream, cap));
    // a config: the defaults, then one field at a time
    rmcv_tracker_config ok{};
    ok.n_streams = 3, ok.track_cap = 2, ok.process_noise = 5e-5, ok.measurement_noise = 0.5, ok.error = 0.05, ok.tick_frequency = 1e9;
    ok.roi_scale_w = ok.roi_scale_h = 1.0f, ok.frame_w = 640, ok.frame_h = 512;
    int row = 0;
    const auto cfg = [&row](const rmcv_tracker_config& c) {
        for (int with = 0; with < 2; with++) {
            const char* no = tracker_config_refusal(c, with != 0);
            printf("C %d %d : %s\n", row, with, no ? no : "-");
        }
        row++;
    };
    cfg(ok);
    for (int v_ : {0, -1}) { auto c = ok; c.n_streams = v_; cfg(c); }
    for (int v_ : {0, 1, 64, 65}) { auto c = ok; c.track_cap = v_; cfg(c); }
    for (double v_ : {(double)NAN, (double)INFINITY, 0.0, -1.0}) {
        { auto c = ok; c.process_noise = v_; cfg(c); }
        { auto c = ok; c.measurement_noise = v_; cfg(c); }
        { auto c = ok; c.error = v_; cfg(c); }
        { auto c = ok; c.tick_frequency = v_; cfg(c); }
        { auto c = ok; c.roi_scale_w = (float)v_; cfg(c); }
        { auto c = ok; c.roi_scale_h = (float)v_; cfg(c); }
    }
    for (int v_ : {0, 1, 65536, 65537}) {
        { auto c = ok; c.frame_w = v_; cfg(c); }
        { auto c = ok; c.frame_h = v_; cfg(c); }
    }
    const int wins[8][2] = {{0, 0}, {1, 1}, {640, 512}, {641, 512}, {640, 513}, {0, 1}, {1, 0}, {-1, -1}};
    for (auto& w : wins) { auto c = ok; c.win_w = w[0], c.win_h = w[1]; cfg(c); }
    return 0;
}
'''


def build_and_run(d, name, flags):
    src = d / "tracker_plan.cpp"
    src.write_text(SRC)
    out = d / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", ROOT, str(src), "-o", str(out)], check=True)
    return subprocess.run([str(out)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("tracker_plan")
    plain = build_and_run(d, "tracker_plan", [])
    rows = {}
    for ln in plain.splitlines():
        rows.setdefault(ln[0], []).append(ln[2:])
    return d, plain, rows


def state_of(m):
    """the tracker of mask m as the parent's struct rmcv_tracker held it"""
    t = {k: bool((m >> i) & 1) for i, k in enumerate(BITS)}
    for k in ("aim_cfgs", "stream_g2c", "aims", "aim_inputs", "attitudes", "packet_errors"):
        t[k] = P[k] if t[k] else 0
    t.update(b_origins=P["b_origins"], b_camps=P["b_camps"], b_lower_bounds=P["b_lower_bounds"], win_w=320 if t["win"] else 0, win_h=256 if t["win"] else 0)
    return t


def test_view_is_what_every_caller_computed(built):
    got = built[2]["V"]
    assert len(got) == 1 << len(BITS)
    seen_per_stream = set()
    for m, ln in enumerate(got):
        head, vals = ln.split(" : ")
        assert int(head) == m
        f = vals.split()
        copied, aim_on, att_on, has_aim, has_att, has_camps = (int(x) for x in f[:6])
        origins, camps, lbs, aim_cfgs, g2c, aims, inputs, attitudes, errors = (int(x, 16) for x in f[6:])
        t = state_of(m)
        assert copied == 1 and (aim_on, att_on) == (int(t["aim_on"]), int(t["att_on"]))
        # launch_aim and launch_attitude pass the view's fields where they passed these expressions
        assert (inputs, aims, aim_cfgs) == R.launch_aim_args(t), m
        r_att, r_camps, r_err, r_in, r_per_stream, r_g2c = R.launch_attitude_args(t)
        assert (attitudes, camps, errors, inputs, g2c) == (r_att, r_camps, r_err, r_in, r_g2c), m
        # the PER_STREAM build: chosen by the mode before, by the view's pointer now.  The two agree wherever the mode's table exists -- the
        # setter switches the mode on behind the allocation only; in the state it cannot reach the old rule launched the kernel on a null table
        if t["stream_g2c"] or not t["stream_g2c_on"]:
            assert (g2c != 0) == r_per_stream, m
            seen_per_stream.add(r_per_stream)
        assert (aims, inputs, aim_cfgs, attitudes, errors, g2c, has_aim, has_att, has_camps, bool(att_on)) == R.loop_args(t), m
        assert (origins, t["win_w"], t["win_h"], camps, lbs) == R.tracked_submit(t), m
    assert seen_per_stream == {False, True}


def refusal_rows():
    dxy = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
    win = ((0, 640, 512), (1, 320, 256), (1, 321, 256), (1, 320, 255))
    return itertools.product((0, 1), (0, 1), (0, 1), (0, 2, 3, 4), (0, 1), dxy, (15, 7), win)


def test_step_refusals_in_order_with_their_messages(built):
    want = []
    for track, dev, att, n, frames, d, stages, w in refusal_rows():
        if track:
            no = R.ctx_track_refusal(dev, TC, 0, n, frames, 640 + d[0], 512 + d[1], w[0], w[1], w[2], stages)
        else:
            no = R.ctx_attitude_refusal(dev, TC, att, 0, n, frames)
        want.append("%d %d %d %d %d %d %d %d %d %d %d : %s" % (track, dev, att, n, frames, d[0], d[1], stages, w[0], w[1], w[2], no or "-"))
    got = built[2]["R"]
    assert len(got) == len(want) == 2 * 2 * 2 * 4 * 2 * 5 * 2 * 4
    for g, w in zip(got, want):
        assert g == w
    # every message of both entry points is reached, and so is a pass of each
    msgs = {ln.split(" : ")[1] for ln in got}
    assert len([m for m in msgs if m.startswith("rmcv_batch_track: ")]) == 11 and len([m for m in msgs if m.startswith("rmcv_batch_attitude: ")]) == 5
    assert any(ln.startswith("1 ") and ln.endswith(": -") for ln in got) and any(ln.startswith("0 ") and ln.endswith(": -") for ln in got)


def test_current_list_offset_and_config_refusal(built):
    rows = [(tuple(int(v) for v in a.split()), int(b)) for a, b in (ln.split(":") for ln in built[2]["A"])]
    assert len(rows) == 5 * 3 * 3 * 3
    for (sel, n_streams, stream, cap), at in rows:
        assert at == R.current_list_at(sel, n_streams, stream, cap)
    nan, inf = float("nan"), float("inf")
    ok = dict(n_streams=3, track_cap=2, process_noise=5e-5, measurement_noise=0.5, error=0.05, tick_frequency=1e9, roi_scale_w=1.0, roi_scale_h=1.0,
              frame_w=640, frame_h=512, win_w=0, win_h=0)
    cases = [ok] + [dict(ok, n_streams=v) for v in (0, -1)] + [dict(ok, track_cap=v) for v in (0, 1, 64, 65)]
    for v in (nan, inf, 0.0, -1.0):
        cases += [dict(ok, **{k: v}) for k in ("process_noise", "measurement_noise", "error", "tick_frequency", "roi_scale_w", "roi_scale_h")]
    for v in (0, 1, 65536, 65537):
        cases += [dict(ok, frame_w=v), dict(ok, frame_h=v)]
    cases += [dict(ok, win_w=w, win_h=h) for w, h in ((0, 0), (1, 1), (640, 512), (641, 512), (640, 513), (0, 1), (1, 0), (-1, -1))]
    want = ["%d %d : %s" % (i, with_streams, R.check_config(c, with_streams) or "-") for i, c in enumerate(cases) for with_streams in (0, 1)]
    assert built[2]["C"] == want
    assert len({ln.split(" : ")[1] for ln in want}) == 8   # every refusal, and "-"


def test_sanitized_build_prints_the_same(built):
    d, plain, _ = built
    assert build_and_run(d, "tracker_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == plain
