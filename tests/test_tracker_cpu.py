"""rmcv_tracker_step_host -- the device tracker's step for one stream, run on the CPU from the source the kernel is compiled from
(rmcv_amd/csrc/device_track.h) -- against the CPU oracle's tracker with only hypot replaced (tests/track_ref.py), byte for byte: whole
rmcv_track arrays, counts, status, side records and origins.  Expected origins come from rmcv_get_roi / rmcv_window_origin applied to
the oracle's view of the target.  Against the UNMODIFIED oracle (libm's hypot) everything discrete is equal; the largest relative
difference of a finite filter field is printed (DESIGN.md 4e quotes it), not asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import track_ref as R
import track_scenarios as S
from rmcv_amd import abi
from rmcv_amd.tracker import TRACKER_OVF, Tracker, default_tracker_config

FRAME = (1280, 1024)
FILTER_FIELDS = ("measurement", "state_pre", "state_post", "transition", "measurement_matrix", "process_noise_cov", "measurement_noise_cov",
                 "error_cov_pre", "error_cov_post", "gain")
DISCRETE_FIELDS = ("armour", "timestamp", "lost_count", "identity", "position", "initialized", "n_ids", "ids", "counts")


def eff_origin(req, cfg):
    """the library's clamp and snap (window_origin_eff); (0, 0) without windows"""
    if cfg.win_w == 0:
        return 0, 0
    x = min(max(req[0], 0), cfg.frame_w - cfg.win_w) & ~15
    y = min(max(req[1], 0), cfg.frame_h - cfg.win_h)
    return x, y


def to_window(armours, ex, ey):
    a = armours.copy()
    for f in ("icon", "vertices"):
        a[f] -= np.array([ex, ey], np.float32)
    a["bbox"][:, 0] -= np.float32(ex)
    a["bbox"][:, 1] -= np.float32(ey)
    assert abi.armours_to_frame(a, ex, ey).tobytes() == armours.tobytes()   # (integer-valued boxes: exact)
    return a


def run(name, ref_lib, compare_bytes=True):
    over, steps = S.scenarios()[name]
    cfg = default_tracker_config(frame_w=FRAME[0], frame_h=FRAME[1], **over)
    ref = R.RefStream(ref_lib, cap=cfg.track_cap, tick=cfg.tick_frequency, noise=(cfg.process_noise, cfg.measurement_noise, cfg.error), roi_scale=(cfg.roi_scale_w, cfg.roi_scale_h), frame=FRAME,
                      win=(cfg.win_w, cfg.win_h), origin=(37, -5))
    tr, side, st, org = np.zeros(0, abi.TRACK), np.zeros((0, 4, 2), np.float32), 0, (37, -5)
    worst = 0.0
    assert len(steps) >= 60
    for k, (arm, ids, pos, ts) in enumerate(steps):
        ex, ey = eff_origin(ref.origin, cfg)              # closed loop: this frame was read through the window the last step asked for
        tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, to_window(arm, ex, ey), ids, pos, (ex, ey), ts)
        assert ref.step(arm, ids, pos, ts), (name, k)
        assert len(tr) == len(ref.tracks) and st == ref.status == 0 and org == ref.origin, (name, k, len(tr), len(ref.tracks), org, ref.origin)
        assert side.tobytes() == ref.side.tobytes(), (name, k)
        if compare_bytes:
            assert tr.tobytes() == ref.tracks.tobytes(), (name, k)
        else:
            for f in DISCRETE_FIELDS:
                assert tr[f].tobytes() == ref.tracks[f].tobytes(), (name, k, f)
            for f in FILTER_FIELDS:
                a, b = tr[f].ravel(), ref.tracks[f].ravel()
                assert np.array_equal(np.isfinite(a), np.isfinite(b)), (name, k, f)
                m = np.isfinite(a) & (a != b)
                if m.any():
                    worst = max(worst, float(np.max(np.abs(a[m] - b[m]) / np.maximum(np.abs(a[m]), np.abs(b[m])))))
    # the condition on every parity scenario, from the ORACLE's own run: never beyond track_cap or 32 identities
    assert 0 < ref.max_tracks <= cfg.track_cap and ref.max_ids <= abi.TRACK_IDS, (name, ref.max_tracks, ref.max_ids)
    return tr, ref, worst


@pytest.mark.parametrize("name", sorted(S.scenarios()))
def test_step_host_equals_the_hypot_pinned_oracle_byte_for_byte(name):
    tr, ref, _ = run(name, R.lib())
    if name == "drift":       # tracks were spawned, coasted and erased (with the erase-skip) along the way
        assert ref.max_tracks >= 4 and len(tr) < 110 // 7
    if name == "crossing":
        assert ref.max_tracks >= 2
    if name == "identities":
        assert ref.max_ids >= 10
    if name == "equal_stamps":
        assert not np.isfinite(tr["state_post"]).all()    # dt = 0 on a matched update: NaN, compared as bytes above
    if name == "bare":
        assert (tr["identity"] == -1).all() and not tr["position"].any()


def test_drift_erases_on_the_27th_miss_and_skips_the_neighbour():
    """the drift scenario step by step on the reference: the step that erases target 0 leaves the target behind it un-aged"""
    over, steps = S.scenarios()["drift"]
    cfg = default_tracker_config(frame_w=FRAME[0], frame_h=FRAME[1], **over)
    tr, side, st, org = np.zeros(0, abi.TRACK), np.zeros((0, 4, 2), np.float32), 0, (0, 0)
    seen = False
    for arm, ids, pos, ts in steps:
        before = tr.copy()
        tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, arm, ids, pos, (0, 0), ts)
        if len(before) and int(before[0]["lost_count"]) == 26 and len(before) >= 2:
            assert tr[0].tobytes() == before[1].tobytes()   # moved into slot 0, skipped: not matched, not aged
            seen = True
    assert seen


def test_against_the_unmodified_oracle_everything_discrete_is_equal(capsys):
    worst = {}
    for name in sorted(S.scenarios()):
        worst[name] = run(name, O.lib(), compare_bytes=False)[2]
    with capsys.disabled():
        print("\n[tracker] largest relative difference of a finite filter field, pm_hypot against libm's hypot: %.3e (%s)"
              % (max(worst.values()), ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))


def test_overflow_is_refused_whole_and_the_flag_sticks():
    cfg = default_tracker_config(track_cap=4, frame_w=FRAME[0], frame_h=FRAME[1], win_w=512, win_h=384)
    mk = lambda xs: np.array([S.armour(x, 300) for x in xs], abi.ARMOUR)
    tr, side, st, org = Tracker.step_host(cfg, [], [], 0, (5, 6), mk([100, 300, 500]), [1, 2, 3], None, (0, 0), 10)
    assert len(tr) == 3 and st == 0
    before = (tr.tobytes(), side.tobytes(), org)
    # 3 targets matched by nobody + 2 far armours: 5 > 4 -> the whole step is refused
    tr2, side2, st2, org2 = Tracker.step_host(cfg, tr, side, st, org, mk([800, 1000]), [1, 1], None, (0, 0), 20)
    assert st2 == TRACKER_OVF and (tr2.tobytes(), side2.tobytes(), org2) == before
    # a step that fits is applied, the flag stays
    tr3, side3, st3, org3 = Tracker.step_host(cfg, tr2, side2, st2, org2, mk([102, 800]), [1, 1], None, (0, 0), 30)
    assert st3 == TRACKER_OVF and len(tr3) == 4 and int(tr3[0]["timestamp"]) == 30 and [int(v) for v in tr3["lost_count"]] == [0, 1, 1, 0]
    ref = R.RefStream(R.lib(), cap=4, frame=FRAME, win=(512, 384), origin=(5, 6))
    assert ref.step(mk([100, 300, 500]), [1, 2, 3], None, 10) and not ref.step(mk([800, 1000]), [1, 1], None, 20) and ref.step(mk([102, 800]), [1, 1], None, 30)
    assert tr3.tobytes() == ref.tracks.tobytes() and side3.tobytes() == ref.side.tobytes() and org3 == ref.origin and ref.status == TRACKER_OVF


def test_the_33rd_identity_is_refused():
    cfg = default_tracker_config(frame_w=FRAME[0], frame_h=FRAME[1])
    a = np.array([S.armour(400, 400)], abi.ARMOUR)
    tr, side, st, org = np.zeros(0, abi.TRACK), np.zeros((0, 4, 2), np.float32), 0, (0, 0)
    for k in range(33):      # the first step creates the target; 32 matched updates fill the histogram
        tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, a, [k], None, (0, 0), (k + 1) * 1000)
    assert st == 0 and int(tr[0]["n_ids"]) == 32
    before = tr.tobytes()
    tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, a, [99], None, (0, 0), 50_000)
    assert st == TRACKER_OVF and tr.tobytes() == before
    tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, a, [7], None, (0, 0), 60_000)   # a known identity still fits
    assert int(tr[0]["timestamp"]) == 60_000 and st == TRACKER_OVF


def test_get_roi_and_window_origin_kept_their_arithmetic():
    """their bodies moved into device_track.h: the exports against a restatement in Python, the width-for-height line included"""
    import math
    rng = np.random.default_rng(8)
    for _ in range(300):
        pts = rng.uniform(-50, 1400, (4, 2)).astype(np.float32)
        sw, sh = (1.0, 1.0) if rng.random() < 0.3 else (float(np.float32(rng.uniform(0.5, 3))), float(np.float32(rng.uniform(0.5, 3))))
        x, y = math.floor(pts[:, 0].min()), math.floor(pts[:, 1].min())
        w, h = math.floor(pts[:, 0].max()) - x + 1, math.floor(pts[:, 1].max()) - y + 1
        if sw != 1.0 or sh != 1.0:
            mw, mh = int(w * sw / 2.0), int(h * sh / 2.0)
            x, y, w, h = x - mw, y - mh, w + 2 * mw, h + 2 * mw
        x, y = max(x, 0), max(y, 0)
        if x + w >= 1280:
            w = 1280 - x - 1
        if y + h >= 1024:
            h = 1024 - y - 1
        exp = (0, 0, 0, 0) if w < 0 or h < 0 else (x, y, w, h)
        got = abi.get_roi(pts, (sw, sh), (1280, 1024))
        assert got == exp
        ox, oy = abi.window_origin(got, 512, 384)
        assert (ox, oy) == (got[0] + int(got[2] / 2) - 256, got[1] + int(got[3] / 2) - 192)


REVERSED_SRC = r"""
#define TRK_HOST_REVERSED 1
#include <string.h>
#include <vector>
#include "rmcv_amd/csrc/device_track.h"
extern "C" int step_reversed(const trk_cfg* k, rmcv_track* tracks, float* side, int32_t* n, int32_t* status, rmcv_point* origin, const rmcv_armour* armours,
                             int n_obs, const int32_t* ids, const double* pos, int x_eff, int y_eff, int64_t ts)
{
    trk_obs ob;
    ob.armours = armours; ob.identity = ids; ob.pos = pos; ob.pos_stride = 3; ob.n = n_obs; ob.fx = (float)x_eff; ob.fy = (float)y_eff; ob.timestamp = ts;
    std::vector<trk_plan_t> pl(1);
    trk_plan(&pl[0], tracks, *n, &ob, k);
    if (pl[0].ovf) { *status |= 1; return 0; }
    if (pl[0].apply) {
        const int n_out = pl[0].n_src + pl[0].n_new;
        std::vector<rmcv_track> nxt((size_t)n_out);
        std::vector<float> snx((size_t)n_out * 8);
        std::vector<trk_ws> ws(1);
        for (int j = n_out - 1; j >= 0; j--) trk_apply_slot(&ws[0], &pl[0], j, tracks, side, nxt.data(), snx.data(), &ob, k, 0);   /* slots in any order too */
        memcpy(tracks, nxt.data(), (size_t)n_out * sizeof(rmcv_track));
        memcpy(side, snx.data(), (size_t)n_out * 8 * sizeof(float));
        *n = n_out;
    }
    trk_next_window(tracks, side, *n, k, origin);
    return 0;
}
"""


class StepCfg(C.Structure):
    """trk_cfg of device_track.h"""
    _fields_ = [("track_cap", C.c_int32), ("frame_w", C.c_int32), ("frame_h", C.c_int32), ("win_w", C.c_int32), ("win_h", C.c_int32),
                ("roi_scale_w", C.c_float), ("roi_scale_h", C.c_float), ("process_noise", C.c_double), ("measurement_noise", C.c_double),
                ("error", C.c_double), ("tick_frequency", C.c_double)]


def test_no_phase_depends_on_the_order_of_its_elements(tmp_path):
    """on the device the elements of a TRK_EACH phase are lanes running at once, and the slots of a step are wavefronts: the shared source
    built with every phase's elements (and the slots) in the OPPOSITE order must give the same bytes"""
    import subprocess
    src = tmp_path / "rev.cpp"
    src.write_text(REVERSED_SRC)
    so = tmp_path / "rev.so"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I", root, str(src), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    for name, (over, steps) in sorted(S.scenarios().items()):
        cfg = default_tracker_config(frame_w=FRAME[0], frame_h=FRAME[1], **over)
        k = StepCfg(cfg.track_cap, cfg.frame_w, cfg.frame_h, cfg.win_w, cfg.win_h, cfg.roi_scale_w, cfg.roi_scale_h, cfg.process_noise,
                    cfg.measurement_noise, cfg.error, cfg.tick_frequency)
        tr, side, st, org = np.zeros(0, abi.TRACK), np.zeros((0, 4, 2), np.float32), 0, (0, 0)
        rt, rs, rn, rst, ro = np.zeros(cfg.track_cap, abi.TRACK), np.zeros((cfg.track_cap, 4, 2), np.float32), C.c_int32(0), C.c_int32(0), np.zeros(1, abi.POINT)
        for arm, ids, pos, ts in steps[:70]:
            tr, side, st, org = Tracker.step_host(cfg, tr, side, st, org, arm, ids, pos, (0, 0), ts)
            i32 = None if ids is None else np.ascontiguousarray(ids, np.int32)
            f64 = None if pos is None else np.ascontiguousarray(pos, np.float64)
            rc = L.step_reversed(C.byref(k), abi.ptr(rt), abi.ptr(rs), C.byref(rn), C.byref(rst), abi.ptr(ro), abi.ptr(arm) if len(arm) else None, len(arm),
                                 abi.ptr(i32) if i32 is not None and len(arm) else None, abi.ptr(f64) if f64 is not None and len(arm) else None, 0, 0,
                                 C.c_int64(ts))
            assert rc == 0 and rn.value == len(tr) and rt[:rn.value].tobytes() == tr.tobytes() and rs[:rn.value].tobytes() == side.tobytes(), name
            assert (int(ro[0]["x"]), int(ro[0]["y"])) == org and rst.value == st, name
