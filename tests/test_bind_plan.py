"""bind_plan.h (rmcv_amd/csrc) against the code it replaced: compiled with the host C++ compiler, every decision of a batch context's host
side is compared, over whole grids and line by line, with the statements as they stood in rmcv_host.hip before the header, restated in
tests/bind_plan_ref.py (each function there names its lines): what a binding refuses and in which order and what it records in Geom
(set_geom, check_layout, check_windows, set_extent), when planes are re-zeroed and the frame order recomputed, the upload's device layout
and its refusal of the host's, check_params, the launches of run_stages, and the values rmcv_ctx_set_option takes."""
import itertools
import os
import subprocess

import pytest

import bind_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIM = (4, 70, 40)            # max_frames, max_width, max_height of the grids (small, so that "limit + 1" stays cheap)
GAINS = (7.5, 2.25)
OPTS = list(itertools.product(range(5), (8, 16), range(5), range(4), (0, 1)))   # format, sample bits, valid bit, orient, enhance
SIZES = (0, 1, 2, 3)         # ... and the limit and limit + 1 of each axis
STEP_FIELDS = ("status_clear", "enhance_tables", "window_origins", "frame_keys", "binary", "image", "sparse", "sparse_pairs", "sparse_identity", "contours", "match",
               "match_pairs", "blobs_armours", "blobs", "armours", "classify", "pnp")

SRC = r'''
#include <stdio.h>
#include <initializer_list>
#include "rmcv_amd/csrc/bind_plan.h"
using namespace rmcv;
static const Limits LIM = {4, 70, 40, 8, 8, 8, 8};
static void bind(const InputOptions& in, int n, int w, int h, int stride, long long pitch, int ww, int wh)
{
    printf("G %d %d %d %d %d %d %d %d %d %lld %d %d : ", in.format, in.sample_bits, in.valid_bit, in.orient, in.enhance, n, w, h, stride, pitch, ww, wh);
    const Refusal r = binding_refusal(LIM, in, n, w, h, stride, pitch, ww, wh);
    if (r) { printf("%d|%s\n", r.code, r.why); return; }
    Geom g;
    g.device = 3; g.n_cu = 5; g.pixel_halo_nt = 1; g.pixel_rowquad = 1; g.overloads = 2; g.contour_tier = 1;   // (not a binding's: they stay)
    g.input_format = g.sample_bytes = g.valid_bit = g.orient = g.n_frames = g.w = g.h = g.stride = g.ww = g.prow = g.enhance = g.win = g.frame_w = g.frame_h = g.keys = -7;
    g.frame_pitch = g.plane_pitch = -7; g.enh_max_gain = g.enh_min_gain = -7.0f;
    bind_geom(g, in, n, w, h, stride, pitch, ww, wh);
    printf("%d|%d %g %g %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %lld|%d %d %d %d %d %d\n", r.code, g.enhance, g.enh_max_gain, g.enh_min_gain, g.input_format, g.sample_bytes,
           g.valid_bit, g.orient, g.n_frames, g.stride, (long long)g.frame_pitch, g.frame_w, g.frame_h, g.win, g.keys, g.w, g.h, g.ww, g.prow, (long long)g.plane_pitch,
           g.device, g.n_cu, g.pixel_halo_nt, g.pixel_rowquad, g.overloads, g.contour_tier);
}
int main()
{
    const int ws[6] = {0, 1, 2, 3, LIM.max_width, LIM.max_width + 1}, hs[6] = {0, 1, 2, 3, LIM.max_height, LIM.max_height + 1};
    for (int fmt = 0; fmt < 5; fmt++) for (int bits : {8, 16}) for (int valid = 0; valid < 5; valid++) for (int orient = 0; orient < 4; orient++) for (int enh = 0; enh < 2; enh++) {
        InputOptions in;
        in.format = fmt; in.sample_bits = bits; in.valid_bit = valid; in.orient = orient; in.enhance = enh; in.max_gain = 7.5f; in.min_gain = 2.25f;
        const int bpp = in.pixel_bytes();
        // sizes, strides and pitches around every bound; one frame, whole frames
        for (int w : ws) for (int h : hs) for (int ds = -1; ds <= 2; ds++) for (int dp = -1; dp <= 1; dp++) {
            const int stride = bpp * w + ds;
            bind(in, 1, w, h, stride, (long long)stride * (h - 1) + bpp * w + dp, 0, 0);
        }
        // windows around the frame and the limits, frames at and below the limits
        const int fs[3][2] = {{3, 3}, {LIM.max_width, LIM.max_height}, {LIM.max_width, 3}};
        for (auto& f : fs) for (int ww : {0, 1, f[0], f[0] + 1, LIM.max_width + 1}) for (int wh : {0, 1, f[1], f[1] + 1, LIM.max_height + 1})
            bind(in, 2, f[0], f[1], bpp * f[0] + (bpp * f[0] & 1), (long long)(bpp * f[0] + (bpp * f[0] & 1)) * f[1], ww, wh);
        // frame counts around the limit (a refusal of the size behind it must wait)
        for (int n : {-1, 0, 1, LIM.max_frames, LIM.max_frames + 1}) for (int w : {0, 16}) bind(in, n, w, 8, bpp * 16, bpp * 16 * 8, 0, 0);
    }
    for (int w : {0, 1, 63, 64, 65, 128, 129}) for (int h : {0, 1, 39, 40}) {
        Geom g{};
        extent_fields(g, w, h);
        printf("F %d %d : %d %d %d %d %lld\n", w, h, g.w, g.h, g.ww, g.prow, (long long)g.plane_pitch);
    }
    for (int first = 0; first < 2; first++) for (int w : {63, 64, 65}) for (int h : {47, 48, 49}) for (int n : {3, 4, 5}) {
        const ExtentChange c = first ? extent_change(-1, -1, -1, -1, w, h, n) : extent_change(64, 48, 4, 48, w, h, n);
        printf("X %d %d %d %d : %d %d\n", first, w, h, n, (int)c.planes, (int)c.order);
    }
    for (int bpp = 1; bpp <= 3; bpp++) for (int w : {1, 5, 15, 16, 17, 31, 32, 33, 48}) for (int h : {1, 3}) {
        const UploadLayout l = upload_layout(bpp, w, h);
        for (int s : {bpp * w - 1, bpp * w, bpp * w + 1, l.stride}) for (long long dp : {-1, 0, 1, 1000}) {
            const long long pitch = dp == 1000 ? l.pitch : (long long)s * (h - 1) + bpp * w + dp;
            const char* no = l.refusal(s, pitch);
            printf("U %d %d %d %d %lld : %s|%d %lld %d\n", bpp, w, h, s, pitch, no ? no : "-", l.stride, (long long)l.pitch, (int)l.same(s, pitch));
        }
    }
    for (int have = 0; have < 2; have++) for (int morph : {-1, 0, 2, 3}) for (int stages : {-1, 0, 1, 15, 16, 32, 48, 127, 128}) for (int svm = 0; svm < 2; svm++) for (int pnp = 0; pnp < 2; pnp++) {
        rmcv_params p{};
        p.morph = morph;
        const char* no = stage_refusal(have ? &p : nullptr, stages, svm, pnp);
        printf("P %d %d %d %d %d : %s\n", have, morph, stages, svm, pnp, no ? no : "-");
    }
    // the run: every stage mask the ABI accepts; bit i of `m` = timed, legacy, Bayer format, enhance, win, keys
    for (int stages = 1; stages <= 127; stages++) for (int m = 0; m < 64; m++) {
        const RunSteps s = run_steps(stages, m & 1, (m >> 1) & 1, (m >> 2) & 1 ? RMCV_BAYER_BG : RMCV_INPUT_BGR, (m >> 3) & 1, (m >> 4) & 1, (m >> 5) & 1);
        printf("S %d %d : %s|%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", stages, m, s.refusal ? s.refusal : "-", s.status_clear, (int)s.enhance_tables, (int)s.window_origins,
               (int)s.frame_keys, (int)s.binary, (int)s.image, (int)s.sparse, (int)s.sparse_pairs, (int)s.sparse_identity, (int)s.contours, (int)s.match, (int)s.match_pairs,
               (int)s.blobs_armours, (int)s.blobs, (int)s.armours, (int)s.classify, (int)s.pnp);
    }
    for (int last : {0, 5, 15, 63}) for (int stages = 1; stages <= 127; stages++) printf("N %d %d : %d\n", last, stages, next_last_stages(last, stages));
    for (int option = -1; option <= 1002; option++) {
        if (option == 31) option = 999;
        const OptionRule* r = option_rule(option);
        printf("E %d : %d %d %d\n", option, r ? 1 : 0, r ? r->lo : 0, r ? r->hi : 0);
        for (int v = -1; v <= 17; v++) printf("O %d %d : %d\n", option, v, (int)(r && r->accepts(v)));
        if (r)
            for (long long v : {r->lo - 1ll, r->lo + 1ll, r->hi - 1ll, (long long)r->hi, r->hi + 1ll})
                if (v <= INT_MAX) printf("O %d %lld : %d\n", option, v, (int)r->accepts((int)v));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("bind_plan")
    src = d / "bind_plan.cpp"
    src.write_text(SRC)
    out = d / "bind_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(out)], check=True)
    rows = {}
    for ln in subprocess.run([str(out)], check=True, capture_output=True, text=True).stdout.splitlines():
        rows.setdefault(ln[0], []).append(ln[2:])
    return rows


def bind_line(opt, n, w, h, stride, pitch, ww, wh):
    code, why = R.set_geom_refusal(LIM, opt, n, w, h, stride, pitch, ww, wh)
    head = "%d %d %d %d %d %d %d %d %d %d %d %d : " % (opt + (n, w, h, stride, pitch, ww, wh))
    if code:
        return head + "%d|%s" % (code, why)
    f = R.set_geom_fields(opt, GAINS, n, w, h, stride, pitch, ww, wh)
    return head + "0|%d %g %g " % f[:3] + " ".join(str(v) for v in f[3:]) + "|3 5 1 1 2 1"


def test_binding_refusals_in_order_and_bound_fields(table):
    want = []
    ws, hs = SIZES + (LIM[1], LIM[1] + 1), SIZES + (LIM[2], LIM[2] + 1)
    for opt in OPTS:
        bpp = R.pixel_bytes(opt[0], opt[1])
        for w, h, ds, dp in itertools.product(ws, hs, (-1, 0, 1, 2), (-1, 0, 1)):
            stride = bpp * w + ds
            want.append(bind_line(opt, 1, w, h, stride, stride * (h - 1) + bpp * w + dp, 0, 0))
        for fw, fh in ((3, 3), (LIM[1], LIM[2]), (LIM[1], 3)):
            stride = bpp * fw + (bpp * fw & 1)
            for ww, wh in itertools.product((0, 1, fw, fw + 1, LIM[1] + 1), (0, 1, fh, fh + 1, LIM[2] + 1)):
                want.append(bind_line(opt, 2, fw, fh, stride, stride * fh, ww, wh))
        for n, w in itertools.product((-1, 0, 1, LIM[0], LIM[0] + 1), (0, 16)):
            want.append(bind_line(opt, n, w, 8, bpp * 16, bpp * 16 * 8, 0, 0))
    got = table["G"]
    assert len(got) == len(want) == len(OPTS) * (36 * 12 + 75 + 10)
    for g, w in zip(got, want):
        assert g == w
    # every message is reached, each also as the FIRST of several that apply (the order is the parent's), and bindings pass in every format
    seen = {ln.split("|")[1] for ln in got if ln.split(" : ")[1].startswith("-1|")}
    assert seen == {"n_frames out of range", "frame size out of range", R.LAYOUT_BITS, R.LAYOUT_ORIENT, "a Bayer frame needs w >= 3 and h >= 3", "bad stride/pitch", R.EVEN,
                    R.ENH_BAYER, R.WIN_BAYER, R.WIN_ENH, R.WIN_SMALL, R.WIN_FRAMES}   # (R.WIN_LIMITS: a window inside the frame is inside the limits)
    assert R.set_geom_refusal(LIM, (0, 16, 0, 1, 0), 0, 0, 0, 0, 0, 0, 0)[1] == "n_frames out of range"
    assert R.set_geom_refusal(LIM, (1, 16, 0, 0, 1), 1, 2, 2, 3, 3, 1, 1)[1] == "a Bayer frame needs w >= 3 and h >= 3"
    assert R.set_geom_refusal(LIM, (1, 16, 0, 0, 1), 1, 3, 3, 7, 21, 4, 4)[1] == R.EVEN
    assert {int(ln.split()[0]) for ln in got if " : 0|" in ln} == set(range(5))


def test_extent_fields_and_change(table):
    rows = {tuple(int(v) for v in a.split()): tuple(int(v) for v in b.split()) for a, b in (ln.split(":") for ln in table["F"])}
    assert set(rows) == set(itertools.product((0, 1, 63, 64, 65, 128, 129), (0, 1, 39, 40)))
    for (w, h), g in rows.items():
        assert g == R.extent(w, h)
    rows = {tuple(int(v) for v in a.split()): tuple(int(v) for v in b.split()) for a, b in (ln.split(":") for ln in table["X"])}
    assert set(rows) == set(itertools.product((0, 1), (63, 64, 65), (47, 48, 49), (3, 4, 5)))
    for (first, w, h, n), g in rows.items():
        prev = (-1, -1, -1, -1) if first else (64, 48, 4, 48)
        assert g == tuple(int(v) for v in R.extent_change(*prev, w, h, n)), (first, w, h, n)
    assert rows[(0, 64, 48, 4)] == (0, 0) and rows[(0, 65, 48, 4)] == (1, 0) and rows[(0, 64, 48, 5)] == (0, 1) and rows[(0, 64, 49, 4)] == (1, 1)


def test_upload_layout(table):
    want = []
    for bpp, w, h in itertools.product((1, 2, 3), (1, 5, 15, 16, 17, 31, 32, 33, 48), (1, 3)):
        dstride = R.upload(bpp, w, h, 0, 0)[1]
        for s, dp in itertools.product((bpp * w - 1, bpp * w, bpp * w + 1, dstride), (-1, 0, 1, 1000)):
            pitch = dstride * h if dp == 1000 else s * (h - 1) + bpp * w + dp
            why, ds, dpitch, same = R.upload(bpp, w, h, s, pitch)
            assert ds % 16 == 0 and 0 <= ds - bpp * w < 16
            want.append("%d %d %d %d %d : %s|%d %d %d" % (bpp, w, h, s, pitch, why or "-", ds, dpitch, same))
    assert table["U"] == want
    assert any("|" in ln and ln.endswith(" 1") for ln in want) and any(R.EVEN in ln for ln in want) and any("bad stride/pitch" in ln for ln in want)


def test_stage_refusal(table):
    want = ["%d %d %d %d %d : %s" % (have, morph, stages, svm, pnp, R.check_params(have, morph, stages, svm, pnp) or "-")
            for have, morph, stages, svm, pnp in itertools.product((0, 1), (-1, 0, 2, 3), (-1, 0, 1, 15, 16, 32, 48, 127, 128), (0, 1), (0, 1))]
    assert table["P"] == want
    assert {ln.split(" : ")[1] for ln in want} == {"-", "null params", "bad morph", "bad stage mask", "RMCV_STAGE_IDENTITY needs rmcv_svm_load first",
                                                   "RMCV_STAGE_POSE needs rmcv_pnp_load first"}


def steps_of(ladder):
    """the flat record of a ladder's launches, in STEP_FIELDS' order; a launch must not appear twice"""
    names = [l[0] for l in ladder]
    assert len(names) == len(set(names))
    d = {l[0]: l for l in ladder}
    s = dict.fromkeys(STEP_FIELDS, 0)
    s["status_clear"] = d["status_clear"][1] if "status_clear" in d else 0
    for k in ("enhance_tables", "window_origins", "frame_keys", "binary", "sparse", "contours", "match", "blobs_armours", "blobs", "armours", "classify", "pnp"):
        s[k] = int(k in d)
    if "binary" in d:
        s["image"] = d["binary"][1]
    if "sparse" in d:
        s["sparse_pairs"], s["sparse_identity"] = d["sparse"][1:]
    if "match" in d:
        s["match_pairs"] = d["match"][1]
    return s


ORDER = ("status_clear", "enhance_tables", "window_origins", "frame_keys", "binary", "sparse", "contours", "match", "blobs_armours", "blobs", "armours", "classify", "pnp")


def test_run_steps_are_the_ladder(table):
    got = table["S"]
    assert len(got) == 127 * 64
    it = iter(got)
    for stages, m in itertools.product(range(1, 128), range(64)):
        timed, legacy, fmt, enh, win, keys = ((m >> i) & 1 for i in range(6))
        why, ladder = R.run_ladder(stages, timed, legacy, 4 * fmt, enh, win, keys)
        s = steps_of(ladder)
        assert next(it) == "%d %d : %s|%s" % (stages, m, why or "-", " ".join(str(s[k]) for k in STEP_FIELDS)), (stages, m)
        assert [l[0] for l in ladder] == [k for k in ORDER if s[k]]          # run_stages enqueues in the order of the record's fields
        # what the ladder implies: blobs and armours each come from exactly one launch when asked for, from none otherwise; the classifier
        # has a launch of its own exactly when identities are asked for and do not ride in the fused kernel; the prologues go with the pixel pass
        assert s["sparse"] + s["match"] + s["blobs_armours"] + s["blobs"] == int(bool(stages & R.STAGE_BLOBS))
        assert s["sparse_pairs"] + s["match_pairs"] + s["blobs_armours"] + s["armours"] == int(bool(stages & R.STAGE_ARMOURS))
        assert s["sparse"] + s["contours"] == int(bool(stages & R.STAGE_CONTOURS))
        assert s["classify"] == int(bool(stages & R.STAGE_IDENTITY) and not s["sparse_identity"])
        assert s["sparse_identity"] <= s["sparse_pairs"] <= s["sparse"] and s["match_pairs"] <= s["match"] and s["image"] <= s["binary"]
        assert (s["enhance_tables"], s["window_origins"], s["frame_keys"]) == tuple(s["binary"] * v for v in (enh, win, keys))
        assert bool(s["status_clear"]) <= (not stages & R.STAGE_CONTOURS) and (why is None or legacy)
    rows = {tuple(int(v) for v in a.split()): int(b) for a, b in (ln.split(":") for ln in table["N"])}
    assert set(rows) == set(itertools.product((0, 5, 15, 63), range(1, 128)))
    for (last, stages), g in rows.items():
        assert g == R.next_last_stages(last, stages)


def test_option_rules(table):
    ends = {int(a): tuple(int(v) for v in b.split()) for a, b in (ln.split(":") for ln in table["E"])}
    assert set(ends) == set(range(-1, 31)) | {999, 1000, 1001, 1002}
    assert {o for o, e in ends.items() if e[0]} == set(R.OPTIONS) == set(R.OPTION_ENDS)
    for o, (lo, hi) in R.OPTION_ENDS.items():
        assert ends[o] == (1, lo, hi)
    seen = {}
    for ln in table["O"]:
        (o, v), acc = (int(x) for x in ln.split(":")[0].split()), int(ln.split(":")[1])
        assert acc == (int(R.OPTIONS[o](v)) if o in R.OPTIONS else 0), (o, v)
        seen.setdefault(o, set()).add(v)
    for o in ends:
        need = set(range(-1, 18))
        if o in R.OPTIONS:
            lo, hi = R.OPTION_ENDS[o]
            need |= {v for v in (lo - 1, lo + 1, hi - 1, hi, hi + 1) if v <= R.INT_MAX}
            assert R.OPTIONS[o](lo) and R.OPTIONS[o](hi) and not R.OPTIONS[o](lo - 1) and (hi == R.INT_MAX or not R.OPTIONS[o](hi + 1))
        assert seen[o] == need, o
