"""view_plan.h (rmcv_amd/csrc) compiled with the host C++ compiler alone: the frame-list rule -- a list, 1 <= n <= n_frames, every index inside
the batch, none twice -- and the five refusal functions that read it (debug_views_refusal, source_views_refusal, icon_strips_refusal,
corners_refusal, chessboards_refusal) against tests/view_plan_ref.py, the Python restatement of what each of them was before the rule was
written once.  For every function the grid holds the accepted case, every single fault of its list, every PAIR of faults at once -- which
message wins is part of the contract -- and n = 1 with out_pitch = 0.  No GPU."""
import itertools
import os
import subprocess

import pytest

import view_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rmcv_amd/csrc/chess_plan.h"
#include "rmcv_amd/csrc/corner_plan.h"
#include "rmcv_amd/csrc/icon_strip_plan.h"
#include "rmcv_amd/csrc/source_view_plan.h"
#include "rmcv_amd/csrc/view_plan.h"
using namespace rmcv;
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    char fn[8], list[256];
    static const char table = 0;
    while (fscanf(f, "%7s %255s", fn, list) == 2) {
        int32_t fr[64];
        int len = 0;
        const bool null = !strcmp(list, "-");
        for (char* t = strtok(list, ","); !null && t; t = strtok(nullptr, ",")) fr[len++] = atoi(t);
        const int32_t* frames = null ? nullptr : fr;
        int n, nf, a[16];
        long long pitch;
        double eps;
        const char* why = nullptr;
        if (fscanf(f, "%d %d", &n, &nf) != 2) return 2;
        if (fn[0] == 'L') {
            printf("%d\n", (int)frame_list_fault(frames, n, nf));
            continue;
        } else if (fn[0] == 'D' || fn[0] == 'S') { // stages need vw vh max_width max_height flags out_stride out_pitch
            if (fscanf(f, "%d %d %d %d %d %d %d %d %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, &pitch) != 9) return 2;
            why = (fn[0] == 'D' ? debug_views_refusal : source_views_refusal)(frames, n, nf, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], pitch);
        } else if (fn[0] == 'I') { // stages side cap max_armours out_stride out_pitch
            if (fscanf(f, "%d %d %d %d %d %lld", a, a + 1, a + 2, a + 3, a + 4, &pitch) != 6) return 2;
            why = icon_strips_refusal(frames, n, nf, a[0], a[1], a[2], a[3], a[4], pitch);
        } else if (fn[0] == 'C') { // kind stages d_corners per_frame win_x win_y zero_x zero_y max_iters eps
            if (fscanf(f, "%d %d %d %d %d %d %d %d %d %lf", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, &eps) != 10) return 2;
            why = corners_refusal(frames, n, nf, a[0], a[1], a[2] ? &table : nullptr, a[3], a[4], a[5], a[6], a[7], a[8], eps);
        } else if (fn[0] == 'H') { // kind stages d_corners d_counts per_frame cols rows threshold contrast nms dist_min dist_max
            if (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10, a + 11) != 12) return 2;
            const rmcv_chess_params p = {a[7], a[8], a[9], a[10], a[11]};
            why = chessboards_refusal(frames, n, nf, a[0], a[1], a[2] ? &table : nullptr, a[3] ? &table : nullptr, a[4], a[5], a[6], p);
        } else return 3;
        printf("%s\n", why ? why : "");
    }
    fclose(f);
    return 0;
}
'''

# ---- the faults.  A fault edits a case; the layout (out_stride, out_pitch) is worked out from the case's final sizes, so that a fault of a
# size is that fault alone


def edit(**kw):
    return lambda c: c.update(kw)


def at(k, value=None, same_as=None):
    def f(c):
        c["frames"] = list(c["frames"])
        c["frames"][k] = c["frames"][same_as] if same_as is not None else (c["n_frames"] if value == "n_frames" else value)
    return f


LIST_FAULTS = [("null", edit(null=True)), ("n=0", edit(n=0)), ("n>n_frames", lambda c: c.update(n_frames=c["n"] - 1)), ("index -1", at(2, -1)),
               ("index n_frames", at(2, "n_frames")), ("repeat (0,1)", at(1, same_as=0)), ("repeat (0,n-1)", at(-1, same_as=0))]
LIST = dict(frames=[3, 1, 4, 0], n=4, n_frames=6, null=False)

VIEW = dict(LIST, stages=R.STAGE_ALL, flags=R.VIEW_ALL, vw=10, vh=8, max_width=64, max_height=48, d_stride=0, d_pitch=0)
VIEW_FAULTS = LIST_FAULTS + [("flags 8", edit(flags=8)), ("flags -1", edit(flags=-1)), ("vw 0", edit(vw=0)), ("vh 0", edit(vh=0)), ("vw > max", edit(vw=65)),
                             ("vh > max", edit(vh=49)), ("stride", edit(d_stride=-1)), ("pitch", edit(d_pitch=-1)), ("stages", edit(stages=R.STAGE_BINARY))]
STRIP = dict(LIST, stages=R.STAGE_ALL, side=20, cap=5, max_armours=8, d_stride=0, d_pitch=0)
STRIP_FAULTS = LIST_FAULTS + [("side 0", edit(side=0)), ("side 257", edit(side=257)), ("cap 0", edit(cap=0)), ("cap > max_armours", edit(cap=9)),
                              ("stride", edit(d_stride=-1)), ("pitch", edit(d_pitch=-1)), ("stages", edit(stages=7))]
CORNER = dict(LIST, kind=R.SOURCE_BGR, stages=0, d_corners=1, per_frame=54, win_x=8, win_y=5, zero_x=-1, zero_y=-1, max_iters=40, eps=0.001)
CORNER_FAULTS = LIST_FAULTS + [("null table", edit(d_corners=0)), ("per_frame 0", edit(per_frame=0)), ("per_frame 1025", edit(per_frame=1025)), ("win 0", edit(win_x=0)),
                               ("win 16", edit(win_y=16)), ("zero zone", edit(zero_x=8, zero_y=0)), ("iters 0", edit(max_iters=0)), ("iters 101", edit(max_iters=101)),
                               ("eps < 0", edit(eps=-1.0)), ("windowed, no run", edit(kind=R.SOURCE_BGR_WIN)), ("enhanced, no run", edit(kind=R.SOURCE_BGR_LUT))]
CHESS = dict(LIST, kind=R.SOURCE_BGR, stages=0, d_corners=1, d_counts=1, per_frame=54, cols=9, rows=6, threshold=1000, contrast=10, nms=3, dist_min=6, dist_max=255)
CHESS_FAULTS = LIST_FAULTS + [("null corners", edit(d_corners=0)), ("null counts", edit(d_counts=0)), ("cols 1", edit(cols=1)), ("rows 33", edit(rows=33)),
                              ("threshold", edit(threshold=-1)), ("contrast", edit(contrast=256)), ("nms", edit(nms=8)), ("dist", edit(dist_min=7, dist_max=6)),
                              ("per_frame", edit(per_frame=53)), ("per_frame 1025", edit(per_frame=1025)), ("windowed, no run", edit(kind=R.SOURCE_BGR_WIN))]


def layout(c, row, rows):
    """out_stride and out_pitch: the least the function accepts for the case's sizes, plus what a fault took off"""
    c["out_stride"] = row + c["d_stride"]
    c["out_pitch"] = c["out_stride"] * (rows - 1) + row + c["d_pitch"]


def finish_view(c):
    c["need"] = R.view_stages_needed(c["flags"] & R.VIEW_ALL)
    layout(c, 3 * c["vw"], c["vh"])


def finish_strip(c):
    layout(c, 3 * c["cap"] * c["side"], c["side"])


def frames_word(c):
    return "-" if c["null"] else ",".join(map(str, c["frames"]))


FUNCTIONS = {
    "D": (VIEW, VIEW_FAULTS, finish_view, R.debug_views, "stages need vw vh max_width max_height flags out_stride out_pitch"),
    "S": (VIEW, VIEW_FAULTS, finish_view, R.source_views, "stages need vw vh max_width max_height flags out_stride out_pitch"),
    "I": (STRIP, STRIP_FAULTS, finish_strip, R.icon_strips, "stages side cap max_armours out_stride out_pitch"),
    "C": (CORNER, CORNER_FAULTS, None, R.corners, "kind stages d_corners per_frame win_x win_y zero_x zero_y max_iters eps"),
    "H": (CHESS, CHESS_FAULTS, None, R.chessboards, "kind stages d_corners d_counts per_frame cols rows threshold contrast nms dist_min dist_max"),
}


def grid(key):
    """(name, case) of the accepted case, every single fault, every pair, and -- a function with a layout -- n = 1 with out_pitch = 0"""
    base, faults, finish, _, _ = FUNCTIONS[key]
    combos = [()] + [(f,) for f in faults] + list(itertools.combinations(faults, 2))
    out = []
    for combo in combos:
        c = dict(base)
        for _, fault in combo:
            fault(c)
        if finish:
            finish(c)
        out.append((" + ".join(name for name, _ in combo) or "accepted", c))
    if finish:
        c = dict(base, frames=[5], n=1)
        finish(c)
        c["out_pitch"] = 0
        out.append(("n = 1, out_pitch = 0", c))
    return out


def as_ref(c):
    return dict(c, frames=None if c["null"] else c["frames"])


def rule_cases():
    """the rule alone: every list of the grids above, and lists as long as the batch"""
    cases = [c for _, c in grid("C")]
    cases += [dict(LIST, frames=list(range(8)), n=8, n_frames=8), dict(LIST, frames=[7, 6, 5, 4, 3, 2, 1, 7], n=8, n_frames=8),
              dict(LIST, frames=[0, 1, 2, 3, 4, 5, 6, 8], n=8, n_frames=8), dict(LIST, frames=[0], n=1, n_frames=1), dict(LIST, frames=[1], n=1, n_frames=1)]
    return cases


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_plan")
    with open(d / "main.cpp", "w") as f:
        f.write(SRC)
    with open(d / "cases.txt", "w") as f:
        for key, (_, _, _, _, fields) in FUNCTIONS.items():
            for _, c in grid(key):
                f.write("%s %s %d %d %s\n" % (key, frames_word(c), c["n"], c["n_frames"], " ".join(repr(c[k]) for k in fields.split())))
        for c in rule_cases():
            f.write("L %s %d %d\n" % (frames_word(c), c["n"], c["n_frames"]))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", ROOT, str(d / "main.cpp"), "-o", str(d / "plan")], check=True)
    lines = subprocess.run([str(d / "plan"), str(d / "cases.txt")], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    out = {}
    for key in FUNCTIONS:
        out[key], lines = lines[:len(grid(key))], lines[len(grid(key)):]
    out["L"] = lines
    return out


@pytest.mark.parametrize("key", list(FUNCTIONS))
def test_refusals_are_the_parents(answers, key):
    ref = FUNCTIONS[key][3]
    cases = grid(key)
    assert len(answers[key]) == len(cases)
    got = {name: line for (name, _), line in zip(cases, answers[key])}
    want = {name: ref(as_ref(c)) or "" for name, c in cases}
    assert got == want
    # the grid is what it says: the accepted case and the one-view case pass, every single fault is refused, and the list's faults are told apart
    assert want["accepted"] == "" and want.get("n = 1, out_pitch = 0", "") == ""
    singles = [want[name] for name, _ in FUNCTIONS[key][1]]
    assert all(singles) and len(set(singles[:7])) == 4


def test_the_rule(answers):
    cases = rule_cases()
    assert [int(x) for x in answers["L"]] == [R.frame_list_fault(as_ref(c)["frames"], c["n"], c["n_frames"]) for c in cases]
    assert {int(x) for x in answers["L"]} == {R.OK, R.NONE, R.TOO_MANY, R.OUTSIDE, R.REPEATED}


def test_which_message_wins():
    """what the grid pins, spelled out on the restatement: the count in front of a layout fault, a layout fault in front of an index, an index
    outside the batch in front of a repeat further up the list and behind one in front of it"""
    def source(*names):
        c = dict(VIEW)
        for name, fault in VIEW_FAULTS:
            if name in names:
                fault(c)
        finish_view(c)
        return R.source_views(as_ref(c))
    assert source("n>n_frames", "stride") == "source views: more views than the batch has frames"
    assert source("stride", "index -1") == "source views: out_stride < 3 vw"
    assert source("index -1", "stages") == "source views: a frame index is outside the batch"
    assert source("index -1", "repeat (0,n-1)") == "source views: a frame index is outside the batch"
    assert source("index -1", "repeat (0,1)") == "source views: a frame index is repeated"
