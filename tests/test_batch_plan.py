"""batch_plan.h (rmcv_amd/csrc) against the code it replaced: compiled with the host C++ compiler, every decision of the pipelined schedule
is compared, over whole grids, with the statements as they stood in rmcv_pipeline.hip before the header, restated in tests/batch_plan_ref.py
(each function there names its lines): the configuration (175-189, 227-257), the record's layout (275-277) and report word (514, 618-619),
hot_for and the range rule of rmcv_pipeline_set_hot_contexts (422-430, 403-404), the stream's mood and the split rule (621-622, 515), the
front and back halves of a batch's plan (628-638, 667-668; 499-520, 531-540), a ticket's slot and streams (610, 669, 682), the burst
hold-back (700-716) and the submit refusals (598-605, 648-658).

The hold-back has a floor: a launch expected to take less than 100 us is not held back at all (line 710), so 48 frames of 1280x1024 -- 45.8 us
of launch -- are held for 0 us, not for a quarter of that; the quarter shows from 100 us on (128 frames: 122 us -> 30 us)."""
import itertools
import os
import subprocess

import pytest

import batch_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEPTHS = (1, 2, 3, 4, 8, 64, 65)
STREAMS = (-1, 0, 1, 4, 16, 17)
GEOMS = ((256, 1280, 1024), (256, 1920, 1200), (96, 1920, 1200), (32, 640, 512), (1, 1, 1))
HOLD_SHAPES = ((16, 640, 512), (48, 1280, 1024), (256, 1280, 1024), (256, 1920, 1200), (128, 1280, 1024))
PLACES = ((8, 2, 4), (3, 2, 3), (1, 1, 1), (64, 16, 16), (5, 2, 4))

SRC = r'''
#include <stdio.h>
#include <initializer_list>
#include "rmcv_amd/csrc/batch_plan.h"
using namespace rmcv;
static int hots(int depth, int* out) // -1, 0, 2, 3, depth - 1, depth, without repeats
{
    const int all[6] = {-1, 0, 2, 3, depth - 1, depth};
    int n = 0;
    for (int i = 0; i < 6; i++) {
        bool seen = false;
        for (int j = 0; j < n; j++) seen |= out[j] == all[i];
        if (!seen) out[n++] = all[i];
    }
    return n;
}
static void print_config(const rmcv_pipeline_config* c)
{
    const BatchConfig r = resolve_config(c);
    const rmcv_pipeline_config& d = r.cfg;
    printf(": %d %d %d %d %d %d %d %d %d %d %d\n", r.rc, d.depth, d.pixel_streams, d.sparse_streams, d.armour_cap, d.sparse_waves, d.pixel_groups, d.host_results,
           d.dense_streams, d.hot_contexts, r.hot_cfg);
}
int main()
{
    const int depths[7] = {1, 2, 3, 4, 8, 64, 65}, streams[6] = {-1, 0, 1, 4, 16, 17}, waves[3] = {0, 4, 8}, groups[3] = {0, 2, 3};
    printf("C null ");
    print_config(nullptr);
    for (int depth : depths) for (int ps : streams) for (int ss : streams) for (int ds : streams) for (int sw : waves) for (int pg : groups)
        for (int hr = 0; hr < 4; hr++) {
            int hot[6];
            const int nh = hots(depth, hot);
            for (int i = 0; i < nh; i++) {
                rmcv_pipeline_config c = {depth, ps, ss, (depth + hr) % 2 ? 100 : 0, sw, pg, hr, ds, hot[i], 0};
                printf("C %d %d %d %d %d %d %d %d %d ", c.depth, c.pixel_streams, c.sparse_streams, c.armour_cap, c.sparse_waves, c.pixel_groups, c.host_results, c.dense_streams, c.hot_contexts);
                print_config(&c);
            }
        }
    {
        const rmcv_pipeline_config d = default_batch_config();
        printf("D %d %d %d %d %d %d %d %d %d %d\n", d.depth, d.pixel_streams, d.sparse_streams, d.armour_cap, d.sparse_waves, d.pixel_groups, d.host_results, d.dense_streams, d.hot_contexts, d._reserved);
    }
    for (int mf : {1, 2, 3, 5, 256}) for (int cap : {0, 1, 100}) {
        const RecordLayout l = record_layout(mf, cap);
        printf("L %d %d : %d %lld %lld %d %d\n", mf, cap, l.armour_cap, (long long)l.head_bytes, (long long)l.record_bytes, l.status_word, l.report_word);
    }
    printf("S %zu\n", sizeof(rmcv_armour));
    const int geoms[5][3] = {{256, 1280, 1024}, {256, 1920, 1200}, {96, 1920, 1200}, {32, 640, 512}, {1, 1, 1}};
    for (int hc : {-1, 0, 5}) for (int depth : {4, 8}) for (auto& g : geoms) printf("H %d %d %d %d %d : %d\n", hc, depth, g[0], g[1], g[2], hot_for(hc, depth, g[0], g[1], g[2]));
    for (int n = -1; n <= 9; n++) for (int depth : {4, 8}) for (int hr : {1, 2}) for (int sw : {4, 8}) {
        rmcv_pipeline_config c = default_batch_config();
        c.depth = depth; c.host_results = hr; c.sparse_waves = sw;
        const char* no = n > 0 ? hot_contexts_refusal(n, c) : nullptr;
        printf("N %d %d %d %d : %s\n", n, depth, hr, sw, no ? no : "-");
    }
    for (int n : {8, 48, 256}) for (int dense : {0, 1, n / 8, n / 8 + 1, n}) for (unsigned p16 : {0u, 74u, 75u, 93u, 94u, 4095u}) for (int lean = 0; lean < 2; lean++) {
        const uint32_t word = (uint32_t)dense | (p16 << 20);
        const RecordReport r = record_report(word);
        const Mood m = stream_mood(r, lean != 0, n);
        printf("M %d %u %d : %d %d %d %d %d\n", n, word, lean, r.dense, r.points, (int)m.heavy, (int)m.calm, (int)split_rule(r, n));
    }
    // the front half: bit i of `b` = hot (4), calm, heavy, legacy, POSE, IDENTITY, CONTOURS, BLOBS, ws_variant, tracked, host_results (2), sparse_waves (8), hot_seq (5), k (7)
    for (int b = 0; b < (1 << 14); b++) {
        const auto bit = [b](int i) { return (b >> i) & 1; };
        rmcv_pipeline_config c = default_batch_config();
        c.host_results = bit(10) ? 2 : 1;
        c.sparse_waves = bit(11) ? 8 : 4;
        const int stages = RMCV_STAGE_BINARY | RMCV_STAGE_ARMOURS | (bit(4) ? RMCV_STAGE_POSE : 0) | (bit(5) ? RMCV_STAGE_IDENTITY : 0) | (bit(6) ? RMCV_STAGE_CONTOURS : 0) | (bit(7) ? RMCV_STAGE_BLOBS : 0);
        const size_t k = bit(13) ? 7 : 0;
        const FrontPlan f = front_plan(bit(0) ? 4 : 0, bit(1), bit(2), c, stages, bit(3), bit(8), bit(9), bit(12) ? 5 : 0, k);
        const RunPlan in = {7, 2, c.sparse_waves, bit(13) ? SPARSE_SPLIT_BOTH : SPARSE_STANDARD}, out = f.plan(in); // (the context's options: whatever they are)
        printf("F %d : %d %d %zu %d %d %d %d\n", b, (int)f.fast, (int)f.heavy, f.j, out.pixel_ws, out.pixel_groups, out.sparse_waves, (int)out.form);
    }
    // the back half: bit i of `b` = latency, sparse_waves (8), legacy, form (SPARSE_LEAN), split_now, dense streams (4), CONTOURS, BLOBS, k (5)
    for (int b = 0; b < (1 << 9); b++) {
        const auto bit = [b](int i) { return (b >> i) & 1; };
        rmcv_pipeline_config c = default_batch_config();
        c.sparse_waves = bit(1) ? 8 : 4;
        const RunPlan plan = {1, 2, c.sparse_waves, bit(3) ? SPARSE_LEAN : SPARSE_STANDARD};
        const int sparse = RMCV_STAGE_ARMOURS | (bit(6) ? RMCV_STAGE_CONTOURS : 0) | (bit(7) ? RMCV_STAGE_BLOBS : 0);
        const BackPlan p = back_plan(bit(0), c, bit(2), plan, bit(4), bit(5) ? 4 : 0, sparse, bit(8) ? 5 : 0);
        printf("B %d : %d %d %d %d %d %d\n", b, (int)p.w8, (int)p.split, p.sparse_waves, (int)p.first, (int)p.second, p.dense_stream);
    }
    const int places[5][3] = {{8, 2, 4}, {3, 2, 3}, {1, 1, 1}, {64, 16, 16}, {5, 2, 4}};
    for (auto& pc : places) for (uint64_t t = 0; t < 140; t++) {
        rmcv_pipeline_config c = default_batch_config();
        c.depth = pc[0]; c.pixel_streams = pc[1]; c.sparse_streams = pc[2];
        const TicketPlace at = ticket_place(t, c);
        printf("T %d %d %d %llu : %zu %zu %zu\n", pc[0], pc[1], pc[2], (unsigned long long)t, at.slot, at.pixel, at.sparse);
    }
    printf("E %d %d %d\n", (int)waits_for_free(&places[0], &places[1]), (int)waits_for_free(&places[1], &places[1]), (int)waits_for_free(nullptr, &places[1]));
    const int shapes[5][3] = {{16, 640, 512}, {48, 1280, 1024}, {256, 1280, 1024}, {256, 1920, 1200}, {128, 1280, 1024}};
    for (auto& s : shapes) for (uint64_t t : {0, 1, 9}) for (int b = 0; b < 32; b++) {
        const HoldBack hb = hold_back(b & 1, t, (b >> 1) & 1, (b >> 2) & 1, (b >> 3) & 1, (b >> 4) & 1, s[0], s[1], s[2]);
        printf("K %d %d %d %llu %d : %d %d\n", s[0], s[1], s[2], (unsigned long long)t, b, (int)hb.cold, hb.hold_us);
    }
    // the refusals: "R <case> : code|message"
    rmcv_tracker_config tc{};
    tc.n_streams = 16; tc.frame_w = 640; tc.frame_h = 512;
    const int all = RMCV_STAGE_ALL;
    char buf[3][200];
    const char* rs[11] = {
        tracked_refusal(0, 0, tc, 16, 640, 512, all, false, false), tracked_refusal(0, 0, tc, 16, 640, 512, all, true, true),
        tracked_refusal(1, 0, tc, 16, 640, 512, all, false, false), tracked_refusal(0, 0, tc, 15, 640, 512, all, false, false),
        tracked_refusal(0, 0, tc, 16, 641, 512, all, false, false), tracked_refusal(0, 0, tc, 16, 640, 511, all, false, false),
        tracked_refusal(0, 0, tc, 16, 640, 512, all & ~RMCV_STAGE_ARMOURS, false, false), tracked_refusal(0, 0, tc, 16, 640, 512, all, true, false),
        cameras_refusal(16, 16, true, buf[0]), cameras_refusal(16, 256, true, buf[1]), cameras_refusal(16, 16, false, buf[2])};
    for (int i = 0; i < 11; i++) printf("R %d : %s\n", i, rs[i] ? rs[i] : "-");
    return 0;
}
'''


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_plan")
    src = d / "batch_plan.cpp"
    src.write_text(SRC)
    out = d / "batch_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(out)], check=True)
    rows = {}
    for ln in subprocess.run([str(out)], check=True, capture_output=True, text=True).stdout.splitlines():
        rows.setdefault(ln[0], []).append(ln[2:])
    return rows


def ints(s):
    return tuple(int(v) for v in s.split())


def test_config_resolution(table):
    got = {}
    for ln in table["C"]:
        given, res = ln.split(":")
        got[given.strip()] = ints(res)
    want_keys = {"null"}
    for depth, ps, ss, ds, sw, pg, hr in itertools.product(DEPTHS, STREAMS, STREAMS, STREAMS, (0, 4, 8), (0, 2, 3), (0, 1, 2, 3)):
        for hot in {-1, 0, 2, 3, depth - 1, depth}:
            cfg = dict(zip(R.CONFIG_FIELDS, (depth, ps, ss, 100 if (depth + hr) % 2 else 0, sw, pg, hr, ds, hot)))
            key = " ".join(str(cfg[k]) for k in R.CONFIG_FIELDS)
            want_keys.add(key)
            rc, d, hot_cfg = R.config(cfg)
            g = got[key]
            assert g[0] == rc, (key, g)
            if rc == 0:
                assert g[1:] == tuple(d[k] for k in R.CONFIG_FIELDS) + (hot_cfg,), (key, g, d, hot_cfg)
    assert set(got) == want_keys and len(got) > 250000
    rc, d, hot_cfg = R.config(None)
    assert got["null"] == (0,) + tuple(d[k] for k in R.CONFIG_FIELDS) + (hot_cfg,) == (0, 8, 2, 4, 0, 4, 2, 1, 4, 0, 0)
    assert ints(table["D"][0]) == tuple(R.DEFAULTS[k] for k in R.CONFIG_FIELDS) + (0,)  # rmcv_default_pipeline_config, the memset's zero included
    # what tests/test_gpu_pipeline.py::test_hot_contexts_config_and_switch sees of it at depth 8: off, exactly 6, out of range, ...
    for kw, want in ((dict(hot_contexts=-1), -1), (dict(hot_contexts=6), 6), (dict(hot_contexts=9), -1), (dict(depth=3), -1), (dict(host_results=2), -1), (dict(sparse_waves=8), -1), ({}, 0)):
        assert R.config(dict(dict.fromkeys(R.CONFIG_FIELDS, 0), **kw))[2] == want, kw


def test_record_layout(table):
    rows = {ints(a): ints(b) for a, b in (ln.split(":") for ln in table["L"])}
    assert set(rows) == set(itertools.product((1, 2, 3, 5, 256), (0, 1, 100)))
    for (mf, cap), g in rows.items():
        assert g == R.layout(mf, cap), (mf, cap)
        assert g[1] % 16 == 0 and g[1] >= 4 * (g[4] + 1)  # the armours start on 16 bytes, behind the report word
    assert table["S"] == [str(R.ARMOUR_BYTES)]


def test_hot_for_and_its_range_rule(table):
    rows = {ints(a): int(b) for a, b in (ln.split(":") for ln in table["H"])}
    assert set(rows) == set((hc, d) + g for hc in (-1, 0, 5) for d in (4, 8) for g in GEOMS)
    for key, g in rows.items():
        assert g == R.hot_for(*key), key
    assert [rows[(0, 8) + g] for g in GEOMS[:4]] == [4, 3, 7, 7]  # the figures quoted in the code and the GPU tests
    rules = {ints(a): b.strip() for a, b in (ln.split(":", 1) for ln in table["N"])}
    assert len(rules) == 11 * 8
    for (n, depth, hr, sw), g in rules.items():
        assert g == ((R.hot_contexts_refusal(n, depth, hr, sw) or "-") if n > 0 else "-"), (n, depth, hr, sw)


def test_report_decode_mood_and_split(table):
    rows = {ints(a): ints(b) for a, b in (ln.split(":") for ln in table["M"])}
    want = set()
    for n in (8, 48, 256):
        for dense, p16, lean in itertools.product({0, 1, n // 8, n // 8 + 1, n}, (0, 74, 75, 93, 94, 4095), (0, 1)):
            word = dense | (p16 << 20)
            assert word == R.report_word(dense, p16 * 16) == R.report_word(dense, p16 * 16 + 15)  # (the encoder floors)
            want.add((n, word, lean))
            heavy, calm = R.mood(word, lean, n)
            assert rows[(n, word, lean)] == R.report(word) + (heavy, calm, R.split_now(word, n)), (n, dense, p16, lean)
    assert set(rows) == want
    # the thresholds sit where the comments say: 1 200 points on the way back, 1 500 on the way in, more than an eighth / up to an eighth of the frames
    assert R.mood(74 << 20, 1, 48) == (False, True) and R.mood(75 << 20, 1, 48) == (True, False)
    assert R.mood(93 << 20, 0, 48) == (False, True) and R.mood(94 << 20, 0, 48) == (True, False)
    assert R.mood(6, 0, 48) == (False, False) and R.mood(7, 0, 48) == (True, False) and R.split_now(6, 48) and not R.split_now(7, 48) and not R.split_now(0, 48)


def test_front_plan(table):
    rows = {int(a): ints(b) for a, b in (ln.split(":") for ln in table["F"])}
    assert set(rows) == set(range(1 << 14))
    for b, g in rows.items():
        hot, calm, heavy, legacy, pose, ident, cont, blobs, ws, tracked, hr2, sw8, seq, k7 = ((b >> i) & 1 for i in range(14))
        stages = R.STAGE_BINARY | R.STAGE_ARMOURS | pose * R.STAGE_POSE | ident * R.STAGE_IDENTITY | cont * R.STAGE_CONTOURS | blobs * R.STAGE_BLOBS
        sw = 8 if sw8 else 4
        fast, hv, j = R.front(4 * hot, calm, heavy, 2 if hr2 else 1, sw, stages, legacy, ws, tracked, 5 * seq, 7 * k7)
        form = R.LEAN if hv else (R.SPLIT_BOTH if k7 else R.STANDARD)
        assert g == (fast, hv, j, 1 if fast else 0, 2, sw, form), (b, g)
    assert any(g[0] for g in rows.values()) and any(g[1] for g in rows.values()) and any(g[0] and g[1] for g in rows.values())


def test_back_plan(table):
    rows = {int(a): ints(b) for a, b in (ln.split(":") for ln in table["B"])}
    assert set(rows) == set(range(1 << 9))
    for b, g in rows.items():
        latency, sw8, legacy, lean, split_now, dn, cont, blobs, k5 = ((b >> i) & 1 for i in range(9))
        sw = 8 if sw8 else 4
        sparse = R.STAGE_ARMOURS | cont * R.STAGE_CONTOURS | blobs * R.STAGE_BLOBS
        w8, split, waves, first, second, stream = R.back(latency, sw, legacy, R.LEAN if lean else R.STANDARD, sw, split_now, 4 * dn, sparse, 5 * k5)
        assert g[:4] == (w8, split, waves, first) and g[5] == stream, (b, g)
        if split:
            assert g[4] == second and stream == (1 if k5 else 0), (b, g)
    assert any(g[0] for g in rows.values()) and any(g[1] for g in rows.values())


def test_ticket_place_and_the_early_rule(table):
    rows = {ints(a): ints(b) for a, b in (ln.split(":") for ln in table["T"])}
    assert set(rows) == set(pc + (t,) for pc in PLACES for t in range(140))
    for (depth, ps, ss, t), g in rows.items():
        assert g == R.place(t, depth, ps, ss), (depth, ps, ss, t)
    assert table["E"] == ["0 1 0"]  # line 682: ev_free where the context's last batch was finished on this batch's sparse stream (never a null one), else ev_done


def test_hold_back(table):
    rows = {ints(a): ints(b) for a, b in (ln.split(":") for ln in table["K"])}
    assert set(rows) == set(s + (t, b) for s in HOLD_SHAPES for t in (0, 1, 9) for b in range(32))
    for (n, w, h, t, b), g in rows.items():
        assert g == R.hold_back(b & 1, t, (b >> 1) & 1, (b >> 2) & 1, (b >> 3) & 1, (b >> 4) & 1, n, w, h), (n, w, h, t, b)  # bits: fast, was_cold, prev_live, prev_done, ws_full
    # a burst's second launch (fast, the one before was cold and is still running, k_binary_ws on every CU): the hold per shape -- 3.8 us and
    # 45.8 us of launch are below the 100 us floor, 122 us gives its quarter, 244 us and 429 us the cap
    second = 1 | 2 | 4 | 16
    assert [rows[s + (1, second)] for s in HOLD_SHAPES] == [(0, 0), (0, 0), (0, 60), (0, 60), (0, 30)]
    assert all(g == (0, 0) for (n, w, h, t, b), g in rows.items() if not b & 1)   # not in the hot rotation: never cold, never held
    assert all(g == (1, 0) for (n, w, h, t, b), g in rows.items() if b & 1 and t == 0)  # the first ticket: cold


def test_refusals(table):
    tracker = (16, 640, 512)
    cases = [R.tracked_refusal(0, 0, *tracker, 16, 640, 512, 15, False, False), R.tracked_refusal(0, 0, *tracker, 16, 640, 512, 15, True, True),
             R.tracked_refusal(1, 0, *tracker, 16, 640, 512, 15, False, False), R.tracked_refusal(0, 0, *tracker, 15, 640, 512, 15, False, False),
             R.tracked_refusal(0, 0, *tracker, 16, 641, 512, 15, False, False), R.tracked_refusal(0, 0, *tracker, 16, 640, 511, 15, False, False),
             R.tracked_refusal(0, 0, *tracker, 16, 640, 512, 7, False, False), R.tracked_refusal(0, 0, *tracker, 16, 640, 512, 15, True, False),
             R.cameras_refusal(16, 16, True), R.cameras_refusal(16, 256, True), R.cameras_refusal(16, 16, False)]
    assert [c is None for c in cases] == [True, True] + [False] * 6 + [True, False, False] and len(set(cases)) == 8
    assert table["R"] == ["%d : %s" % (i, c or "-") for i, c in enumerate(cases)]  # (the code is RMCV_ERR_BAD_ARG for every one of them: the caller's)
