"""pixel_plan.h (rmcv_amd/csrc) against the code it replaced: compiled with the host C++ compiler, the launch shape, every chunk's launch
values, ws_full, the variant table and the refusals are compared with the arithmetic and the ladders as they stood before the plan --
K1_LAUNCH_T of k_binary_launch.inc, binary_ws_full and launch_binary of k_binary.hip, the name ladders of run_stages and of the pipeline's
submit, and the eight refusal sites -- restated below."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BGR, BAYER, ENH, WIN, CAMP, CAMP_WIN = range(6)

# the full product of the geometry axes under a few option sets, and the full product of the options at the geometries on an edge
VARIANTS = (BGR, BAYER, ENH, WIN, CAMP, CAMP_WIN)
PIXEL_WS = (0, 1)
GROUPS = (0, 1, 2, 4)
N_CU = (0, 8, 256)
ROWQUAD = (0, 1)
LOWER_BOUND = (-1, 0, 1, 100, 256, 300)
W = (16, 64, 100, 1280, 4672, 4736, 6848)
H = (1, 31, 32, 33, 1024)
STRIDE = (0, 1, 2)       # 3w; 3w rounded up to 16 plus 16; 3w + 1
BASE_ALIGNED = (1, 0)
N_FRAMES = (1, 4, 5, 7, 8, 128, 129, 256, 1092, 1093, 2200)
EDGES = ((1280, 1024, 0, 1, 4), (1280, 1024, 0, 1, 5), (1280, 1024, 0, 1, 7), (1280, 1024, 0, 1, 8), (1280, 32, 0, 1, 128), (1280, 32, 0, 1, 129),
         (1280, 1024, 0, 1, 1092), (1280, 1024, 0, 1, 1093), (1280, 1024, 0, 1, 2200), (4672, 33, 0, 1, 256), (4736, 33, 0, 1, 256),
         (6848, 31, 0, 1, 8), (100, 33, 0, 1, 7), (64, 1, 1, 1, 256), (1280, 1024, 1, 1, 8), (1280, 1024, 0, 0, 8), (16, 32, 2, 1, 1))


def points():
    """(variant, pixel_ws, pixel_groups, n_cu, pixel_rowquad, lower_bound, w, h, stride kind, base aligned, n_frames)"""
    seen = set()
    for v, ws, ncu, w, h, sk, al, n in itertools.product(VARIANTS, PIXEL_WS, N_CU, W, H, STRIDE, BASE_ALIGNED, N_FRAMES):
        seen.add((v, ws, 2, ncu, 0, 100, w, h, sk, al, n))
    for v, ws, grp, ncu, rq, lb, (w, h, sk, al, n) in itertools.product(VARIANTS, PIXEL_WS, GROUPS, N_CU, ROWQUAD, LOWER_BOUND, EDGES):
        seen.add((v, ws, grp, ncu, rq, lb, w, h, sk, al, n))
    return sorted(seen)


def geometry(w, h, sk):
    stride = (3 * w, ((3 * w + 15) & ~15) + 16, 3 * w + 1)[sk]
    ww = (w + 63) // 64
    return stride, stride * h, ww, (h + 2) * (ww + 2)  # stride, frame_pitch, ww, plane_pitch (set_extent)


SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/pixel_plan.h"
using namespace rmcv;
int main(int argc, char** argv)
{
    if (argc > 1) { // the shape of every point of the file
        FILE* f = fopen(argv[1], "r");
        if (!f) return 1;
        int v, ws, grp, ncu, rq, lb, w, h, stride, al, n, ww;
        long long fp, pp;
        while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %lld %d %lld", &v, &ws, &grp, &ncu, &rq, &lb, &w, &h, &stride, &al, &n, &fp, &ww, &pp) == 14) {
            const PixelShape s = pixel_shape({(PixelVariant)v, n, w, h, ww, stride, fp, pp, ncu, rq, al != 0, lb, ws, grp});
            printf("%d %d %d %d %d %zu %zu %d :", s.strips, s.lb, s.all_pass, s.chunk, s.mode, s.planes, s.planes_ws, (int)s.ws_full);
            for (int f0 = 0; f0 < n; f0 += s.chunk) {
                const int nf = s.chunk < n - f0 ? s.chunk : n - f0;
                const PixelChunk c = pixel_chunk(s, nf);
                printf(" %d,%d,%d,%d,%d,%d,%d", nf, c.n_blocks, c.grid, c.taper_head, c.taper_tail, (int)c.ws, c.grid_ws);
            }
            printf("\n");
        }
        fclose(f);
        return 0;
    }
    for (int fmt = 0; fmt < 5; fmt++)
    for (int enh = 0; enh < 2; enh++)
    for (int win = 0; win < 2; win++)
    for (int keys = 0; keys < 2; keys++) {
        const PixelVariant v = pixel_variant(fmt, enh, win, keys);
        printf("V %d %d %d %d|%d|%s|%s|%d\n", fmt, enh, win, keys, (int)v, PIXEL_VARIANTS[v].kernel, PIXEL_VARIANTS[v].step, (int)PIXEL_VARIANTS[v].ws);
        for (int legacy = 0; legacy < 2; legacy++) {
            const char* why = pixel_refusal(fmt, enh, win != 0, keys != 0, legacy != 0);
            printf("R %d %d %d %d %d|%s\n", fmt, enh, win, keys, legacy, why ? why : "");
        }
    }
    for (int camp = -2; camp < 5; camp++)
    for (int lb = -1; lb < 260; lb++) {
        const FrameKey k = frame_key_eff(camp, lb);
        const int pair = with_channel_pair(k, [](auto ca, auto cb) { return 10 * decltype(ca)::value + decltype(cb)::value; });
        printf("K %d %d|%d %d %d %d %d\n", camp, lb, k.ca, k.cb, k.lb, k.all_pass, pair);
    }
    return 0;
}
'''

SR = 32
LIM = 0xFFFFF000


def parent_launch(v, pixel_ws, bpc, n_cu, rowquad, lower_bound, w, h, stride, base_aligned, n_frames, frame_pitch, ww, plane_pitch):
    """K1_LAUNCH_T as it stood (k_binary_launch.inc), under the macros of the variant's translation unit: K1_WIN no linear loader; the
    k_binary_ws branch in k_binary.hip alone; launch_binary_camp / _camp_win pass lower_bound 0"""
    k1_win, k1_plain = v in (WIN, CAMP_WIN), v == BGR
    if v in (CAMP, CAMP_WIN):
        lower_bound = 0
    strips = (h + SR - 1) // SR
    lb, all_pass = lower_bound, 0
    if lb <= 0:
        all_pass, lb = 1, 1
    if lb > 256:
        lb = 256
    planes = 2 * (SR + 4) * ww * 8
    aligned = w % 64 == 0 and stride % 16 == 0 and frame_pitch % 16 == 0 and bool(base_aligned)
    per_frame = max(max(frame_pitch, plane_pitch * 8), w * h)
    chunk = min(n_frames, max(1, (LIM - 1) // per_frame)) if aligned else n_frames
    fast = aligned and chunk * per_frame < LIM
    linear = False if k1_win else (fast and not rowquad and stride == 3 * w)
    mode = (2 if linear else 1) if fast else 0
    planes_ws = (2 * (SR + 4) + SR) * ww * 8
    chunks, all_ws = [], True
    for f0 in range(0, n_frames, chunk):
        nf = min(chunk, n_frames - f0)
        n_blocks = nf * strips
        grid = (n_cu if n_cu > 0 else 256) * (bpc if bpc > 0 else 4)
        if grid > ((n_blocks + 7) & ~7):
            grid = (n_blocks + 7) & ~7
        grid = (grid + 7) & ~7
        per_xcd = (n_blocks + 7) >> 3
        taper_head = taper_tail = 0
        if n_blocks * 2 <= (n_cu if n_cu > 0 else 256):
            taper_head, taper_tail, grid = per_xcd, 0, (4 * n_blocks + 7) & ~7
        ws, grid_ws = False, None
        if k1_plain and pixel_ws and linear and not all_pass and taper_head == 0 and planes_ws <= 60 * 1024:
            ws = True
            grid_ws = ((n_cu if n_cu > 0 else 256) + 7) & ~7
            if grid_ws > ((n_blocks + 7) & ~7):
                grid_ws = (n_blocks + 7) & ~7
        else:
            all_ws = False
        chunks.append((nf, n_blocks, grid, taper_head, taper_tail, ws, grid_ws))
    return (strips, lb, all_pass, chunk, mode, planes, planes_ws), chunks, all_ws


def parent_ws_full(v, pixel_ws, n_cu, rowquad, lower_bound, w, h, stride, base_aligned, n_frames, frame_pitch, ww, plane_pitch):
    """binary_ws_full as it stood (k_binary.hip)"""
    strips = (h + SR - 1) // SR
    aligned = w % 64 == 0 and stride % 16 == 0 and frame_pitch % 16 == 0 and bool(base_aligned)
    per_frame = max(max(frame_pitch, plane_pitch * 8), w * h)
    one_launch = aligned and n_frames * per_frame < LIM
    linear = one_launch and not rowquad and stride == 3 * w
    n_cu = n_cu if n_cu > 0 else 256
    n_blocks = n_frames * strips
    planes_ws = (2 * (SR + 4) + SR) * ww * 8
    return bool(v == BGR and pixel_ws and linear and lower_bound > 0 and n_blocks * 2 > n_cu and planes_ws <= 60 * 1024 and n_blocks >= n_cu)


def build(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    return exe


def test_the_grid_holds_every_edge():
    pts = points()
    for axis, want in enumerate((VARIANTS, PIXEL_WS, GROUPS, N_CU, ROWQUAD, LOWER_BOUND, W, H, STRIDE, BASE_ALIGNED, N_FRAMES)):
        assert {p[axis] for p in pts} == set(want)
    assert {p[6:] for p in pts} == set(itertools.product(W, H, STRIDE, BASE_ALIGNED, N_FRAMES))  # every geometry ...
    assert {p[:6] for p in pts} == set(itertools.product(VARIANTS, PIXEL_WS, GROUPS, N_CU, ROWQUAD, LOWER_BOUND))  # ... and every option set
    # the edges the sizes were chosen for, on 256 CUs
    def launch(w, h, n, v=BGR, ws=1):
        stride, fp, ww, pp = geometry(w, h, 0)
        return parent_launch(v, ws, 2, 256, 0, 100, w, h, stride, 1, n, fp, ww, pp), parent_ws_full(v, ws, 256, 0, 100, w, h, stride, 1, n, fp, ww, pp)
    assert launch(1280, 1024, 4)[0][1][0][3] > 0 and launch(1280, 1024, 5)[0][1][0][3] == 0    # the taper
    assert launch(1280, 32, 128)[0][1][0][3] > 0 and launch(1280, 32, 129)[0][1][0][3] == 0
    assert launch(1280, 1024, 7) == (launch(1280, 1024, 7)[0], False) and launch(1280, 1024, 7)[0][2] and launch(1280, 1024, 8)[1]  # ws, not on every CU
    assert len(launch(1280, 1024, 1092)[0][1]) == 1 and len(launch(1280, 1024, 1093)[0][1]) == 2   # 4 GiB
    assert [c[0] for c in launch(1280, 1024, 2200)[0][1]] == [1092, 1092, 16]
    assert launch(4672, 33, 256)[0][2] and not launch(4736, 33, 256)[0][2]                             # planes_ws <= 60 KiB
    assert launch(4736, 33, 256)[0][0][5] <= 60 * 1024 < launch(6848, 31, 8)[0][0][5]                 # planes > 60 KiB


def test_shape_and_chunks_match_the_launcher_they_replaced(tmp_path):
    exe = build(tmp_path)
    pts = points()
    rows = []
    for v, ws, grp, ncu, rq, lb, w, h, sk, al, n in pts:
        stride, fp, ww, pp = geometry(w, h, sk)
        rows.append((v, ws, grp, ncu, rq, lb, w, h, stride, al, n, fp, ww, pp))
    inp = tmp_path / "points.txt"
    inp.write_text("".join(" ".join(str(x) for x in r) + "\n" for r in rows))
    lines = subprocess.run([str(exe), str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(rows)
    for r, line in zip(rows, lines):
        v, ws, grp, ncu, rq, lb, w, h, stride, al, n, fp, ww, pp = r
        head, tail = line.split(":")
        head = [int(x) for x in head.split()]
        got_chunks = [tuple(int(x) for x in c.split(",")) for c in tail.split()]
        assert head[7] == parent_ws_full(v, ws, ncu, rq, lb, w, h, stride, al, n, fp, ww, pp), (r, line)
        if v == BAYER:  # (its launcher is its own: k_binary_bayer.hip takes nothing of the shape; ws_full alone is asked of such a batch)
            assert not any(c[5] for c in got_chunks), r
            continue
        shape, chunks, all_ws = parent_launch(v, ws, grp, ncu, rq, lb, w, h, stride, al, n, fp, ww, pp)
        assert tuple(head[:7]) == shape, (r, line)
        assert len(got_chunks) == len(chunks), (r, line)
        for g, c in zip(got_chunks, chunks):
            assert g[:5] == c[:5] and bool(g[5]) == c[5], (r, line)
            if c[5]:
                assert g[6] == c[6], (r, line)
        assert all(bool(g[5]) for g in got_chunks) == all_ws, (r, line)  # what image_step is told: IMAGE_KERNEL_WS or _OTHER


LEGACY_BAYER = "the legacy matcher votes camps from BGR means: not for Bayer frames (RMCV_OPT_INPUT_FORMAT)"
LEGACY_ENH = "the legacy matcher votes camps from BGR means: not with RMCV_OPT_ENHANCE"
LEGACY_CAMPS = "the legacy matcher votes a camp per blob from BGR means: not with per-frame camps (rmcv_batch_set_frame_camps)"
CAMPS_BAYER = "per-frame camps with a Bayer input format (RMCV_OPT_INPUT_FORMAT): the mosaic kernel takes one camp per run; not supported"
CAMPS_ENH = "per-frame camps with RMCV_OPT_ENHANCE: the threshold table folds one lower bound per run; not supported"
ENH_BAYER = "RMCV_OPT_ENHANCE with a Bayer input format: the mean of a demosaiced frame is not a function of the mosaic's sums"
WIN_BAYER = "windows with a Bayer input format (RMCV_OPT_INPUT_FORMAT): crop-then-demosaic has other border semantics; not supported"
WIN_ENH = "windows with RMCV_OPT_ENHANCE: the mean of a crop is not the frame's; not supported"


def first(*checks):
    for cond, msg in checks:
        if cond:
            return msg
    return ""


# the refusal sites as they stood: site -> (the calls it makes now, as (windows, keys, legacy) of its own (win, keys); its ladder as it stood)
SITES = {
    "set_geom": (lambda w, k: [(0, 0, 0)] + ([(1, 0, 0)] if w else []), lambda f, e, w, k: first((e and f, ENH_BAYER), (w and f, WIN_BAYER), (w and e, WIN_ENH))),
    "check_windows": (lambda w, k: [(1, 0, 0)], lambda f, e, w, k: first((f, WIN_BAYER), (e, WIN_ENH))),
    "check_frame_camps, ctx_check_frame_camps": (lambda w, k: [(0, 1, 0)], lambda f, e, w, k: first((f, CAMPS_BAYER), (e, CAMPS_ENH))),
    "run_stages, rmcv_batch_run_legacy": (lambda w, k: [(0, k, 1)], lambda f, e, w, k: first((f, LEGACY_BAYER), (e, LEGACY_ENH), (k, LEGACY_CAMPS))),
    "rmcv_find_lightblobs": (lambda w, k: [(0, 0, 1)], lambda f, e, w, k: first((f, LEGACY_BAYER), (e, LEGACY_ENH))),
    "submit, with legacy params (never with camps)": (lambda w, k: [(0, 0, 1)], lambda f, e, w, k: first((f, LEGACY_BAYER), (e, LEGACY_ENH))),
    "submit, with camps": (lambda w, k: [(0, 1, 0)], lambda f, e, w, k: first((f, CAMPS_BAYER), (e, CAMPS_ENH))),
}


def test_variants_and_refusals_match_the_ladders_they_replaced(tmp_path):
    exe = build(tmp_path)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    variants, refusals, keys_seen = {}, {}, 0
    for line in lines:
        kind, rest = line[0], line[2:]
        if kind == "V":
            key, v, kernel, step, ws = rest.split("|")
            variants[tuple(int(x) for x in key.split())] = (int(v), kernel, step, int(ws))
        elif kind == "R":
            key, why = rest.split("|")
            refusals[tuple(int(x) for x in key.split())] = why
        else:
            key, val = rest.split("|")
            camp, lb = (int(x) for x in key.split())
            # launch_binary's ladder (GUIDELIGHT 2: <1, 2>; BLUE 1: <0, 2>; everything else <2, 0>) and K1_LAUNCH_T's clamp
            ca, cb = (1, 2) if camp == 2 else (0, 2) if camp == 1 else (2, 0)
            assert [int(x) for x in val.split()] == [ca, cb, 1 if lb <= 0 else min(lb, 256), int(lb <= 0), 10 * ca + cb], line
            keys_seen += 1
    assert keys_seen == 7 * 261
    assert set(variants) == set(itertools.product(range(5), (0, 1), (0, 1), (0, 1)))
    assert set(refusals) == set(itertools.product(range(5), (0, 1), (0, 1), (0, 1), (0, 1)))
    for (f, e, w, k), (v, kernel, step, ws) in variants.items():
        # launch_binary's ladder, run_stages' names, the pipeline's last_what, binary_ws_full's first four terms
        want = BAYER if f else ENH if e else (CAMP_WIN if w else CAMP) if k else WIN if w else BGR
        assert v == want
        assert kernel == ("k_binary_bayer" if f else ("k_binary_enh" if e else (("k_binary_camp_win" if w else "k_binary_camp") if k else ("k_binary_win" if w else "k_binary"))))
        assert step == ("the pixel kernel (k_binary_bayer)" if f else "k_frame_sums, k_enhance_table, the pixel kernel (k_binary_enh)" if e
                        else "k_frame_keys, the pixel kernel (k_binary_camp / k_binary_camp_win)" if k else "k_window_origins, the pixel kernel (k_binary_win)" if w
                        else "the pixel kernel (k_binary / k_binary_ws)")
        assert ws == int(f == 0 and not e and not w and not k)
    for site, (passes, ladder) in SITES.items():
        for f, e, w, k in itertools.product(range(5), (0, 1), (0, 1), (0, 1)):
            got = first(*((True, refusals[(f, e) + call]) for call in passes(w, k) if refusals[(f, e) + call]))
            assert got == ladder(f, e, w, k), (site, f, e, w, k)
    # and whatever a caller passes: the legacy matcher's first, then the keys', the windows', the options against each other; the format
    # before the enhancement in each
    for (f, e, w, k, l), why in refusals.items():
        assert why == first((l and f, LEGACY_BAYER), (l and e, LEGACY_ENH), (l and k, LEGACY_CAMPS), (k and f, CAMPS_BAYER), (k and e, CAMPS_ENH),
                            (w and f, WIN_BAYER), (w and e, WIN_ENH), (f and e, ENH_BAYER)), (f, e, w, k, l)
