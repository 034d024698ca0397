"""frame_plan.h (rmcv_amd/csrc) against the code it replaced: compiled with the host C++ compiler, the adaptive copy-path rule, the chunk
bounds of the byte image's export, the result windows and the chain's parameter fill are compared with the statements as they stood in
rmcv_host.hip before the header -- upload_one, image_ready and the tail of extract_color_body; k_image_export / image_chunk; the nine
std::min(SF_*_WIN, limit); enqueue_blobs, enqueue_armours and the fused_ahead branch -- restated below."""
import itertools
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <string.h>
#include "rmcv_amd/csrc/frame_plan.h"
using namespace rmcv;
static void print_params(const char* tag, const rmcv_params& p)
{
    printf("%s %d %d %d %.9g %.9g %.9g %.17g %.17g %.9g %.9g %.9g %d\n", tag, p.camp, p.lower_bound, p.morph, p.tilt_max, p.ratio_lo, p.ratio_hi,
           p.area_lo, p.area_hi, p.angle_diff_max, p.shear_max, p.length_ratio_max, p._pad);
}
int main(int argc, char** argv)
{
    if (argc > 1) { // the copy path: one line per frame -- "R dir" resets a direction (its option was set), "F dir option binary_out forced us bytes" is a frame
        FILE* f = fopen(argv[1], "r");
        if (!f) return 1;
        CopyPathState st[2] = {{0, 0}, {0, 0}};
        const CopyDirection* dir[2] = {&COPY_UPLOAD, &COPY_IMAGE};
        char kind;
        while (fscanf(f, " %c", &kind) == 1) {
            int d, option, binary_out, forced;
            double us, bytes;
            if (kind == 'R') {
                if (fscanf(f, "%d", &d) != 1) return 1;
                st[d] = {};
                continue;
            }
            if (fscanf(f, "%d %d %d %d %lf %lf", &d, &option, &binary_out, &forced, &us, &bytes) != 6) return 1;
            int path = copy_path(*dir[d], option, st[d]);
            const int wanted = path;
            if (forced) path = 0; // (no mapped pinned memory to be had: the image takes the runtime's copy whatever the rule says)
            if (binary_out) st[d] = copy_path_step(*dir[d], option, st[d], path, us, bytes);
            printf("%d %d %d %d\n", wanted, path, st[d].slow, st[d].hold);
        }
        fclose(f);
        return 0;
    }
    const long long sizes[8] = {0, 1, 15, 16, 17, 333 * 77, 1280 * 1024, 1920 * 1200};
    for (int s = 0; s < 8; s++)
        for (int n = 1; n <= 16; n++)
            for (int g = 0; g < n; g++) {
                const ImageChunk k = image_chunk(sizes[s], n, g);
                const ImageChunk k2 = image_chunk_at(sizes[s], image_chunk_bytes(sizes[s], n), g); // (the two steps k_image_export takes)
                if (k.lo != k2.lo || k.hi != k2.hi) return 2;
                printf("C %lld %d %d %lld %lld\n", sizes[s], n, g, k.lo, k.hi);
            }
    printf("K %d %d %d\n", IMG_CHUNKS, IMG_CHUNKS_DEFAULT, IMG_GROUPS);
    const int lims[5][3] = {{1023, 1024, 1025}, {8191, 8192, 8193}, {63, 64, 65}, {1023, 1024, 1025}, {31, 32, 33}}; // below, at, above each window
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 3; c++) for (int d = 0; d < 3; d++) {
        const int mc = lims[0][a], mp = lims[1][b], mb = lims[2][c], ma = lims[4][d];
        const FrameWindows w = frame_windows(mc, mp, mb, ma);
        printf("W %d %d %d %d : %d %d %d %d %d\n", mc, mp, mb, ma, w.offs, w.pts, w.blobs, w.neg, w.armours);
    }
    {
        const FrameWindows w = frame_windows(1, 1, 1, 1), d = frame_windows(2048, 65536, 256, 256); // the smallest context; rmcv_default_limits
        printf("W 1 1 1 1 : %d %d %d %d %d\n", w.offs, w.pts, w.blobs, w.neg, w.armours);
        printf("W 2048 65536 256 256 : %d %d %d %d %d\n", d.offs, d.pts, d.blobs, d.neg, d.armours);
    }
    // the parameter fill, onto the defaults (rmcv_default_params' literals) and onto a pattern no default has
    const LbParams lb = {61.5f, 1.25f, 77.0f, 12.5, 88888.0, 1};
    const ArParams ar = {13.5f, 21.0f, 0.375f, 2}, ar_same = {13.5f, 21.0f, 0.375f, 1};
    for (int base = 0; base < 2; base++) {
        rmcv_params d;
        memset(&d, 0, sizeof(d));
        if (base == 0) {
            d.camp = RMCV_CAMP_BLUE; d.lower_bound = 80; d.morph = RMCV_MORPH_CLOSE; d.tilt_max = 70.0f; d.ratio_lo = 1.5f; d.ratio_hi = 80.0f;
            d.area_lo = 10.0; d.area_hi = 99999.0; d.angle_diff_max = 12.0f; d.shear_max = 22.0f; d.length_ratio_max = 0.4f;
        } else {
            d.camp = -7; d.lower_bound = -8; d.morph = -9; d.tilt_max = -1.0f; d.ratio_lo = -2.0f; d.ratio_hi = -3.0f;
            d.area_lo = -4.0; d.area_hi = -5.0; d.angle_diff_max = -6.0f; d.shear_max = -7.0f; d.length_ratio_max = -8.0f; d._pad = -10;
        }
        rmcv_params p = d;
        print_params(base ? "P1 base" : "P0 base", p);
        chain_params(&p, &lb, nullptr);
        print_params(base ? "P1 lb" : "P0 lb", p);
        p = d;
        chain_params(&p, nullptr, &ar);
        print_params(base ? "P1 ar" : "P0 ar", p);
        p = d;
        chain_params(&p, &lb, &ar_same);
        print_params(base ? "P1 both" : "P0 both", p);
        p = d;
        chain_params(&p, nullptr, nullptr);
        print_params(base ? "P1 none" : "P0 none", p);
    }
    printf("S %zu %zu\n", sizeof(LbParams), sizeof(ArParams));
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_plan")
    src = d / "frame_plan.cpp"
    src.write_text(SRC)
    out = d / "frame_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def table(exe):
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


# ---- the copy path: the statements of the parent, one object per context ----
UPLOAD, IMAGE = 0, 1
ADAPTIVE = {UPLOAD: 3, IMAGE: 2}
OPTIONS = {UPLOAD: (0, 1, 2, 3), IMAGE: (0, 1, 2)}


def threshold_us(d, nbytes):
    """what a frame's copy may cost before it counts as slow (extract_color_body's tail)"""
    return nbytes / 45e3 + 100.0 if d == UPLOAD else nbytes / 40e3 + 60.0


class Parent:
    """upload_one:  mode = frame_upload == 3 ? (hold_upload > 0 ? 1 : 0) : frame_upload
    image_ready: false unless image_export == 1 || (image_export == 2 && hold_image > 0); false too when mapped memory is not to be had
    the tail of extract_color_body, under `if (binary_out)`:
        if (now == 0) { slow = us > bytes / A + B ? slow + 1 : 0;  if (option == adaptive && slow >= 3) { hold = 512; slow = 0; } }
        else if (hold > 0) hold--;
    rmcv_ctx_set_option of the direction's option: slow = hold = 0"""

    def __init__(self):
        self.slow, self.hold = [0, 0], [0, 0]

    def reset(self, d):
        self.slow[d] = self.hold[d] = 0

    def frame(self, d, option, binary_out, forced, us, nbytes):
        if d == UPLOAD:
            wanted = (1 if self.hold[d] > 0 else 0) if option == 3 else option
        else:
            wanted = 1 if (option == 1 or (option == 2 and self.hold[d] > 0)) else 0
        now = 0 if forced else wanted
        if binary_out:
            if now == 0:
                self.slow[d] = self.slow[d] + 1 if us > threshold_us(d, nbytes) else 0
                if option == ADAPTIVE[d] and self.slow[d] >= 3:
                    self.hold[d], self.slow[d] = 512, 0
            elif self.hold[d] > 0:
                self.hold[d] -= 1
        return wanted, now, self.slow[d], self.hold[d]


def run_script(exe, tmp_path, script):
    """script: ("R", d) or ("F", d, option, binary_out, forced, us, bytes); returns the header's (wanted, path, slow, hold) per frame"""
    f = tmp_path / "script.txt"
    f.write_text("".join(("R %d\n" % s[1]) if s[0] == "R" else ("F %d %d %d %d %r %r\n" % s[1:]) for s in script))
    out = subprocess.run([exe, str(f)], check=True, capture_output=True, text=True).stdout.splitlines()
    return [tuple(int(v) for v in ln.split()) for ln in out]


def moved_bytes(d):
    """what each direction moves at the issue's frame sizes: BGR, 1- and 2-byte mosaics up; one byte per pixel down"""
    sizes = ((64, 48), (1280, 1024), (1920, 1200))
    return [float(bpp * w * h) for (w, h) in sizes for bpp in ((3, 1, 2) if d == UPLOAD else (1,))]


def test_copy_path_matches_the_parents_statements(exe, tmp_path):
    script, want, checks = [], [], []
    for d in (UPLOAD, IMAGE):
        for option, nbytes in itertools.product(OPTIONS[d], moved_bytes(d)):
            thr = threshold_us(d, nbytes)
            fast, at, slow = thr - 1.0, thr, thr + 1.0
            assert fast < thr < slow
            par = Parent()
            script.append(("R", d))

            def frames(us_list, binary_out=1, forced=0):
                got = []
                for us in us_list:
                    script.append(("F", d, option, binary_out, forced, us, nbytes))
                    want.append(par.frame(d, option, binary_out, forced, us, nbytes))
                    got.append(len(want) - 1)
                return got

            adaptive = option == ADAPTIVE[d]
            lib_path = option not in (0, ADAPTIVE[d])  # a fixed value that IS the library's own path
            # two slow frames and a fast one (then: the exact threshold is not slow) reset the count
            i = frames([slow, slow, fast])
            checks.append((i[1], "slow", 0 if lib_path else 2))
            checks.append((i[2], "slow", 0))
            i = frames([slow, slow, at])
            checks.append((i[2], "slow", 0))
            # frames without binary_out leave the state alone, however slow
            i = frames([slow, slow])
            j = frames([slow] * 5, binary_out=0)
            for k in j:
                checks.append((k, "state", want[i[1]][2:]))
            # the third slow frame in a row: the adaptive value switches and holds for exactly 512 frames, a fixed value never does
            i = frames([slow])
            checks.append((i[0], "state", (0, 512) if adaptive else (0, 0) if lib_path else (3, 0)))
            held = frames([slow] * 512)  # (slow or not: the library's own path is not measured against the threshold)
            for n, k in enumerate(held):
                checks.append((k, "path", 1 if adaptive else option))
                if adaptive:
                    checks.append((k, "state", (0, 511 - n)))
            i = frames([fast])           # ... after which the runtime's path is tried again
            checks.append((i[0], "path", 0 if adaptive else option))
            # a set-option reset in the middle of a hold, and in the middle of a count, clears the state
            frames([slow, slow, slow, slow])
            script.append(("R", d))
            par.reset(d)
            i = frames([fast])
            checks.append((i[0], "path", 0 if adaptive else option))
            checks.append((i[0], "state", (0, 0)))
            frames([slow, slow])
            script.append(("R", d))
            par.reset(d)
            i = frames([slow])
            checks.append((i[0], "slow", 0 if lib_path else 1))
            if d == IMAGE:
                # holding, but mapped memory is not to be had: the runtime's copy is taken, slow frames are counted, the hold does not run down
                frames([slow, slow, slow])
                i = frames([slow, slow, fast, slow], forced=1)
                for k in i:
                    checks.append((k, "path", 0))
                if adaptive:
                    checks.append((i[1], "state", (2, 511)))
                    checks.append((i[3], "state", (1, 511)))
                i = frames([slow, slow, slow], forced=1)
                if adaptive:
                    checks.append((i[1], "state", (0, 512)))  # (three in a row with the one before: held afresh)
                    checks.append((i[2], "state", (1, 512)))
    got = run_script(exe, tmp_path, script)
    assert len(got) == len(want) > 20000
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n, g, w)
    # ... and the parent's statements say what the issue says of them
    for k, what, value in checks:
        wanted, path, slow, hold = want[k]
        have = {"slow": slow, "path": path, "state": (slow, hold)}[what]
        assert have == value, (k, what, have, value)


# ---- the chunks ----
SIZES = (0, 1, 15, 16, 17, 333 * 77, 1280 * 1024, 1920 * 1200)


def parent_chunk(nbytes, n_chunks, g):
    """k_image_export and image_chunk, both:  per = ((bytes + n - 1) / n + 15) & ~15;  lo = min(g * per, bytes);  hi = min(lo + per, bytes)"""
    per = ((nbytes + n_chunks - 1) // n_chunks + 15) & ~15
    lo = min(g * per, nbytes)
    return lo, min(lo + per, nbytes)


def test_chunks_tile_the_image_on_16_byte_bounds(table):
    got = {}
    for ln in table:
        if ln.startswith("C "):
            nbytes, n, g, lo, hi = (int(v) for v in ln.split()[1:])
            got[(nbytes, n, g)] = (lo, hi)
    assert set(got) == {(b, n, g) for b in SIZES for n in range(1, 17) for g in range(n)}
    for nbytes in SIZES:
        for n in range(1, 17):
            at = 0
            for g in range(n):
                lo, hi = got[(nbytes, n, g)]
                assert (lo, hi) == parent_chunk(nbytes, n, g), (nbytes, n, g)
                assert lo == at and hi >= lo, (nbytes, n, g, lo, hi, at)  # in order, no gap, no overlap
                if hi > lo:
                    assert lo % 16 == 0, (nbytes, n, g, lo)
                at = hi
            assert at == nbytes, (nbytes, n, at)
    assert "K 16 8 16" in table  # IMG_CHUNKS (the flags' capacity), IMG_CHUNKS_DEFAULT, IMG_GROUPS


# ---- the windows ----
def test_windows_are_the_limits_clamped(table):
    rows = [ln for ln in table if ln.startswith("W ")]
    assert len(rows) == 81 + 2
    for ln in rows:
        lim, win = ln[2:].split(":")
        mc, mp, mb, ma = (int(v) for v in lim.split())
        # offsets, points, blobs, negatives, armours: std::min(SF_*_WIN, c->lim.max_*) as the parent wrote it at every use
        assert tuple(int(v) for v in win.split()) == (min(1024, mc), min(8192, mp), min(64, mb), min(1024, mc), min(32, ma)), ln


# ---- the parameters ----
FIELDS = ("camp", "lower_bound", "morph", "tilt_max", "ratio_lo", "ratio_hi", "area_lo", "area_hi", "angle_diff_max", "shear_max", "length_ratio_max", "_pad")
DEFAULTS = dict(camp=0, lower_bound=80, morph=None, tilt_max=70.0, ratio_lo=1.5, ratio_hi=80.0, area_lo=10.0, area_hi=99999.0, angle_diff_max=12.0,
                shear_max=22.0, length_ratio_max=0.4, _pad=0)  # rmcv_default_params (camp, morph: read from the header below)
PATTERN = dict(camp=-7, lower_bound=-8, morph=-9, tilt_max=-1.0, ratio_lo=-2.0, ratio_hi=-3.0, area_lo=-4.0, area_hi=-5.0, angle_diff_max=-6.0, shear_max=-7.0,
               length_ratio_max=-8.0, _pad=-10)
LB = dict(tilt_max=61.5, ratio_lo=1.25, ratio_hi=77.0, area_lo=12.5, area_hi=88888.0, enemy=1)
AR = dict(angle_diff_max=13.5, shear_max=21.0, length_ratio_max=0.375, enemy=2)


def parent_fill(base, lb, ar):
    """enqueue_blobs (lb alone), enqueue_armours (ar alone) and the fused_ahead branch (both; it runs only when the two enemies agree)"""
    p = dict(base)
    if lb and ar:
        for k in ("tilt_max", "ratio_lo", "ratio_hi", "area_lo", "area_hi"):
            p[k] = lb[k]
        p["camp"] = lb["enemy"]
        for k in ("angle_diff_max", "shear_max", "length_ratio_max"):
            p[k] = ar[k]
    elif lb:
        for k in ("tilt_max", "ratio_lo", "ratio_hi", "area_lo", "area_hi"):
            p[k] = lb[k]
        p["camp"] = lb["enemy"]
    elif ar:
        for k in ("angle_diff_max", "shear_max", "length_ratio_max"):
            p[k] = ar[k]
        p["camp"] = ar["enemy"]
    return p


def test_parameter_fill_matches_the_parents(table):
    hdr = open(os.path.join(ROOT, "include", "rmcv_abi.h")).read()
    defaults = dict(DEFAULTS)
    defaults["camp"] = int(re.search(r"RMCV_CAMP_BLUE\s*=?\s*(-?\d+)", hdr).group(1))
    defaults["morph"] = int(re.search(r"RMCV_MORPH_CLOSE\s*=?\s*(-?\d+)", hdr).group(1))
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    rows = {}
    for ln in table:
        if ln[0] == "P":
            tag, which, *vals = ln.split()
            rows[(tag, which)] = dict(zip(FIELDS, (float(v) for v in vals)))
    assert len(rows) == 10
    for tag, base in (("P0", defaults), ("P1", PATTERN)):
        for which, lb, ar in (("base", None, None), ("none", None, None), ("lb", LB, None), ("ar", None, AR), ("both", LB, dict(AR, enemy=LB["enemy"]))):
            want = parent_fill(base, lb, ar)
            for k in FIELDS:
                got, w = rows[(tag, which)][k], want[k]
                if k not in ("area_lo", "area_hi") and not isinstance(w, int):
                    got, w = f32(got), f32(w)  # (a float field: nine digits name it)
                assert got == w, (tag, which, k, got, w)
    # what rmcv_filter_lightblobs / rmcv_filter_armours compare with memcmp keeps its layout
    assert "S 40 16" in table
