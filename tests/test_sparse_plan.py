"""resolve_sparse (rmcv_amd/csrc/sparse_plan.h) against the launch table it replaced: compiled with the host C++ compiler, every input
combination is checked against the branches of launch_contours_x as they stood before the run plan (restated below)."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/sparse_plan.h"
using namespace rmcv;
static_assert(sparse_lds(LDS_FRAME, 50000) == 50000 && sparse_lds(LDS_ONE_PER_CU, 50000) == 84 * 1024 && sparse_lds(LDS_ONE_PER_CU, 90000) == 90000,
              "LDS_ONE_PER_CU: at least 84 KB, else the frame's own");
int main()
{
    for (int form = 0; form < 5; form++)
    for (int waves = 4; waves <= 8; waves += 4)
    for (int fused = 0; fused < 2; fused++)
    for (int classify = 0; classify < 2; classify++)
    for (int tier = 0; tier < 3; tier++)
    for (int mid = 0; mid < 2; mid++)
    for (int lean_rows = 0; lean_rows < 2; lean_rows++)
    for (int pixel_ws = 0; pixel_ws < 2; pixel_ws++) {
        const SparseLaunches L = resolve_sparse({(SparseForm)form, waves, fused != 0, classify != 0, tier, mid != 0, lean_rows != 0, pixel_ws != 0});
        printf("%d %d %d %d %d %d %d %d :", form, waves, fused, classify, tier, mid, lean_rows, pixel_ws);
        for (int i = 0; i < L.n; i++) printf(" %d,%d,%d", (int)L.l[i].kernel, L.l[i].flags, (int)L.l[i].lds);
        printf("\n");
    }
    return 0;
}
'''

STANDARD, LEAN, SPLIT_FIRST, SPLIT_SECOND, SPLIT_BOTH = range(5)
W8, W4, W_LEAN = range(3)
LDS_FRAME, LDS_ONE_PER_CU = range(2)


def table(form, waves, fused, classify, tier, mid, lean_rows, pixel_ws):
    """launch_contours_x before the run plan: Geom::sparse_lean and Geom::dense_defer (0 off, 1 both launches, 2 / 3 the first / second
    only) as the pipeline set them for each form; an unfused run came through launch_contours with 8 wavefronts"""
    sparse_lean, dense_defer = {STANDARD: (0, 0), LEAN: (1, 0), SPLIT_FIRST: (0, 2), SPLIT_SECOND: (0, 3), SPLIT_BOTH: (0, 1)}[form]
    if not fused:
        waves = 8
    force = tier
    lean_applies = sparse_lean and not dense_defer and tier == 0 and mid and lean_rows
    if waves == 4 and fused and not classify and lean_applies and force == 0:
        return [(W_LEAN, 2, LDS_FRAME)]
    if waves == 4:
        defer = bool(dense_defer) and (force & 3) == 0 and bool(mid)
        if dense_defer == 3 and not defer:
            return []
        out = []
        if dense_defer != 3:
            out.append((W4, force | (4 if defer else 0), LDS_ONE_PER_CU if pixel_ws else LDS_FRAME))
        if not defer or dense_defer == 2:
            return out
        out.append((W8, 2 | 8, LDS_FRAME))
        return out
    return [(W8, force, LDS_FRAME)]


def test_resolve_sparse_matches_the_launch_table(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    seen = set()
    for line in lines:
        key, launches = line.split(":")
        args = tuple(int(v) for v in key.split())
        got = [tuple(int(v) for v in l.split(",")) for l in launches.split()]
        assert got == table(*args), (args, got)
        seen.add(args)
    assert seen == set(itertools.product(range(5), (4, 8), (0, 1), (0, 1), range(3), (0, 1), (0, 1), (0, 1)))
