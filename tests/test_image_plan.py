"""image_step (rmcv_amd/csrc/image_plan.h): how a pixel launch may store the 0/255 byte image given what the context knows about it, and
what the context knows afterwards.  Compiled with the host C++ compiler; every combination of (state, kernel, image wanted, geometry
same or changed, frames against the frames the mask covers, ww <= 32 or not, launch enqueued or failed) is checked against the table
written out below."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include "rmcv_amd/csrc/image_plan.h"
using namespace rmcv;
int main()
{
    const int geo[3][3] = {{1280, 70, 20}, {192, 70, 3}, {2112, 40, 33}}; // w, h, ww
    const int frames[3] = {24, 48, 60};
    for (int tracked = 0; tracked < 2; tracked++)
    for (int sg = 0; sg < 3; sg++)      // geometry of the state (ignored when not tracked)
    for (int sh = 0; sh < 2; sh++)      // ... with another height
    for (int kernel = 0; kernel < 2; kernel++)
    for (int image = 0; image < 2; image++)
    for (int lg = 0; lg < 3; lg++)
    for (int lf = 0; lf < 3; lf++)
    for (int ok = 0; ok < 2; ok++) {
        const ImageState st = tracked ? ImageState{IMAGE_TRACKED, geo[sg][0], geo[sg][1] + sh, 48} : IMAGE_STATE_UNKNOWN;
        const ImageStep r = image_step(st, {(ImageKernel)kernel, image != 0, geo[lg][0], geo[lg][1], geo[lg][2], frames[lf]}, ok != 0);
        printf("%d %d %d %d %d %d %d %d : %d %d %d %d %d\n", tracked, sg, sh, kernel, image, lg, lf, ok, (int)r.mode, (int)r.next.track,
               r.next.w, r.next.h, r.next.frames);
    }
    return 0;
}
'''

GEO = [(1280, 70, 20), (192, 70, 3), (2112, 40, 33)]
FRAMES = [24, 48, 60]
WS, OTHER = 0, 1
FULL, DELTA = 0, 1
UNKNOWN = (0, 0, 0, 0)


def table(tracked, sg, sh, kernel, image, lg, lf, ok):
    """(mode, next state) as the rules read:
    - delta only for k_binary_ws, with the image wanted, on a mask in force for the same w x h that covers the batch's frames, ww <= 32;
    - k_binary_ws with the image leaves the mask in force for its geometry (and for the most frames it has been kept for);
    - a launch without the image touches neither image nor mask: the state stays;
    - any other kernel writing the image, and any launch that failed, leaves nothing known."""
    w, h, ww = GEO[lg]
    n = FRAMES[lf]
    state = (1, GEO[sg][0], GEO[sg][1] + sh, 48) if tracked else UNKNOWN
    same = tracked and sg == lg and sh == 0
    if not ok:
        nxt = UNKNOWN
    elif not image:
        nxt = state
    elif kernel == OTHER:
        nxt = UNKNOWN
    else:
        nxt = (1, w, h, max(n, 48) if same else n)
    mode = DELTA if (kernel == WS and image and same and n <= 48 and ww <= 32) else FULL
    return (mode,) + nxt


def test_image_step_matches_the_table(tmp_path):
    src = tmp_path / "image_plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "image_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    seen, deltas = set(), 0
    for line in lines:
        key, got = line.split(":")
        args = tuple(int(v) for v in key.split())
        got = tuple(int(v) for v in got.split())
        assert got == table(*args), (args, got, table(*args))
        seen.add(args)
        deltas += got[0] == DELTA
    assert seen == set(itertools.product((0, 1), range(3), (0, 1), (0, 1), (0, 1), range(3), range(3), (0, 1)))
    # delta: tracked, same geometry of the two with ww <= 32, k_binary_ws, image, 24 or 48 frames, enqueued or not
    assert deltas == 2 * 2 * 2
