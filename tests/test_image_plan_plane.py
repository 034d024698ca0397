"""plane_step (rmcv_amd/csrc/image_plan.h): whether a pixel launch may store the bit plane in delta mode -- only the words that are or
were non-zero, by the image's mask -- and how many leading frames have plane and image in step afterwards.  Compiled with the host C++
compiler; every combination of (frames in step before, image mode, kernel, image wanted, frames of the launch, enqueued or failed) is
checked against the rules restated below."""
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
    const int syncs[4] = {0, 24, 48, 60}, frames[3] = {24, 48, 60};
    for (int s = 0; s < 4; s++)
    for (int mode = 0; mode < 2; mode++)
    for (int kernel = 0; kernel < 2; kernel++)
    for (int image = 0; image < 2; image++)
    for (int lf = 0; lf < 3; lf++)
    for (int ok = 0; ok < 2; ok++) {
        const PlaneStep r = plane_step(syncs[s], (ImageMode)mode, {(ImageKernel)kernel, image != 0, 1280, 70, 20, frames[lf]}, ok != 0);
        printf("%d %d %d %d %d %d : %d %d\n", s, mode, kernel, image, lf, ok, (int)r.delta, r.next);
    }
    // ... and behind image_step, as the launcher chains them: a launch without the image, then one with it, then a delta launch
    ImageState st = {IMAGE_TRACKED, 1280, 70, 48};
    int sync = 48;
    const ImageLaunch seq[4] = {{IMAGE_KERNEL_WS, true, 1280, 70, 20, 48}, {IMAGE_KERNEL_WS, false, 1280, 70, 20, 48},
                                {IMAGE_KERNEL_WS, true, 1280, 70, 20, 24}, {IMAGE_KERNEL_WS, true, 1280, 70, 20, 48}};
    for (int i = 0; i < 4; i++) {
        const ImageStep is = image_step(st, seq[i], true);
        const PlaneStep ps = plane_step(sync, is.mode, seq[i], true);
        printf("seq %d : %d %d %d\n", i, (int)is.mode, (int)ps.delta, ps.next);
        st = is.next;
        sync = ps.next;
    }
    return 0;
}
'''

SYNCS = [0, 24, 48, 60]
FRAMES = [24, 48, 60]
WS, OTHER = 0, 1
FULL, DELTA = 0, 1


def table(s, mode, kernel, image, lf, ok):
    """(delta, frames in step afterwards) as the rules read:
    - the plane is delta-stored only by k_binary_ws, with the image, in a launch that stores the image in delta mode, and only if every
      frame of the launch has plane and image in step;
    - k_binary_ws with the image, enqueued completely, leaves its frames in step -- and, as a delta launch of fewer frames, the rest too;
    - a launch without the image rewrites the plane alone, any other kernel knows nothing of the mask, a failed launch leaves nothing
      known: no frame is in step."""
    sync, n = SYNCS[s], FRAMES[lf]
    if not image or kernel == OTHER:
        return (0, 0)
    delta = mode == DELTA and n <= sync
    if not ok:
        return (int(delta), 0)
    return (int(delta), sync if delta else n)


def test_plane_step_matches_the_table(tmp_path):
    src = tmp_path / "plane_plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "plane_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    seen, deltas, seq = set(), 0, []
    for line in lines:
        key, got = line.split(":")
        got = tuple(int(v) for v in got.split())
        if key.startswith("seq"):
            seq.append(got)
            continue
        args = tuple(int(v) for v in key.split())
        assert got == table(*args), (args, got, table(*args))
        seen.add(args)
        deltas += got[0]
    assert seen == set(itertools.product(range(4), (0, 1), (0, 1), (0, 1), range(3), (0, 1)))
    # delta: image mode delta, k_binary_ws, image, enqueued or not, and (sync, frames) one of (24, 24), (48, 24), (48, 48), (60, *)
    assert deltas == 2 * (1 + 2 + 3)
    # image delta + plane delta; no image: nothing in step; the image again, 24 frames: image delta, whole plane, 24 frames in step;
    # 48 frames: image delta (its mask still covers 48), whole plane -- frames 24 .. 47 still hold the plane of the launch without the image
    assert seq == [(DELTA, 1, 48), (FULL, 0, 0), (DELTA, 0, 24), (DELTA, 0, 48)]
