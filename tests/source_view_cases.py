"""Inputs of the source-view tests: the frame generator and the size list.  The overlay geometry is tests/view_cases.py's.
Shared by tests/test_source_view_cpu.py, tests/test_source_view_plan.py, tests/test_source_view_sanitized.py and tests/test_gpu_source_view.py."""
import numpy as np

import view_cases as K

# view_cases.SIZES -- every one of them a staged tile (the last, a view of one pixel, has a span of 2 x 2) -- plus what source_view_plan.h needs
# for the gathered path: thumbnails of 1 : 16 in one tile and in two, and a 3 x 3-tile view of 1 : 5 by 1 : 10 whose tiles gather on both
# sides of a seam in either direction.  (200, 136) -> (160, 102) is the staged tile seam in both directions.
SIZES = list(K.SIZES) + [((640, 400), (40, 25)), ((256, 160), (16, 10)), ((640, 400), (130, 40))]
GATHERED = SIZES[len(K.SIZES):]


def frame(w, h, seed=11):
    """a seeded BGR frame (h, w, 3): per-channel noise over a ramp of its own direction and slope per channel, with saturated blocks of
    distinct colours.  No channel is constant and no two are equal anywhere for long: a swapped channel, a missed table lookup or a wrong
    demosaic site each changes bytes."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], 2)
    f = (ramp * 3 // 4 + rng.integers(0, 64, (h, w, 3))).astype(np.uint8)
    f[h // 5:h // 3, w // 6:w // 3] = (255, 0, 0)
    f[h // 2:h // 2 + max(h // 8, 1), w // 2:w // 2 + max(w // 5, 1)] = (0, 255, 255)
    f[h - max(h // 10, 1):, :max(w // 7, 1)] = (255, 255, 255)
    f[:max(h // 12, 1), w - max(w // 9, 1):] = (0, 0, 0)
    return f
