"""Seeded observation sequences for the device tracker's tests (tests/test_tracker_cpu.py, the fixed hypot list of
tests/test_pinned_hypot.py): per scenario a config and a list of steps (frame-coordinate boxes, identities | None, positions | None,
timestamp).  Boxes are integer-valued, so moving them between window and frame coordinates is exact in float32."""
import numpy as np

from rmcv_amd import abi

MS = 1_000_000  # ticks (tick_frequency 1e9)


def armour(x, y, w=60.0, h=50.0):
    a = np.zeros(1, abi.ARMOUR)
    a[0]["bbox"] = (x, y, w, h)
    a[0]["vertices"] = [[x, y + h], [x, y], [x + w, y], [x + w, y + h]]
    a[0]["icon"] = [[x + 8, y + h - 4], [x + 8, y + 4], [x + w - 8, y + 4], [x + w - 8, y + h - 4]]
    a[0]["blob_i"], a[0]["blob_j"] = 0, 1
    return a[0]


def _pack(boxes):
    return np.array([armour(*b) for b in boxes], abi.ARMOUR) if boxes else np.zeros(0, abi.ARMOUR)


def scenarios():
    """name -> (config overrides, [(armours, identities | None, positions | None, timestamp)])"""
    out = {}
    win = dict(win_w=512, win_h=384)
    jit = np.cumsum(np.random.default_rng(100).integers(4 * MS, 13 * MS, 800))   # frame times with jitter: every step its own dt
    rng = np.random.default_rng(101)
    out["static"] = (win, [(_pack([(400, 300)]), [3], 5 + rng.normal(size=(1, 3)), int(jit[k])) for k in range(350)])
    # drifting 3 px a step: IoU with the stale box is (60 - d) / (60 + d) <= 0.5 from d = 20 on -> a new track every 7 steps, the old ones
    # coast and are erased on their 27th miss, the neighbour behind each skipped in that pass
    rng = np.random.default_rng(102)
    out["drift"] = (dict(win, roi_scale_w=1.5, roi_scale_h=2.0),
                    [(_pack([(100 + 3 * k, 500)]), [int(rng.integers(1, 6))], np.array([[0.01 * k, 1.0, 3.0]]) + 0.05 * rng.normal(size=(1, 3)), int(jit[k + 60]))
                     for k in range(110)])
    rng = np.random.default_rng(103)
    out["crossing"] = (dict(win, process_noise=2e-5, measurement_noise=0.8), [(_pack([(200 + 8 * k, 400), (760 - 8 * k, 404)]), [1, 2],
                              np.array([[0.02 * k, 0, 2.0], [1.4 - 0.02 * k, 0, 2.0]]) + 0.01 * rng.normal(size=(2, 3)), int(jit[k + 40])) for k in range(70)])
    rng = np.random.default_rng(104)
    out["identities"] = (dict(win, process_noise=1e-4, measurement_noise=0.3, error=0.1), [(_pack([(640, 200)]), [int(rng.integers(-1, 14))], rng.normal(size=(1, 3)), int(jit[2 * k])) for k in range(250)])
    rng = np.random.default_rng(105)
    steps = []
    for k in range(75):   # no observation in the first two steps and in every third: nothing ages
        seen = k >= 2 and k % 3 != 0
        steps.append((_pack([(300, 600), (900, 100 + (k if k < 40 else 200))] if seen else []), [4, 5] if seen else [], rng.normal(size=(2 if seen else 0, 3)), int(jit[3 * k + 7])))
    out["gaps"] = (dict(win, error=0.2), steps)
    rng = np.random.default_rng(106)
    out["equal_stamps"] = (dict(win, measurement_noise=0.25), [(_pack([(500, 500)]), [2], rng.normal(size=(1, 3)), int(jit[300 + (20 + (k - 20) // 3 if 20 <= k < 40 else k)])) for k in range(120)])
    out["bare"] = (dict(win_w=0, win_h=0, process_noise=3e-4), [(_pack([(100 + (k % 5), 100), (700, 700 + 2 * k)]), None, None, int(jit[400 + 3 * k])) for k in range(120)])
    return out
