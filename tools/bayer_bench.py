"""Raw Bayer input (RMCV_OPT_INPUT_FORMAT) against BGR, in one process with the two alternating, printed as ONE JSON line:
  pipeline   ms per step and frames/s of 256 x 1280x1024 batches, 7 regions x 20 steps per format (median and spread)
  pixel      the pixel stage alone (rmcv_batch_run_timed's events): k_binary on BGR, k_binary_bayer on the mosaics, with and
             without the byte image
  chain      the per-frame drop-in chain (rmcv_extract_color -> rmcv_filter_lightblobs -> rmcv_filter_armours, one host frame):
             median and p90 in ms
The mosaics are the synthetic frames' colour filter arrays (synth.mosaic, pattern RG).   python tools/bayer_bench.py [regions steps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import BAYER_RG, CAMP_BLUE, MORPH_CLOSE, STAGE_ALL, STAGE_BINARY, STAGE_NO_IMAGE, Context, Pipeline, default_params, synth  # noqa: E402
from rmcv_amd.abi import ARMOUR, LIGHTBLOB, POINT, lib, ptr  # noqa: E402

REGIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, W, H = 256, 1280, 1024
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


# ---------------------------------------------------------------- inputs: 4 batches per format, resident in HBM
bgr_sets = [synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16) for k in range(4)]
fmt_sets = {0: [torch.from_numpy(b).to(dev) for b in bgr_sets],
            BAYER_RG: [torch.from_numpy(synth.mosaic(b, BAYER_RG)).to(dev) for b in bgr_sets]}

# ---------------------------------------------------------------- pipeline, regions alternating
pls = {0: Pipeline(device=0, max_frames=N, max_width=W, max_height=H),
       BAYER_RG: Pipeline(device=0, max_frames=N, max_width=W, max_height=H, input_format=BAYER_RG)}
counter = {0: 0, BAYER_RG: 0}


def region(fmt, k):
    pl, sets = pls[fmt], fmt_sets[fmt]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        pl.submit(sets[counter[fmt] % 4].data_ptr(), N, H, W, p, STAGE_ALL)
        counter[fmt] += 1
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for fmt in (0, BAYER_RG):  # warm-up: every context of the ring has bound the geometry
    region(fmt, 100)
ms = {0: [], BAYER_RG: []}
for r in range(REGIONS):
    for fmt in ((0, BAYER_RG) if r % 2 == 0 else (BAYER_RG, 0)):
        ms[fmt].append(region(fmt, STEPS))
for pl in pls.values():
    pl.close()

# ---------------------------------------------------------------- the pixel stage alone (events around the launch)
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
pix = {}
for fmt in (0, BAYER_RG):
    pix[fmt] = {"image": [], "no_image": []}
for r in range(2 * REGIONS):
    for fmt in ((0, BAYER_RG) if r % 2 == 0 else (BAYER_RG, 0)):
        t = fmt_sets[fmt][r % 4]
        ctx.set_input_format(fmt)
        ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
        pix[fmt]["image"].append(ctx.run_timed(p, STAGE_BINARY)[0])
        pix[fmt]["no_image"].append(ctx.run_timed(p, STAGE_BINARY | STAGE_NO_IMAGE)[0])
ctx.close()

# ---------------------------------------------------------------- the per-frame chain
L = lib()
c1 = Context(device=0, max_frames=1, max_width=W, max_height=H)
frames = {0: [np.ascontiguousarray(bgr_sets[0][i]) for i in range(4)], BAYER_RG: [synth.mosaic(bgr_sets[0][i], BAYER_RG) for i in range(4)]}
binary = np.empty((H, W), np.uint8)
pts, offs = np.empty(c1.limits.max_points, POINT), np.empty(c1.limits.max_contours + 1, np.int32)
blobs, neg = np.empty(c1.limits.max_blobs, LIGHTBLOB), np.empty(c1.limits.max_contours, np.int32)
arms = np.empty(c1.limits.max_armours, ARMOUR)
nc, npt, nb, nn, na = (C.c_int32(0) for _ in range(5))


def one_chain(img, rowb):
    t0 = time.perf_counter()
    rc = L.rmcv_extract_color(c1._h, ptr(img), W, H, rowb, CAMP_BLUE, 80, MORPH_CLOSE, ptr(binary), ptr(pts), len(pts), ptr(offs),
                              len(offs) - 1, C.byref(nc), C.byref(npt))
    rc |= L.rmcv_filter_lightblobs(c1._h, ptr(pts), ptr(offs), nc.value, C.c_float(70.0), C.c_float(1.5), C.c_float(80.0), C.c_double(10.0),
                                   C.c_double(99999.0), CAMP_BLUE, ptr(blobs), len(blobs), C.byref(nb), None, ptr(neg), C.byref(nn))
    rc |= L.rmcv_filter_armours(c1._h, ptr(blobs), nb.value, C.c_float(12.0), C.c_float(22.0), C.c_float(0.4), CAMP_BLUE, ptr(arms), len(arms),
                                C.byref(na))
    assert rc == 0
    return (time.perf_counter() - t0) * 1e3


chain = {0: [], BAYER_RG: []}
for r in range(2 * REGIONS):
    for fmt in ((0, BAYER_RG) if r % 2 == 0 else (BAYER_RG, 0)):
        c1.set_input_format(fmt)
        rowb = W if fmt else 3 * W
        for i in range(4):
            one_chain(frames[fmt][i], rowb)
        chain[fmt] += [one_chain(frames[fmt][i % 4], rowb) for i in range(50)]
c1.close()

name = {0: "bgr", BAYER_RG: "bayer"}
out = {"tool": "bayer_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "pattern": "RG"}
for fmt in (0, BAYER_RG):
    s = stats(ms[fmt])
    out[name[fmt]] = {
        "pipeline_ms_per_step": s,
        "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1),
        "pixel_ms": stats(pix[fmt]["image"]),
        "pixel_ms_no_image": stats(pix[fmt]["no_image"]),
        "chain_ms_median": round(float(np.median(chain[fmt])), 4),
        "chain_ms_p90": round(float(np.percentile(chain[fmt], 90)), 4),
    }
# the Bayer pixel stage against its byte bound: 2.125 B/px (1.125 without the byte image) at 8 TB/s
px = N * W * H
out["bayer"]["pixel_bound_ms"] = round(px * 2.125 / 8e12 * 1e3, 4)
out["bayer"]["pixel_fraction_of_bound"] = round(out["bayer"]["pixel_bound_ms"] / out["bayer"]["pixel_ms"]["median"], 3)
out["bayer"]["pixel_bound_ms_no_image"] = round(px * 1.125 / 8e12 * 1e3, 4)
out["bayer"]["pixel_fraction_of_bound_no_image"] = round(out["bayer"]["pixel_bound_ms_no_image"] / out["bayer"]["pixel_ms_no_image"]["median"], 3)
print(json.dumps(out), flush=True)
