"""Raw Bayer input (RMCV_OPT_INPUT_FORMAT) against BGR, and the sensor's own layouts (RMCV_OPT_INPUT_SAMPLE_BITS / _VALID_BIT / _ORIENT:
8-bit flipped, 8-bit mirrored, 16-bit samples, 16-bit mirrored and flipped) against the plain 8-bit mosaic, in one process with all of
them alternating, printed as ONE JSON line:
  pipeline   ms per step and frames/s of 256 x 1280x1024 batches, 7 regions x 20 steps per format (median and spread)
  pixel      the pixel stage alone (rmcv_batch_run_timed's events): k_binary on BGR, k_binary_bayer on the mosaics, with and
             without the byte image
  chain      the per-frame drop-in chain (rmcv_extract_color -> rmcv_filter_lightblobs -> rmcv_filter_armours, one host frame):
             median and p90 in ms
The mosaics are the synthetic frames' colour filter arrays (synth.mosaic, pattern RG); the 16-bit buffers hold them at bits 4..11 with
random bits around (synth.raw_frame).  An orientation reads the same buffers mirrored / flipped: another scene, the same work.
python tools/bayer_bench.py [regions steps]"""
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
mosaics = [synth.mosaic(b, BAYER_RG) for b in bgr_sets]
sets = {"bgr": [torch.from_numpy(b).to(dev) for b in bgr_sets], "m8": [torch.from_numpy(m).to(dev) for m in mosaics],
        "m16": [torch.from_numpy(synth.raw_frame(m, 16, 4).view(np.uint8)).to(dev) for m in mosaics]}
# name -> (input format, layout keywords of Context.set_input_layout / Pipeline, the buffers it reads, bytes per pixel read)
CASES = {"bgr": (0, {}, "bgr", 3), "bayer": (BAYER_RG, {}, "m8", 1),
         "bayer_flip": (BAYER_RG, dict(flip=True), "m8", 1), "bayer_mirror": (BAYER_RG, dict(mirror=True), "m8", 1),
         "raw16": (BAYER_RG, dict(sample_bits=16, valid_bit=4), "m16", 2),
         "raw16_mirror_flip": (BAYER_RG, dict(sample_bits=16, valid_bit=4, mirror=True, flip=True), "m16", 2)}
NAMES = list(CASES)


def rotation(r):
    """the cases in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


# ---------------------------------------------------------------- pipeline, regions alternating
pls = {name: Pipeline(device=0, max_frames=N, max_width=W, max_height=H, input_format=fmt, **lay) for name, (fmt, lay, _, _) in CASES.items()}
counter = {name: 0 for name in NAMES}


def region(name, k):
    pl, bufs = pls[name], sets[CASES[name][2]]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        pl.submit(bufs[counter[name] % 4].data_ptr(), N, H, W, p, STAGE_ALL)
        counter[name] += 1
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for name in NAMES:  # warm-up: every context of the ring has bound the geometry
    region(name, 100)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    for name in rotation(r):
        ms[name].append(region(name, STEPS))
for pl in pls.values():
    pl.close()

# ---------------------------------------------------------------- the pixel stage alone (events around the launch)
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
pix = {name: {"image": [], "no_image": []} for name in NAMES}
for r in range(2 * REGIONS):
    for name in rotation(r):
        fmt, lay, which, _ = CASES[name]
        t = sets[which][r % 4]
        ctx.set_input_format(fmt)
        ctx.set_input_layout(**lay)
        ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
        pix[name]["image"].append(ctx.run_timed(p, STAGE_BINARY)[0])
        pix[name]["no_image"].append(ctx.run_timed(p, STAGE_BINARY | STAGE_NO_IMAGE)[0])
ctx.close()

# ---------------------------------------------------------------- the per-frame chain
L = lib()
c1 = Context(device=0, max_frames=1, max_width=W, max_height=H)
frames = {"bgr": [np.ascontiguousarray(bgr_sets[0][i]) for i in range(4)], "m8": [np.ascontiguousarray(mosaics[0][i]) for i in range(4)],
          "m16": [synth.raw_frame(mosaics[0][i], 16, 4) for i in range(4)]}
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


chain = {name: [] for name in NAMES}
for r in range(2 * REGIONS):
    for name in rotation(r):
        fmt, lay, which, bpp = CASES[name]
        c1.set_input_format(fmt)
        c1.set_input_layout(**lay)
        for i in range(4):
            one_chain(frames[which][i], bpp * W)
        chain[name] += [one_chain(frames[which][i % 4], bpp * W) for i in range(50)]
c1.close()

out = {"tool": "bayer_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "pattern": "RG"}
px = N * W * H
for name in NAMES:
    s = stats(ms[name])
    out[name] = {
        "pipeline_ms_per_step": s,
        "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1),
        "pixel_ms": stats(pix[name]["image"]),
        "pixel_ms_no_image": stats(pix[name]["no_image"]),
        "chain_ms_median": round(float(np.median(chain[name])), 4),
        "chain_ms_p90": round(float(np.percentile(chain[name], 90)), 4),
    }
    if name == "bgr":
        continue
    # the Bayer pixel stage against its byte bound at 8 TB/s: the samples read + 1 B/px of byte image + 1/8 for the plane
    read = CASES[name][3]
    out[name]["pixel_bound_ms"] = round(px * (read + 1.125) / 8e12 * 1e3, 4)
    out[name]["pixel_fraction_of_bound"] = round(out[name]["pixel_bound_ms"] / out[name]["pixel_ms"]["median"], 3)
    out[name]["pixel_bound_ms_no_image"] = round(px * (read + 0.125) / 8e12 * 1e3, 4)
    out[name]["pixel_fraction_of_bound_no_image"] = round(out[name]["pixel_bound_ms_no_image"] / out[name]["pixel_ms_no_image"]["median"], 3)
print(json.dumps(out), flush=True)
