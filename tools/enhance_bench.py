"""Exposure-adaptive detection (RMCV_OPT_ENHANCE) against the plain path of the SAME build, in one process with the two alternating,
at 256 x 1280x1024 and 256 x 1920x1200, printed as ONE JSON line:
  pixel      the pixel stage alone (rmcv_batch_run_timed's events around it): k_binary on the frames; with the option on the same
             bracket holds the sums pass, the table kernel and k_binary_enh -- so `pixel_enh - pixel_plain` is what the option adds to a
             lone batch.  (The kernels apart: run this tool under `rocprofv3 --kernel-trace --stats`; k_frame_sums alone against the
             bare 3:1 copy: tools/enhance_sums_bench.)
  pipeline   ms per step and frames/s, 7 regions x 20 steps each (median and spread between identical regions), plain (hot rotation,
             k_binary_ws), plain with hot_contexts off (k_binary: the shape enhancement batches take) and enhanced
  chunked    one experiment: the enhanced batch submitted as chunks of 32 frames (3.9 MB x 32 = 126 MB at 1280x1024: the frames the
             sums pass has just read fit the 256 MiB Infinity Cache when the pixel pass comes for them)
The frames are the synthetic stream dimmed to 80/256 (an under-exposed camera); plain and enhanced read the same buffers.
python tools/enhance_bench.py [regions steps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, STAGE_BINARY, STAGE_NO_IMAGE, Context, Pipeline, default_params, synth  # noqa: E402

REGIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


def measure(N, W, H):
    sets = []
    for k in range(4):  # 4 batches resident in HBM: consecutive steps read different frames
        b = synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)
        sets.append(torch.from_numpy(((b.astype(np.uint16) * 80) >> 8).astype(np.uint8)).to(dev))
    # ---- the pixel stage alone
    ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
    pix = {"plain": [], "enh": [], "plain_no_image": [], "enh_no_image": []}
    for r in range(2 * REGIONS + 2):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            t = sets[r % 4]
            ctx.set_enhance(on)
            ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
            a, b = ctx.run_timed(p, STAGE_BINARY)[0], ctx.run_timed(p, STAGE_BINARY | STAGE_NO_IMAGE)[0]
            if r >= 2:  # (the first two rounds warm up)
                pix["enh" if on else "plain"].append(a)
                pix["enh_no_image" if on else "plain_no_image"].append(b)
    ctx.close()
    # ---- the pipeline, regions alternating
    cases = {"plain": dict(), "plain_k_binary": dict(hot_contexts=-1), "enh": dict(enhance=True)}
    pls = {name: Pipeline(device=0, max_frames=N, max_width=W, max_height=H, **kw) for name, kw in cases.items()}
    counter = {name: 0 for name in cases}

    def region(name, k, chunk=None):
        pl = pls[name]
        pl.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            t = sets[counter[name] % 4]
            counter[name] += 1
            if chunk:
                for f0 in range(0, N, chunk):
                    pl.submit(t.data_ptr() + f0 * 3 * W * H, min(chunk, N - f0), H, W, p, STAGE_ALL)
            else:
                pl.submit(t.data_ptr(), N, H, W, p, STAGE_ALL)
        pl.drain()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3
    names = list(cases) + ["enh_chunked"]
    for name in cases:
        region(name, 60)
    region("enh", 10, 32)
    ms = {name: [] for name in names}
    for r in range(REGIONS):
        k = r % len(names)
        for name in names[k:] + names[:k]:
            ms[name].append(region("enh", STEPS, 32) if name == "enh_chunked" else region(name, STEPS))
    info = {name: pls[name].get_info() for name in cases}
    out = {"hot_batches": {name: int(info[name].hot_batches) for name in cases}, "host_blocking_calls": {name: int(info[name].host_blocking_calls) for name in cases}}
    for pl in pls.values():
        pl.close()
    out["pixel_ms"] = {k: stats(v) for k, v in pix.items()}
    out["pixel_added_ms"] = round(out["pixel_ms"]["enh"]["median"] - out["pixel_ms"]["plain"]["median"], 4)
    out["pipeline_ms_per_step"] = {k: stats(v) for k, v in ms.items()}
    out["pipeline_frames_per_s"] = {k: round(N / out["pipeline_ms_per_step"][k]["median"] * 1e3, 1) for k in ms}
    del sets
    torch.cuda.empty_cache()
    return out


res = {"tool": "enhance_bench", "regions": REGIONS, "steps": STEPS, "dimmed": "80/256"}
for (N, W, H) in ((256, 1280, 1024), (256, 1920, 1200)):
    res["%dx%dx%d" % (N, W, H)] = measure(N, W, H)
print(json.dumps(res), flush=True)
