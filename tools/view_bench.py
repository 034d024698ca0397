"""What the operator's debug views cost a pipelined step, in one process with the arms alternating, printed as ONE JSON line.
256 resident 1280x1024 frames, RMCV_STAGE_ALL, the host only submits; REGIONS x STEPS per arm (median, spread):
  a_off      no views set: the step as it was (the yardstick)
  a_off2     the same arm once more: what "no difference" means is the spread between these two
  b_4        4 views at 1024x768 per batch (an operator watching a few streams)
  c_256      a view of every frame of every batch
and, on a context of its own, the two view kernels alone for 256 views (HIP events around REPS calls): the bytes they write per second
against the bare copy's 6.25 TB/s (README.md) -- both kernels together, so a lower bound for k_view_resize.
python tools/view_bench.py [regions steps [arm ...]]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, Context, Pipeline, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
NAMES = argv[2:] or ["a_off", "a_off2", "b_4", "c_256"]
N, W, H, VW, VH = 256, 1280, 1024, 1024, 768
VIEWS = {"a_off": [], "a_off2": [], "b_4": [0, 85, 170, 255], "c_256": list(range(N))}
COPY_TBS = 6.25
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


frames = [torch.from_numpy(synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)).to(dev) for k in range(2)]
pls, counter = {}, {name: 0 for name in NAMES}
for name in NAMES:
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    if VIEWS[name]:
        pl.set_views(VIEWS[name], (VW, VH))
    pls[name] = pl


def rotation(r):
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        counter[name] += 1
        pl.submit(frames[counter[name] % 2].data_ptr(), N, H, W, p, STAGE_ALL)
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for name in NAMES:  # warm-up: every context of the ring has bound the geometry
    region(name, 40)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    for name in rotation(r):
        ms[name].append(region(name, STEPS))

out = {"tool": "view_bench", "frames": N, "w": W, "h": H, "view": [VW, VH], "regions": REGIONS, "steps": STEPS, "stages": "ALL"}
base = float(np.median(ms[NAMES[0]]))
for name in NAMES:
    s = stats(ms[name])
    out[name] = {"views": len(VIEWS[name]), "pipeline_ms_per_step": s, "added_ms_per_step": round(s["median"] - base, 4), "step_vs_" + NAMES[0]: round(s["median"] / base, 4),
                 "host_blocking_calls": int(pls[name].get_info().host_blocking_calls)}
if "a_off" in out and "a_off2" in out:
    m = [out[k]["pipeline_ms_per_step"] for k in ("a_off", "a_off2")]
    out["a_spread"] = round(max(abs(m[0]["median"] - m[1]["median"]) / m[0]["median"], m[0]["spread"], m[1]["spread"]), 4)
for name in NAMES:
    pls[name].close()

# the two kernels alone
REPS = 20
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
ctx.bind_device_frames(frames[0].data_ptr(), N, H, W, keepalive=frames[0])
ctx.run(p, STAGE_ALL)
buf = torch.empty((N, VH, VW, 3), dtype=torch.uint8, device=dev)
alone = {}
side = torch.cuda.Stream(device=dev)   # (a stream of torch's, so that its events bracket the calls; NULL would be the context's own stream)
for n in (4, N):
    chosen = list(range(n))
    ctx.debug_views(chosen, (VW, VH), out=buf.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(side)
    for _ in range(REPS):
        ctx.debug_views(chosen, (VW, VH), out=buf.data_ptr(), stream=side.cuda_stream)
    b.record(side)
    side.synchronize()
    per = a.elapsed_time(b) / REPS
    tbs = n * 3 * VW * VH / (per * 1e-3) / 1e12
    alone[str(n)] = {"ms_per_call": round(per, 4), "written_TB_per_s": round(tbs, 3), "of_bare_copy": round(tbs / COPY_TBS, 3)}
out["view_kernels_alone"] = alone
ctx.close()
print(json.dumps(out), flush=True)
