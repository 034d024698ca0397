"""What the dataset harvest costs a pipelined step: ONE pipeline at the benchmark's geometry (256 resident 1280x1024 frames,
RMCV_STAGE_ALL, the host only submits) in one process, regions alternating between harvest off and on (rmcv_pipeline_set_harvest toggles it
between regions; the call drains, no submit blocks); REGIONS x STEPS per arm (median, spread), written to profiles/novelty_bench.json
(profiles/harvest_bench.json is the record of the three-arm tool of DESIGN.md 4m):
  off        no dataset attached: the step as it was (the yardstick)
  off2       the same arm once more: what "no difference" means is the spread between these two
  on         every batch appends its armours' rows (a label per frame, none skipped); the dataset is cleared between regions
  novel      the same into a dataset with novelty on (ring_rows 8, max_sad 0), never cleared: the frame sets repeat, so from their
             second round on every candidate is an exact duplicate of a row its stream's ring holds -- the steady state of a calm stream
and, on a context of its own, the kernels alone between HIP events, REPS appends of one batch: k_harvest_plan + k_harvest_rows, and with
novelty on k_harvest_novel + k_harvest_plan_novel + k_harvest_rows (the first append after a clear, which keeps every row, and the ones
behind it, which keep none).
python tools/harvest_bench.py [regions steps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, Context, DeviceDataset, Pipeline, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H = 256, 1280, 1024
ARMS = ["off", "off2", "on", "novel"]
RING_ROWS, MAX_SAD = 8, 0
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
labels = (np.arange(N) % 7).astype(np.int32)


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


frames = [torch.from_numpy(synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)).to(dev) for k in range(2)]
pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
ctx.bind_device_frames(frames[0].data_ptr(), N, H, W, keepalive=frames[0])
ctx.run(p, STAGE_ALL)
ctx.sync()
per_batch = int(ctx.counts()["n_armours"].sum())
ds = DeviceDataset(ctx, max(1, per_batch) * (STEPS + 40))   # room for a region's appends: nothing is dropped
novel = DeviceDataset(ctx, max(1, per_batch) * (len(ARMS) * REGIONS * STEPS // 4 + 80))   # never cleared: room for what every region keeps
novel.set_novelty(RING_ROWS, MAX_SAD)
count = 0


def region(arm, k):
    global count
    pl.set_harvest({"on": ds, "novel": novel}.get(arm), labels)
    ds.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        count += 1
        pl.submit(frames[count % 2].data_ptr(), N, H, W, p, STAGE_ALL)
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for arm in ARMS:  # warm-up: every context of the ring has bound the geometry
    region(arm, 40)
ms, rows, kept, near = {arm: [] for arm in ARMS}, [], [], []
for r in range(REGIONS):
    for arm in ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]:
        before = (novel.count, novel.novelty["near"])
        ms[arm].append(region(arm, STEPS))
        if arm == "on":
            rows.append(ds.count)
        if arm == "novel":
            kept.append(novel.count - before[0]), near.append(novel.novelty["near"] - before[1])
out = {"tool": "harvest_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "stages": "ALL", "rows_per_batch": per_batch,
       "rows_per_on_region": rows, "novelty": {"ring_rows": RING_ROWS, "max_sad": MAX_SAD, "rows_kept_per_novel_region": kept, "near_per_novel_region": near,
                                               "rows_kept_in_warm_up": novel.count - sum(kept), "dropped": novel.dropped},
       "dropped": ds.dropped, "host_blocking_calls": int(pl.get_info().host_blocking_calls)}
base = float(np.median(ms["off"]))
for arm in ARMS:
    s = stats(ms[arm])
    out[arm] = {"pipeline_ms_per_step": s, "added_ms_per_step": round(s["median"] - base, 4), "step_vs_off": round(s["median"] / base, 4)}
out["off_spread"] = round(max(abs(out["off"]["pipeline_ms_per_step"]["median"] - out["off2"]["pipeline_ms_per_step"]["median"]) / base,
                              out["off"]["pipeline_ms_per_step"]["spread"], out["off2"]["pipeline_ms_per_step"]["spread"]), 4)
pl.set_harvest(None)
pl.close()

# the two kernels alone: REPS appends of one batch between events
REPS = 20
side = torch.cuda.Stream(device=dev)
ds.clear()
ctx.harvest(ds, labels, stream=side.cuda_stream)
side.synchronize()
ds.clear()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
d_labels = torch.from_numpy(labels).to(dev)
a.record(side)
for _ in range(REPS):
    ctx.harvest(ds, d_labels.data_ptr(), stream=side.cuda_stream)
b.record(side)
side.synchronize()
out["harvest_kernels_alone"] = {"ms_per_append": round(a.elapsed_time(b) / REPS, 4), "rows_per_append": per_batch, "appends": REPS, "rows": ds.count}
# ... and with novelty on: the append that meets empty rings (every row kept, pushed and computed twice), then REPS that keep nothing
novel.clear()
a.record(side)
ctx.harvest(novel, d_labels.data_ptr(), stream=side.cuda_stream)
b.record(side)
side.synchronize()
first_ms, first_rows = a.elapsed_time(b), novel.count
a.record(side)
for _ in range(REPS):
    ctx.harvest(novel, d_labels.data_ptr(), stream=side.cuda_stream)
b.record(side)
side.synchronize()
out["novelty_kernels_alone"] = {"first_append_ms": round(first_ms, 4), "first_append_rows_kept": first_rows, "ms_per_append_all_near": round(a.elapsed_time(b) / REPS, 4),
                                "appends": REPS, "rows_kept_by_them": novel.count - first_rows, "near": novel.novelty["near"]}
novel.close()
ds.close()
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "novelty_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(json.dumps(out), flush=True)
