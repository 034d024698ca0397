"""What the per-stream model table costs a C5 step, in one process with the arms alternating, printed as ONE JSON line and
written to profiles/models_bench.json.  256 resident 1280x1024 frames through the pipeline, RMCV_STAGE_ALL | IDENTITY; REGIONS x STEPS per
arm (median, spread):
  a_off      selection off: the fused classifier of the sparse kernel, the step as it was (the yardstick)
  a_off2     the same arm once more: what "no difference" means is the spread between these two
  b_one      selection on, one model for all frames (every index 0): the fused classifier traded for the batch-wide k_classify_models
  c_four     selection on, 4 models interleaved over the frames
and the classifier alone between device events on a context whose batch has been through STAGE_ALL (a run of RMCV_STAGE_IDENTITY is that
one launch; 10 x STEPS launches per region, enqueued behind a k_delay so that they run back to back): k_classify with one model,
k_classify_models with one model and with four.
python tools/models_bench.py [regions steps [arm ...]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, OPT_TEST_DELAY_US, STAGE_ALL, STAGE_IDENTITY, Context, Pipeline, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
NAMES = argv[2:] or ["a_off", "a_off2", "b_one", "c_four"]
N, W, H = 256, 1280, 1024
C5 = STAGE_ALL | STAGE_IDENTITY
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
MODELS = [synth.svm_weights(20241008, 7), synth.svm_weights(7, 7), synth.svm_weights(11, 3), synth.svm_weights(13, 8)]


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


host_frames = [synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16) for k in range(2)]
frames = [torch.from_numpy(f).to(dev) for f in host_frames]
pls, counter = {}, {name: 0 for name in NAMES}
for name in NAMES:
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    for c in pl.contexts:
        c.svm_load_models(MODELS)
    if name in ("b_one", "c_four"):
        idx = torch.tensor([f % 4 if name == "c_four" else 0 for f in range(N)], dtype=torch.int32, device=dev)
        pl.set_frame_models(idx.data_ptr(), N, keepalive=idx)
    pls[name] = pl


def rotation(r):
    """the arms in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        i = counter[name] % 2
        counter[name] += 1
        pl.submit(frames[i].data_ptr(), N, H, W, p, C5)
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for name in NAMES:  # warm-up: every context of the ring has bound the geometry
    region(name, 40)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    for name in rotation(r):
        ms[name].append(region(name, STEPS))

out = {"tool": "models_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "stages": "ALL|IDENTITY", "models": len(MODELS)}
base = float(np.median(ms[NAMES[0]]))
for name in NAMES:
    s = stats(ms[name])
    info = pls[name].get_info()
    out[name] = {"pipeline_ms_per_step": s, "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1), "host_blocking_calls": int(info.host_blocking_calls),
                 "step_vs_" + NAMES[0]: round(s["median"] / base, 4)}
if "a_off" in out and "a_off2" in out:
    m = [out[k]["pipeline_ms_per_step"] for k in ("a_off", "a_off2")]
    out["a_spread"] = round(max(abs(m[0]["median"] - m[1]["median"]) / m[0]["median"], m[0]["spread"], m[1]["spread"]), 4)
for name in NAMES:
    pls[name].close()

# ---- the classifier alone, between device events: the same armours, the launch repeated (it is idempotent: icons are clamped once)
c = Context(device=0, max_frames=N, max_width=W, max_height=H)
c.svm_load_models(MODELS)
c.upload(host_frames[0])
c.run(p, C5)
c.sync()
out["armours"] = int(len(c.armours()[0]))
stream = torch.cuda.Stream()   # a stream of its own: the launches and the events that time them are on the same one
LAUNCHES = 10 * STEPS
kernel = {}
for name, idx in (("k_classify_one_model", None), ("k_classify_models_one_model", [0] * N), ("k_classify_models_four_models", [f % 4 for f in range(N)])):
    c.set_frame_models(idx)
    for _ in range(20):
        c.run(p, STAGE_IDENTITY, stream.cuda_stream)
    us = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c.set_option(OPT_TEST_DELAY_US, 20000)   # the stream is held back while the host enqueues: the launches then run back to back
        c.run(p, STAGE_IDENTITY, stream.cuda_stream)
        e0.record(stream)
        for _ in range(LAUNCHES):
            c.run(p, STAGE_IDENTITY, stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) / LAUNCHES * 1e3)
    c.sync()
    kernel[name] = stats(us)
out["kernel_us_per_launch"] = kernel
c.close()
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "models_bench.json"), "w").write(line + "\n")
print(line, flush=True)
