"""What the view labels cost, in one process with the arms alternating, written as ONE JSON line to
profiles/view_labels_bench.json (or the path given) and to stdout.  256 resident 1280x1024 frames through RMCV_STAGE_ALL | _IDENTITY | _POSE,
every frame's view at 1024x768:
  pass      the label pass alone (k_view_text over 256 finished views; armours' lines) at scale 1 and 2: REGIONS regions of REPS calls between
            device events on a side stream (median, spread)
  pipeline  a pipeline step (submit .. drained, STEPS batches a region) with views only, and with views + labels at scale 1 and at scale 2,
            the three arms rotating from region to region
No threshold is set.  The only pass condition: the labelled views of two frames equal the host restatement (exit status 1 otherwise).
python tools/view_labels_bench.py [out.json [regions reps steps]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import (CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, VIEW_ALL, Context, Pipeline, default_params, synth, view_labels_host)  # noqa: E402
from rmcv_amd import abi  # noqa: E402

argv = sys.argv[1:]
OUT = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "view_labels_bench.json")
REGIONS = int(argv[1]) if len(argv) > 1 else 5
REPS = int(argv[2]) if len(argv) > 2 else 10
STEPS = int(argv[3]) if len(argv) > 3 else 8
N, W, H = 256, 1280, 1024
SIZE = (1024, 768)
SCALES = (1, 2)
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
eye = np.tile(np.eye(4), (N, 1, 1))

frames = synth.batch(1000003, N, W, H, CAMP_BLUE, 0, threads=16)
d_frames = torch.from_numpy(frames).to(dev)
chosen = np.arange(N, dtype=np.int32)


def loaded(c):
    c.svm_load(*synth.svm_weights())
    c.pnp_load()
    c.set_base2gripper(eye)


c = Context(device=0, max_frames=N, max_width=W, max_height=H)
loaded(c)
c.bind_device_frames(d_frames.data_ptr(), N, H, W, keepalive=d_frames)
c.set_base2gripper(eye)
c.run(p, FULL)
c.sync()
arm, offs = c.armours()
ids, pos = c.identities(), c.poses()[2]
buf = torch.empty((N, SIZE[1], SIZE[0], 3), dtype=torch.uint8, device=dev)

# ---- the pass condition
ok, checked = True, 0
for scale in SCALES:
    c.debug_views(chosen, SIZE, out=buf.data_ptr())
    c.batch_view_labels(chosen, buf.data_ptr(), SIZE, scale)
    c.sync()
    for f in (0, 171):
        lo, hi = int(offs[f]), int(offs[f + 1])
        want = c.debug_view(f, SIZE)   # (the renderer has its own tests; here only the labels over it are in question)
        view_labels_host(want, (W, H), scale, arm[lo:hi], ids[lo:hi], pos[lo:hi])
        same = bool(np.array_equal(buf[f].cpu().numpy(), want))
        ok, checked = ok and same, checked + 1
        if not same:
            print("MISMATCH frame %d at scale %d" % (f, scale), file=sys.stderr)
labels_per_batch = int(offs[N])

# ---- the label pass alone
side = torch.cuda.Stream(device=dev)
c.debug_views(chosen, SIZE, out=buf.data_ptr(), stream=side.cuda_stream)


def pass_region(scale):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(side)
    for _ in range(REPS):
        c.batch_view_labels(chosen, buf.data_ptr(), SIZE, scale, stream=side.cuda_stream)
    b.record(side)
    side.synchronize()
    return a.elapsed_time(b) / REPS


for scale in SCALES:
    c.batch_view_labels(chosen, buf.data_ptr(), SIZE, scale, stream=side.cuda_stream)
side.synchronize()
pass_ms = {s: [] for s in SCALES}
for r in range(REGIONS):
    for scale in (SCALES if r % 2 == 0 else SCALES[::-1]):
        pass_ms[scale].append(pass_region(scale))
c.close()

# ---- a pipeline step: views against views + labels
pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
for pc in pl.contexts:
    loaded(pc)
pl.set_views(chosen, SIZE, flags=VIEW_ALL)
ARMS = [("views", 0, 0), ("views_labels_s1", abi.LABEL_ARMOURS, 1), ("views_labels_s2", abi.LABEL_ARMOURS, 2)]


def pipeline_region(what, scale):
    pl.set_view_labels(what, scale)   # (drains)
    for _ in range(2):                # warm: the arm's first batches
        pl.submit(d_frames.data_ptr(), N, H, W, p, FULL)
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        pl.submit(d_frames.data_ptr(), N, H, W, p, FULL)
    pl.drain()
    return (time.perf_counter() - t0) * 1e3 / STEPS


step_ms = {name: [] for name, _, _ in ARMS}
launches0 = abi.lib().rmcv_view_text_launches()
for r in range(REGIONS):
    k = r % len(ARMS)
    for name, what, scale in ARMS[k:] + ARMS[:k]:
        step_ms[name].append(pipeline_region(what, scale))
blocking = pl.get_info().host_blocking_calls
launches = abi.lib().rmcv_view_text_launches() - launches0
pl.close()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    med = float(np.median(xs))
    return {"ms": round(med, 5), "spread": round(float((xs.max() - xs.min()) / med), 4), "regions": [round(float(x), 5) for x in xs]}


out = {"tool": "view_labels_bench", "frames": N, "w": W, "h": H, "view": list(SIZE), "regions": REGIONS, "reps": REPS, "steps": STEPS,
       "labels_per_batch": labels_per_batch, "views_checked": checked, "views_equal_host": ok, "host_blocking_calls": int(blocking),
       "label_launches_in_pipeline_arms": int(launches), "label_launches_expected": REGIONS * 2 * (STEPS + 2),
       "pass": {"scale_%d" % s: stats(pass_ms[s]) for s in SCALES}, "pipeline_step": {name: stats(step_ms[name]) for name, _, _ in ARMS}}
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
sys.exit(0 if ok else 1)
