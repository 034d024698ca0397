"""What the recorder's loop records cost a tracked step: the tracked submit loop of tools/track_bench.py -- 256 resident
1280x1024 frames a step, a moving synthetic scene, windows of 512x384, RMCV_STAGE_ALL, the host only submits -- with a recorder of 8 chosen
frames attached, three ways, in ONE process with the arms alternating region by region, printed as one JSON line:
  cap0      track_cap = 0: no loop records -- what the recorder did before it knew them.  THE BASELINE
  cap16     track_cap = 16: k_loop_record behind every step
  armed     track_cap = 16 with every trigger armed (the rule runs either way; armed adds the latch's compare-and-swap when a bit fires --
            the recorder is resumed between regions so that it keeps recording)
  packing   the recorder's packing alone: cap0 against the same loop with no recorder at all (what the launch sits beside)
Each arm has its own pipeline, tracker and recorder; ratios are per region pair, the baseline is always the cap0 arm of the same rotation,
never a second run of the arm under test.  Nothing is asserted: nobody had measured this launch.
python tools/loop_bench.py [regions steps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, Context, Pipeline, Recorder, Tracker, abi, default_aim_config, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H, WW, WH, SCENE = 256, 1280, 1024, 512, 384, 4
CHOSEN = [0, 37, 74, 111, 148, 185, 222, 255]
MS = 1_000_000
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


base = synth.batch(0, N, W, H, CAMP_BLUE, 0, threads=16)
scene = []
for k in range(SCENE):
    f = np.zeros_like(base)
    f[:, 2 * k:, 4 * k:] = base[:, :H - 2 * k, :W - 4 * k]
    scene.append(torch.from_numpy(f).to(dev))
del base
order = list(range(SCENE)) + list(range(SCENE - 2, 0, -1))

ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
ctx.bind_device_frames(scene[0].data_ptr(), N, H, W, keepalive=scene[0])
ctx.run(p, STAGE_ALL)
ctx.sync()
arm, offs = ctx.armours()
first = np.array([abi.window_origin(abi.get_roi(arm[offs[f]]["vertices"], 1.0, (W, H)), WW, WH) if offs[f + 1] > offs[f] else (W // 2 - WW // 2, H // 2 - WH // 2)
                  for f in range(N)], np.int32)
ctx.close()

NAMES = ["cap0", "cap16", "armed", "bare"]
CAP = {"cap0": 0, "cap16": 16, "armed": 16, "bare": None}
pls, trks, recs, counter = {}, {}, {}, {}
for name in NAMES:
    pls[name] = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    trks[name] = Tracker(device=0, n_streams=N, frame_w=W, frame_h=H, win_w=WW, win_h=WH)
    trks[name].set_origins(first)
    trks[name].set_aim(default_aim_config())
    counter[name] = 0
    if CAP[name] is not None:
        recs[name] = Recorder(device=0, slots=pls[name].depth + 1, max_frames=len(CHOSEN), max_w_bytes=3 * W, max_h=H, track_cap=CAP[name])
        if name == "armed":
            recs[name].set_trigger(abi.TRIG_ALL, post_batches=1, frame_status_mask=0x7F, aim_jump_deg=1e9)
        pls[name].set_recorder(recs[name], CHOSEN)


def region(name, k):
    pl = pls[name]
    if name == "armed":
        recs[name].resume()     # (off the timed path: a latch taken in the last region is cleared, the recorder records again)
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        i = counter[name]
        fr = scene[order[i % len(order)]]
        pl.submit(fr.data_ptr(), N, H, W, p, STAGE_ALL, tracker=trks[name], timestamp=(i + 1) * 8 * MS)
        counter[name] += 1
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def rotation(r):
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


for name in NAMES:
    region(name, 40)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    for name in rotation(r):
        ms[name].append(region(name, STEPS))
ratio = {name: stats(np.array(ms[name]) / np.array(ms["cap0"])) for name in ("cap16", "armed")}
packing = stats(np.array(ms["cap0"]) / np.array(ms["bare"]))
info = {name: pls[name].get_info() for name in NAMES}
latch = recs["armed"].trigger()
out = {"tool": "loop_bench", "frames": N, "chosen": len(CHOSEN), "regions": REGIONS, "steps": STEPS, "ms_per_step": {name: stats(ms[name]) for name in NAMES},
       "ratio_to_cap0": ratio, "cap0_to_no_recorder": packing,
       "added_ms_median": {name: round(float(np.median(np.array(ms[name]) - np.array(ms["cap0"]))), 4) for name in ("cap16", "armed")},
       "packing_ms_median": round(float(np.median(np.array(ms["cap0"]) - np.array(ms["bare"]))), 4),
       "armed_latch_fired": int(latch.fired), "host_blocking_calls": {name: int(info[name].host_blocking_calls) for name in NAMES}}
print(json.dumps(out))
