"""Windowed detection (rmcv_pipeline_submit_windows) against the whole-frame step, in one process with all cases alternating, printed
as ONE JSON line:
  pipeline   ms per step and frames/s of 256 resident 1280x1024 frames through the pipeline, REGIONS x STEPS per case (median, spread):
             "whole" = rmcv_pipeline_submit on the whole frames (the step bench.py measures), then one case per window size -- 1280x1024
             (the window IS the frame: what the windowed path costs by itself), 640x512, 512x384, 256x192
  pixel      the pixel stage alone (rmcv_batch_run_timed's events): k_binary / k_binary_ws on the whole frames, k_binary_win on the windows
  bytes      what the pixel pass of one step moves by the contract: 3 B/px read + 1 B/px byte image + 1/8 B/px bit plane, per case
  sanity     the 512x384 step is not slower than the whole-frame step (it moves strictly fewer bytes): true / false, nothing tuned around it
With --parent-lib PATH the whole-frame step also runs on ANOTHER build of the library (the parent commit's librmcv_hip.so), as the case
"whole_parent", alternating with the others in the same run.
Every frame's window is centred on the first armour the library itself finds on the whole frame (the locked-target loop: detect ->
rmcv_get_roi -> rmcv_window_origin -> window); frames without one get the frame's centre.  The origins live in device memory.
python tools/window_bench.py [regions steps] [--parent-lib PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, STAGE_BINARY, Context, Pipeline, abi, default_params, synth  # noqa: E402

argv = sys.argv[1:]
PARENT = None
if "--parent-lib" in argv:
    i = argv.index("--parent-lib")
    PARENT = argv[i + 1]
    del argv[i:i + 2]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H = 256, 1280, 1024
SIZES = [(1280, 1024), (640, 512), (512, 384), (256, 192)]
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


# ---------------------------------------------------------------- inputs: 2 batches resident in HBM, and every frame's target
host_sets = [synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16) for k in range(2)]
sets = [torch.from_numpy(b).to(dev) for b in host_sets]
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
rects, locked = [], 0
for t in sets:
    ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
    ctx.run(p, STAGE_ALL)
    ctx.sync()
    arm, offs = ctx.armours()
    r = []
    for f in range(N):
        if offs[f + 1] > offs[f]:
            r.append(abi.get_roi(arm[offs[f]]["vertices"], 1.0, (W, H)))
            locked += 1
        else:
            r.append((W // 2, H // 2, 0, 0))
    rects.append(r)
origins = {size: [torch.from_numpy(np.array([abi.window_origin(rc, *size) for rc in r], np.int32)).to(dev) for r in rects] for size in SIZES}

NAMES = ["whole"] + ["win_%dx%d" % s for s in SIZES] + (["whole_parent"] if PARENT else [])
SIZE_OF = {"win_%dx%d" % s: s for s in SIZES}


def rotation(r):
    """the cases in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


# ---------------------------------------------------------------- pipeline, regions alternating
pls = {name: Pipeline(device=0, max_frames=N, max_width=W, max_height=H) for name in NAMES if name != "whole_parent"}
if PARENT:
    here = abi.use(abi.load(PARENT))     # the other build: its pipeline keeps its own handle of it
    pls["whole_parent"] = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    abi.use(here)
counter = {name: 0 for name in NAMES}


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        i = counter[name] % 2
        if name in SIZE_OF:
            ww, wh = SIZE_OF[name]
            pl.submit(sets[i].data_ptr(), N, H, W, p, STAGE_ALL, windows=(origins[(ww, wh)][i].data_ptr(), ww, wh))
        else:
            pl.submit(sets[i].data_ptr(), N, H, W, p, STAGE_ALL)
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
blocking = {name: int(pl.get_info().host_blocking_calls) for name, pl in pls.items()}
armours = {}
for name in NAMES:  # what a step finds (one more batch, collected)
    pl = pls[name]
    if name in SIZE_OF:
        ww, wh = SIZE_OF[name]
        t = pl.submit(sets[0].data_ptr(), N, H, W, p, STAGE_ALL, windows=(origins[(ww, wh)][0].data_ptr(), ww, wh))
    else:
        t = pl.submit(sets[0].data_ptr(), N, H, W, p, STAGE_ALL)
    armours[name] = int(len(pl.collect(t)[0]))
for name in NAMES:
    if name == "whole_parent":
        here = abi.use(pls[name]._lib)
        pls[name].close()
        abi.use(here)
    else:
        pls[name].close()

# ---------------------------------------------------------------- the pixel stage alone (events around the launch)
pix = {name: [] for name in NAMES if name != "whole_parent"}
for r in range(2 * REGIONS):
    for name in rotation(r):
        if name == "whole_parent":
            continue
        t = sets[r % 2]
        ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
        if name in SIZE_OF:
            ww, wh = SIZE_OF[name]
            ctx.set_windows(origins[(ww, wh)][r % 2].data_ptr(), ww, wh)
        ctx.run_timed(p, STAGE_BINARY)
        pix[name].append(ctx.run_timed(p, STAGE_BINARY)[0])
ctx.close()

out = {"tool": "window_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "frames_with_a_target": locked, "of": 2 * N,
       "parent_lib": bool(PARENT)}
for name in NAMES:
    s = stats(ms[name])
    ww, wh = SIZE_OF.get(name, (W, H))
    px = N * ww * wh
    out[name] = {"pipeline_ms_per_step": s, "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1), "host_blocking_calls": blocking[name],
                 "armours_per_step": armours[name], "pixel_bytes_per_step": int(px * 4.125), "pixel_bytes_read_per_step": int(px * 3)}
    if name in pix:
        out[name]["pixel_ms"] = stats(pix[name])
        out[name]["pixel_bound_ms_at_8TBps"] = round(px * 4.125 / 8e12 * 1e3, 4)
    out[name]["step_vs_whole"] = round(s["median"] / float(np.median(ms["whole"])), 4)
    out[name]["bytes_vs_whole"] = round(ww * wh / float(W * H), 4)
out["sanity_512x384_not_slower_than_whole"] = bool(np.median(ms["win_512x384"]) <= np.median(ms["whole"]))
print(json.dumps(out), flush=True)
