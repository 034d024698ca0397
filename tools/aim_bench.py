"""The tracked loop (detect -> track -> re-window) with its aim three ways, in one process with the cases alternating, printed as ONE JSON
line:
  aim_on     (a) rmcv_pipeline_submit_tracked on a tracker with aiming on: k_aim runs behind every step and leaves one rmcv_aim per stream in
             HBM; the host only submits
  host_aim   (b) the same loop with aiming off plus what a host had to do before device-resident aiming: wait for the ticket, rmcv_tracker_get
             per stream (about 2.5 KB per track), rmcv_aim_step_host per stream.  The host side is THIS Python process calling the C-ABI
             through ctypes with preallocated buffers (two calls per stream and step): a C host pays less per call, the round trip stays
  aim_off    (c) aiming off, nothing read back: the floor
  aim_kernel_ms  k_aim alone, by events around rmcv_tracker_aim
  sanity     (a) is not slower than (b): true / false -- the tool's one pass condition; false is a finding to explain, nothing is tuned around it
256 resident 1280x1024 frames per step, a moving synthetic scene of SCENE steps (played forwards and backwards), windows of 512x384,
RMCV_STAGE_ALL | RMCV_STAGE_POSE (so the tracks carry positions), COMPENSATE_CLASSIC, one lead iteration.  REGIONS x STEPS per case after a
warm-up, as tools/track_bench.py.
python tools/aim_bench.py [regions steps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, STAGE_POSE, Context, Pipeline, Tracker, abi, default_aim_config, default_params, default_pnp_config, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H, WW, WH, SCENE = 256, 1280, 1024, 512, 384, 4
MS = 1_000_000
STAGES = STAGE_ALL | STAGE_POSE
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
L = abi.lib()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


# ---------------------------------------------------------------- the scene: every stream's frame moved (4, 2) pixels a step
base = synth.batch(0, N, W, H, CAMP_BLUE, 0, threads=16)
scene = []
for k in range(SCENE):
    f = np.zeros_like(base)
    f[:, 2 * k:, 4 * k:] = base[:, :H - 2 * k, :W - 4 * k]
    scene.append(torch.from_numpy(f).to(dev))
del base
order = list(range(SCENE)) + list(range(SCENE - 2, 0, -1))  # 0 1 2 3 2 1 0 1 ...

ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
ctx.bind_device_frames(scene[0].data_ptr(), N, H, W, keepalive=scene[0])
ctx.run(p, STAGE_ALL)
ctx.sync()
arm, offs = ctx.armours()
first = np.array([abi.window_origin(abi.get_roi(arm[offs[f]]["vertices"], 1.0, (W, H)), WW, WH) if offs[f + 1] > offs[f] else (W // 2 - WW // 2, H // 2 - WH // 2)
                  for f in range(N)], np.int32)
ctx.close()

aim_cfg = default_aim_config(mode=abi.COMPENSATE_CLASSIC, v0=28.0, lead_iterations=1)
inputs = np.zeros(N, abi.AIM_INPUT)
inputs["world2camera"] = abi.rigid_inverse(np.array(default_pnp_config().gripper2camera).reshape(4, 4))

NAMES = ["aim_on", "host_aim", "aim_off"]
pls, trks = {}, {}
for name in NAMES:
    pls[name] = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    for c in pls[name].contexts:
        c.pnp_load()
        c.set_base2gripper(np.tile(np.eye(4), (N, 1, 1)))
    trks[name] = Tracker(device=0, n_streams=N, frame_w=W, frame_h=H, win_w=WW, win_h=WH)
    trks[name].set_origins(first)
trks["aim_on"].set_aim(aim_cfg)
trks["aim_on"].set_aim_inputs(inputs)
counter = {name: 0 for name in NAMES}

# (b)'s host state, preallocated
CAP = 64
h_tracks = np.zeros(CAP, abi.TRACK)
h_n = C.c_int32(0)
h_aims = np.zeros(N, abi.AIM)


def host_aim(ticket, ts):
    """wait + per stream rmcv_tracker_get + rmcv_aim_step_host: what the host did after every step before device-resident aiming"""
    pls["host_aim"].wait(ticket)
    t = trks["host_aim"]._h
    for f in range(N):
        L.rmcv_tracker_get(t, f, abi.ptr(h_tracks), CAP, C.byref(h_n), None, None)
        L.rmcv_aim_step_host(C.byref(aim_cfg), 1e9, abi.ptr(h_tracks), h_n.value, abi.ptr(inputs[f:f + 1]), C.c_int64(ts), abi.ptr(h_aims[f:f + 1]))


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        i = counter[name]
        fr = scene[order[i % len(order)]]
        ts = (i + 1) * 8 * MS
        ticket = pl.submit(fr.data_ptr(), N, H, W, p, STAGES, tracker=trks[name], timestamp=ts)
        if name == "host_aim":
            host_aim(ticket, ts)
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
d_aims = trks["aim_on"].aims()
n_dev, st_dev = trks["aim_on"].counts()
blocking = {name: int(pl.get_info().host_blocking_calls) for name, pl in pls.items()}
for pl in pls.values():
    pl.close()

# ---------------------------------------------------------------- k_aim alone (events around rmcv_tracker_aim), on the lists the loop left
s = torch.cuda.Stream()
aim_ms = []
for i in range(3 * REGIONS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    trks["aim_on"].aim((counter["aim_on"] + i) * 8 * MS, stream=s.cuda_stream)
    e1.record(s)
    s.synchronize()
    aim_ms.append(e0.elapsed_time(e1))
for t in trks.values():
    t.close()

med = {name: float(np.median(ms[name])) for name in NAMES}
out = {"tool": "aim_bench", "frames": N, "w": W, "h": H, "win_w": WW, "win_h": WH, "regions": REGIONS, "steps": STEPS, "scene_steps": SCENE,
       "host_of_b": "python + ctypes", "tracks_per_stream_mean": round(float(n_dev.mean()), 3), "streams_overflowed": int((st_dev != 0).sum()),
       "streams_with_target": int((d_aims["track"] >= 0).sum()), "streams_with_solution": int(((d_aims["track"] >= 0) & (d_aims["status"] == 0)).sum())}
for name in NAMES:
    out[name] = {"ms_per_step": stats(ms[name]), "host_blocking_calls": blocking[name]}
out["aim_kernel_ms"] = stats(aim_ms[REGIONS:])
out["aim_on_minus_aim_off_ms"] = round(med["aim_on"] - med["aim_off"], 4)
out["aim_on_vs_host_aim"] = round(med["aim_on"] / med["host_aim"], 4)
out["sanity_aim_on_not_slower_than_host_aim"] = bool(med["aim_on"] <= med["host_aim"])
print(json.dumps(out), flush=True)
sys.exit(0 if out["sanity_aim_on_not_slower_than_host_aim"] else 1)
