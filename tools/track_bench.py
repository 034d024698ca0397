"""The closed locked-target loop (detect -> track -> GetROI -> window -> detect) three ways, in one process with the cases alternating,
printed as ONE JSON line:
  tracked    (a) rmcv_pipeline_submit_tracked: the device-resident tracker steps behind every batch and writes the next batch's origins; the
             host only submits
  host_loop  (b) the same loop from the API that predates the device tracker: rmcv_pipeline_collect, then per stream rmcv_track_init /
             _reset / rmcv_track_step, rmcv_get_roi, rmcv_window_origin, an upload of the origins, rmcv_pipeline_submit_windows -- one batch
             in flight, as that loop must be.  The host side is THIS Python process calling the C-ABI through ctypes with preallocated
             buffers (about seven calls per stream and step): a C host pays less per call, the round trip stays
  open_loop  (c) rmcv_pipeline_submit_windows with fixed origins and nothing tracked: the floor
  step_ms    the tracker's step kernel alone, by events around rmcv_batch_track on one context
  sanity     (a) is not slower than (b): true / false -- the tool's one pass condition; false is a finding to explain, nothing is tuned around it
256 resident 1280x1024 frames per step, a moving synthetic scene of SCENE steps (played forwards and backwards), windows of 512x384,
RMCV_STAGE_ALL (identity -1, position 0 in every case).  REGIONS x STEPS per case after a warm-up, as tools/window_bench.py.
python tools/track_bench.py [regions steps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, Context, Pipeline, Tracker, abi, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H, WW, WH, SCENE = 256, 1280, 1024, 512, 384, 4
MS = 1_000_000
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
d_first = torch.from_numpy(first).to(dev)

NAMES = ["tracked", "host_loop", "open_loop"]
pls = {name: Pipeline(device=0, max_frames=N, max_width=W, max_height=H) for name in NAMES}
trk = Tracker(device=0, n_streams=N, frame_w=W, frame_h=H, win_w=WW, win_h=WH)
trk.set_origins(first)
counter = {name: 0 for name in NAMES}

# (b)'s host state: one list per stream, preallocated
CAP = 64
h_tracks = np.zeros((N, CAP), abi.TRACK)
h_n = np.zeros(N, np.int32)
h_side = np.zeros((N, CAP, 4, 2), np.float32)
h_obs = np.zeros(CAP, abi.TRACK)
h_req = first.copy()
d_req = torch.from_numpy(h_req).to(dev)
h_rect, h_xy, zero3 = np.zeros(4, np.int32), np.zeros(2, np.int32), np.zeros(3)
pending = [None]


def host_step(ticket, ts):
    """collect + track + GetROI + window origin for every stream + upload: what the host did between two batches before the device tracker"""
    a, o = pls["host_loop"].collect(ticket)
    eff_x = np.clip(h_req[:, 0], 0, W - WW) & ~15
    eff_y = np.clip(h_req[:, 1], 0, H - WH)
    for f in range(N):
        lo, hi = int(o[f]), int(o[f + 1])
        if hi > lo:
            obs = a[lo:hi]
            L.rmcv_armours_to_frame(abi.ptr(obs), hi - lo, int(eff_x[f]), int(eff_y[f]))
            for k in range(hi - lo):
                L.rmcv_track_init(abi.ptr(h_obs[k:k + 1]), abi.ptr(obs[k:k + 1]), -1, C.c_int64(ts), abi.ptr(zero3))
                L.rmcv_track_reset(abi.ptr(h_obs[k:k + 1]), C.c_double(5e-5), C.c_double(0.5), C.c_double(0.05))
            no = C.c_int32(hi - lo)
            L.rmcv_track_step(abi.ptr(h_tracks[f]), abi.ptr(h_n[f:f + 1]), CAP, abi.ptr(h_obs), C.byref(no), C.c_double(1e9))
        if h_n[f]:
            # (the host tracker has no side record: the newest observation's vertices stand in for it, as a host loop would do)
            if hi > lo:
                h_side[f, 0] = a[lo]["vertices"]
            L.rmcv_get_roi(abi.ptr(h_side[f, 0]), 4, C.c_float(1.0), C.c_float(1.0), W, H, None, abi.ptr(h_rect))
            L.rmcv_window_origin(abi.ptr(h_rect), WW, WH, abi.ptr(h_xy))
            h_req[f] = h_xy
    d_req.copy_(torch.from_numpy(h_req))   # the upload


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        i = counter[name]
        fr = scene[order[i % len(order)]]
        ts = (i + 1) * 8 * MS
        if name == "tracked":
            pl.submit(fr.data_ptr(), N, H, W, p, STAGE_ALL, tracker=trk, timestamp=ts)
        elif name == "open_loop":
            pl.submit(fr.data_ptr(), N, H, W, p, STAGE_ALL, windows=(d_first.data_ptr(), WW, WH))
        else:
            if pending[0] is not None:
                host_step(*pending[0])
            pending[0] = (pl.submit(fr.data_ptr(), N, H, W, p, STAGE_ALL, windows=(d_req.data_ptr(), WW, WH)), ts)
        counter[name] += 1
    if name == "host_loop" and pending[0] is not None:
        host_step(*pending[0])
        pending[0] = None
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
n_dev, st_dev = trk.counts()
blocking = {name: int(pl.get_info().host_blocking_calls) for name, pl in pls.items()}
for pl in pls.values():
    pl.close()

# ---------------------------------------------------------------- the step kernel alone (events around rmcv_batch_track)
s = torch.cuda.Stream()
step_ms = []
trk.reset()
trk.set_origins(first)
for i in range(3 * REGIONS):
    fr = scene[order[i % len(order)]]
    ctx.bind_device_frames(fr.data_ptr(), N, H, W, keepalive=fr)
    ctx.set_windows(trk.device_origins(), WW, WH)
    ctx.run(p, STAGE_ALL, stream=s.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    ctx.track(trk, (i + 1) * 8 * MS, stream=s.cuda_stream)
    e1.record(s)
    s.synchronize()
    step_ms.append(e0.elapsed_time(e1))
ctx.close()
trk.close()

out = {"tool": "track_bench", "frames": N, "w": W, "h": H, "win_w": WW, "win_h": WH, "regions": REGIONS, "steps": STEPS, "scene_steps": SCENE,
       "host_of_b": "python + ctypes", "tracks_per_stream_mean": round(float(n_dev.mean()), 3), "streams_overflowed": int((st_dev != 0).sum())}
for name in NAMES:
    out[name] = {"ms_per_step": stats(ms[name]), "host_blocking_calls": blocking[name]}
out["step_kernel_ms"] = stats(step_ms[REGIONS:])
out["tracked_vs_open_loop"] = round(float(np.median(ms["tracked"]) / np.median(ms["open_loop"])), 4)
out["tracked_vs_host_loop"] = round(float(np.median(ms["tracked"]) / np.median(ms["host_loop"])), 4)
out["sanity_tracked_not_slower_than_host_loop"] = bool(np.median(ms["tracked"]) <= np.median(ms["host_loop"]))
print(json.dumps(out), flush=True)
sys.exit(0 if out["sanity_tracked_not_slower_than_host_loop"] else 1)
