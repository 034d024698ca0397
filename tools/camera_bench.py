"""What the per-stream camera and ballistics tables cost a tracked step, in one process with the arms alternating, printed as
ONE JSON line.  256 resident 1280x1024 frames, whole-frame tracker in the tracked loop (the host only submits), attitude and aiming on,
RMCV_STAGE_ALL | IDENTITY | POSE; REGIONS x STEPS per arm (median, spread):
  a_off      tables off: the tracked step as it was (the yardstick)
  a_off2     the same arm once more: what "no difference" means is the spread between these two
  b_same     tables on, every frame's index 0, every per-stream matrix and aim config equal to the single one
  c_mixed    4 cameras, 4 hand-eye matrices and 4 aim configs, mixed over the streams
python tools/camera_bench.py [regions steps [arm ...]]      (arms: all four; a build without the feature runs the a_off arms alone)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import (CAMP_BLUE, COMPENSATE_CLASSIC, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Pipeline, Tracker, default_aim_config, default_attitude_config,  # noqa: E402
                      default_params, default_pnp_config, synth)

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
NAMES = argv[2:] or ["a_off", "a_off2", "b_same", "c_mixed"]
N, W, H = 256, 1280, 1024
FULL = STAGE_ALL | STAGE_IDENTITY | STAGE_POSE
MS = 1000000   # ticks per millisecond at the tracker's default tick frequency
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


frames = [torch.from_numpy(synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)).to(dev) for k in range(2)]


def camera(k):
    """camera k of the fleet: 0 the default; the others another lens, plate and mount"""
    c = default_pnp_config()
    if k:
        c.camera_matrix[0], c.camera_matrix[4], c.camera_matrix[2], c.camera_matrix[5] = 1200.0 + 150.0 * k, 1210.0 + 150.0 * k, 640.0 - 9.0 * k, 512.0 + 7.0 * k
        c.dist[0], c.dist[1] = 0.02 * k, -0.05 * k
        c.square_w, c.square_h = 27.0 - 4.5 * k, 27.0 - 7.0 * k
        c.gripper2camera[3] += 10.0 * k
        c.gripper2camera[7] -= 6.0 * k
    return c


def ballistics(k):
    return default_aim_config(mode=COMPENSATE_CLASSIC if k % 2 else 0, v0=15.0 + 5.0 * k, height=10.0 * k, latency_s=0.004 * k)


CAMS = [camera(k) for k in range(4)]
pls, trks, counter = {}, {}, {name: 0 for name in NAMES}
for name in NAMES:
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
    t = Tracker(device=0, n_streams=N, frame_w=W, frame_h=H)
    t.set_aim(ballistics(0))
    t.set_attitude(default_attitude_config())
    if name in ("b_same", "c_mixed"):
        mixed = name == "c_mixed"
        idx = torch.tensor([f % 4 if mixed else 0 for f in range(N)], dtype=torch.int32, device=dev)
        for c in pl.contexts:
            c.pnp_load_cameras(CAMS if mixed else CAMS[:1])
        pl.set_frame_cameras(idx.data_ptr(), N, keepalive=idx)
        t.set_stream_cameras([CAMS[f % 4 if mixed else 0] for f in range(N)])
        t.set_aim_configs([ballistics(f % 4 if mixed else 0) for f in range(N)])
    pls[name], trks[name] = pl, t


def rotation(r):
    """the arms in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


def step(name):
    i = counter[name] % 2
    counter[name] += 1
    return pls[name].submit(frames[i].data_ptr(), N, H, W, p, FULL, tracker=trks[name], timestamp=counter[name] * 8 * MS)


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        step(name)
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for name in NAMES:  # warm-up: every context of the ring has bound the geometry
    region(name, 40)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    for name in rotation(r):
        ms[name].append(region(name, STEPS))

out = {"tool": "camera_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "stages": "ALL|IDENTITY|POSE", "attitude": True, "aiming": True}
base = float(np.median(ms[NAMES[0]]))
for name in NAMES:
    s = stats(ms[name])
    info = pls[name].get_info()
    aims = trks[name].aims()
    out[name] = {"pipeline_ms_per_step": s, "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1), "host_blocking_calls": int(info.host_blocking_calls),
                 "streams_with_a_target": int((aims["track"] >= 0).sum()), "step_vs_" + NAMES[0]: round(s["median"] / base, 4)}
if "a_off" in out and "a_off2" in out:   # "no difference": the distance between the two runs of the same arm, and each one's own spread
    m = [out[k]["pipeline_ms_per_step"] for k in ("a_off", "a_off2")]
    out["a_spread"] = round(max(abs(m[0]["median"] - m[1]["median"]) / m[0]["median"], m[0]["spread"], m[1]["spread"]), 4)
    for name in NAMES:
        if name not in ("a_off", "a_off2"):
            out[name]["within_a_spread"] = bool(out[name]["step_vs_" + NAMES[0]] - 1.0 <= out["a_spread"])
for name in NAMES:
    pls[name].close()
    trks[name].close()
print(json.dumps(out), flush=True)
