"""What the attitude step (k_attitude and its event wait for the tracker's previous step, in front of every tracked batch) costs a tracked
step, in one process with the arms alternating, printed as ONE JSON line.  256 resident 1280x1024 frames, whole-frame tracker, aiming on,
RMCV_STAGE_ALL | IDENTITY | POSE; REGIONS x STEPS per arm (median, spread):
  a_off          attitude off: the tracked step as it was (the yardstick)
  b_on           attitude on, no packets: the step reads the attitude table as it stands
  c_on_packets   attitude on, every batch with its 256 serial packets in device memory
python tools/attitude_bench.py [regions steps [arm ...]]      (arms: all three; a build without the feature runs a_off alone)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, Pipeline, Tracker, abi, default_aim_config, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
NAMES = argv[2:] or ["a_off", "b_on", "c_on_packets"]
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
packets = []
if "c_on_packets" in NAMES:
    for k in range(2):   # a gimbal that swings: every stream's angles differ, and differ between the two batches
        host = b"".join(abi.serial_encode(CAMP_BLUE, 0.1 * f + 5.0 * k, -0.05 * f + 2.0 * k, 0.01 * f) for f in range(N))
        packets.append(torch.from_numpy(np.frombuffer(host, np.uint8).reshape(N, 24).copy()).to(dev))

pls, trks, counter = {}, {}, {name: 0 for name in NAMES}
for name in NAMES:
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    for c in pl.contexts:
        c.svm_load(*synth.svm_weights())
        c.pnp_load()
    t = Tracker(device=0, n_streams=N, frame_w=W, frame_h=H)
    t.set_aim(default_aim_config())
    if name != "a_off":
        t.set_attitude()
    pls[name], trks[name] = pl, t


def rotation(r):
    """the arms in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


def step(name):
    i = counter[name] % 2
    counter[name] += 1
    kw = {"packets": packets[i].data_ptr()} if name == "c_on_packets" else {}
    return pls[name].submit(frames[i].data_ptr(), N, H, W, p, FULL, tracker=trks[name], timestamp=counter[name] * 8 * MS, **kw)


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

out = {"tool": "attitude_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "stages": "ALL|IDENTITY|POSE", "aiming": True}
base = float(np.median(ms[NAMES[0]]))
for name in NAMES:
    s = stats(ms[name])
    info = pls[name].get_info()
    aims = trks[name].aims()
    out[name] = {"pipeline_ms_per_step": s, "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1), "host_blocking_calls": int(info.host_blocking_calls),
                 "streams_with_a_target": int((aims["track"] >= 0).sum()), "step_vs_" + NAMES[0]: round(s["median"] / base, 4)}
    if name != "a_off":
        out[name]["packet_errors"] = int(trks[name].attitudes()[1].sum())
        out[name]["within_" + NAMES[0] + "_spread"] = bool(s["median"] / base - 1.0 <= out[NAMES[0]]["pipeline_ms_per_step"]["spread"])
for name in NAMES:
    pls[name].close()
    trks[name].close()
print(json.dumps(out), flush=True)
