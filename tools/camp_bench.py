"""Per-frame detection keys (rmcv_pipeline_submit_camps) against the uniform step and against what a mixed fleet has to do without them, in
one process with all cases alternating, printed as ONE JSON line.  256 resident 1280x1024 frames; REGIONS x STEPS per case (median, spread):
  a_uniform_ws      the uniform batch (every frame BLUE) on the default path: the hot rotation's k_binary_ws
  b_uniform_k1      the same batch on the k_binary shape (pipeline: out of the hot rotation; pixel stage: RMCV_OPT_PIXEL_SHAPE 0) -- the
                    kernel whose shape the keyed one shares
  c_keys_equal      the same frames with per-frame keys that are all equal: c against b is the cost of the key alone
  d_keys_mixed      frames and camps alternating per frame (frame i generated and detected with camp i & 1)
  e_split           what a host has to do for d without keys: two submits of 128 frames, each colour's frames contiguous in a buffer of their
                    own, regrouped beforehand ...
  e_split_regroup   ... or regrouped in every step by a device-to-device gather the host waits for before it submits
  pipeline   ms per step and frames/s through the pipeline;   pixel   the pixel stage alone (rmcv_batch_run_timed's events)
python tools/camp_bench.py [regions steps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, CAMP_RED, STAGE_ALL, STAGE_BINARY, Context, Pipeline, abi, default_params, synth  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
N, W, H = 256, 1280, 1024
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
p_of = {0: default_params(camp=CAMP_RED), 1: default_params(camp=CAMP_BLUE)}


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


# ---------------------------------------------------------------- inputs: 2 batches of each kind resident in HBM
camps_mixed = np.array([i & 1 for i in range(N)], np.int32)
uniform = [torch.from_numpy(synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)).to(dev) for k in range(2)]
mixed_host = []
for k in range(2):
    b = synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16)
    red = synth.batch(k * 1000003, N, W, H, CAMP_RED, 0, threads=16)
    b[0::2] = red[0::2]
    mixed_host.append(b)
mixed = [torch.from_numpy(b).to(dev) for b in mixed_host]
groups = [{c: torch.from_numpy(np.ascontiguousarray(b[c::2])).to(dev) for c in (0, 1)} for b in mixed_host]   # regrouped beforehand
scratch = {c: torch.empty((N // 2, H, W, 3), dtype=torch.uint8, device=dev) for c in (0, 1)}                   # regrouped per step
index = {c: torch.arange(c, N, 2, device=dev) for c in (0, 1)}
d_equal = torch.full((N,), CAMP_BLUE, dtype=torch.int32, device=dev)
d_mixed = torch.from_numpy(camps_mixed).to(dev)
del mixed_host

NAMES = ["a_uniform_ws", "b_uniform_k1", "c_keys_equal", "d_keys_mixed", "e_split", "e_split_regroup"]


def rotation(r):
    """the cases in an order that starts one further on in every round, so that none always runs behind the same neighbour"""
    k = r % len(NAMES)
    return NAMES[k:] + NAMES[:k]


# ---------------------------------------------------------------- pipeline, regions alternating
pls = {name: Pipeline(device=0, max_frames=N, max_width=W, max_height=H, **({"hot_contexts": -1} if name == "b_uniform_k1" else {})) for name in NAMES}
counter = {name: 0 for name in NAMES}


def step(name, pl, i):
    """one step of 256 frames; returns the tickets"""
    if name in ("a_uniform_ws", "b_uniform_k1"):
        return [pl.submit(uniform[i].data_ptr(), N, H, W, p, STAGE_ALL)]
    if name == "c_keys_equal":
        return [pl.submit(uniform[i].data_ptr(), N, H, W, p, STAGE_ALL, camps=(d_equal.data_ptr(), None))]
    if name == "d_keys_mixed":
        return [pl.submit(mixed[i].data_ptr(), N, H, W, p, STAGE_ALL, camps=(d_mixed.data_ptr(), None))]
    if name == "e_split":
        return [pl.submit(groups[i][c].data_ptr(), N // 2, H, W, p_of[c], STAGE_ALL) for c in (0, 1)]
    out = []
    for c in (0, 1):   # the gather of one colour's frames, waited for (the pipeline's streams know nothing of torch's), then the submit
        torch.index_select(mixed[i], 0, index[c], out=scratch[c])
        torch.cuda.current_stream().synchronize()
        out.append(pl.submit(scratch[c].data_ptr(), N // 2, H, W, p_of[c], STAGE_ALL))
    return out


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        step(name, pl, counter[name] % 2)
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
hot = {name: int(pl.get_info().hot_batches) for name, pl in pls.items()}
armours = {}
for name in NAMES:  # what a step finds (one more step, collected)
    armours[name] = int(sum(len(pls[name].collect(t)[0]) for t in step(name, pls[name], 0)))
for pl in pls.values():
    pl.close()

# ---------------------------------------------------------------- the pixel stage alone (events around the launch)
ctx = Context(device=0, max_frames=N, max_width=W, max_height=H)
pix = {name: [] for name in NAMES if name != "e_split_regroup"}
ws0 = abi.lib().rmcv_pixel_ws_launches()
ws_by = {}
for r in range(2 * REGIONS):
    for name in rotation(r):
        if name == "e_split_regroup":
            continue
        i = r % 2
        before = abi.lib().rmcv_pixel_ws_launches()
        ctx.set_option(abi.OPT_PIXEL_SHAPE, 0 if name == "b_uniform_k1" else 1)
        if name == "e_split":
            total = 0.0
            for c in (0, 1):
                t = groups[i][c]
                ctx.bind_device_frames(t.data_ptr(), N // 2, H, W, keepalive=t)
                ctx.run_timed(p_of[c], STAGE_BINARY)
                total += ctx.run_timed(p_of[c], STAGE_BINARY)[0]
            pix[name].append(total)
        else:
            t = mixed[i] if name == "d_keys_mixed" else uniform[i]
            ctx.bind_device_frames(t.data_ptr(), N, H, W, keepalive=t)
            if name == "c_keys_equal":
                ctx.set_frame_camps(d_equal.data_ptr())
            elif name == "d_keys_mixed":
                ctx.set_frame_camps(d_mixed.data_ptr())
            ctx.run_timed(p, STAGE_BINARY)
            pix[name].append(ctx.run_timed(p, STAGE_BINARY)[0])
        ws_by[name] = ws_by.get(name, 0) + int(abi.lib().rmcv_pixel_ws_launches() - before)
ctx.close()

out = {"tool": "camp_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "steps": STEPS}
for name in NAMES:
    s = stats(ms[name])
    out[name] = {"pipeline_ms_per_step": s, "pipeline_frames_per_s": round(N / s["median"] * 1e3, 1), "host_blocking_calls": blocking[name],
                 "hot_batches": hot[name], "armours_per_step": armours[name],
                 "step_vs_b": round(s["median"] / float(np.median(ms["b_uniform_k1"])), 4)}
    if name in pix:
        out[name]["pixel_ms"] = stats(pix[name])
        out[name]["pixel_vs_b"] = round(float(np.median(pix[name])) / float(np.median(pix["b_uniform_k1"])), 4)
        out[name]["pixel_ws_launches"] = ws_by[name]
b_spread, c_over_b = out["b_uniform_k1"]["pixel_ms"]["spread"], out["c_keys_equal"]["pixel_vs_b"] - 1.0
out["pixel_c_within_b_spread"] = bool(c_over_b <= b_spread)
out["step_c_within_b_spread"] = bool(out["c_keys_equal"]["step_vs_b"] - 1.0 <= out["b_uniform_k1"]["pipeline_ms_per_step"]["spread"])
print(json.dumps(out), flush=True)
