"""What the session recorder costs and gives, in one process, printed as ONE JSON line and written to profiles/record_bench.json:
  kernels_alone   rmcv_pack_frames / rmcv_unpack_frames on 64 resident 1280x1024 synth frames (HIP events around REPS calls): GB/s of INPUT
                  (the unpacked bytes), beside the 8 TB/s HBM peak
  ratio           packed / input bytes on synth frames, BGR (lag 3) and their RG mosaic (lag 2), and on Poisson(6) noise rows of 3840 bytes
  pipeline        a pipelined step (256 resident frames, RMCV_STAGE_ALL, the host only submits) with 0, 0 again, 1 and 8 recorded frames
                  per batch, the arms alternating region by region: median ms per step, spread, what the recorder adds
python tools/record_bench.py [regions steps [out.json]]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

from rmcv_amd import CAMP_BLUE, STAGE_ALL, Pipeline, Recorder, default_params, pack_bound, synth  # noqa: E402
from rmcv_amd.abi import lib  # noqa: E402

argv = sys.argv[1:]
REGIONS = int(argv[0]) if len(argv) > 0 else 7
STEPS = int(argv[1]) if len(argv) > 1 else 20
OUT = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "record_bench.json")
N, W, H, NK = 256, 1280, 1024, 64
PEAK_GBS = 8000.0
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
p = default_params()
L = lib()


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 4), "min": round(float(xs.min()), 4), "max": round(float(xs.max()), 4),
            "spread": round(float((xs.max() - xs.min()) / np.median(xs)), 4)}


def mosaic_rg(bgr):
    """the RG mosaic of BGR frames [n, h, w, 3]: R G / G B"""
    m = bgr[..., 1].copy()
    m[:, 0::2, 0::2] = bgr[:, 0::2, 0::2, 2]
    m[:, 1::2, 1::2] = bgr[:, 1::2, 1::2, 0]
    return m


host = [synth.batch(k * 1000003, N, W, H, CAMP_BLUE, 0, threads=16) for k in range(2)]
frames = [torch.from_numpy(b).to(dev) for b in host]
out = {"tool": "record_bench", "w": W, "h": H, "regions": REGIONS, "steps": STEPS, "hbm_peak_GB_per_s": PEAK_GBS}

# ---- the kernels alone, and the ratios
REPS = 10
side = torch.cuda.Stream(device=dev)   # (a stream of torch's, so that its events bracket the calls)
planes = {"bgr_lag3": (frames[0][:NK].reshape(NK, H, 3 * W), 3),
          "mosaic_rg_lag2": (torch.from_numpy(mosaic_rg(host[0][:NK])).to(dev), 2),
          "poisson6_3840_lag3": (torch.from_numpy(np.minimum(np.random.default_rng(6).poisson(6.0, (16, H, 3840)), 255).astype(np.uint8)).to(dev), 3)}
alone, ratio = {}, {}
for name, (t, lag) in planes.items():
    n, h, wb = t.shape
    pitch = pack_bound(wb, h)
    packed = torch.empty(n * pitch, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    back = torch.zeros_like(t)
    pack = lambda: L.rmcv_pack_frames(0, t.data_ptr(), n, wb, h, wb, C.c_int64(wb * h), lag, packed.data_ptr(), C.c_int64(pitch), sizes.data_ptr(), side.cuda_stream)  # noqa: E731
    unpack = lambda: L.rmcv_unpack_frames(0, packed.data_ptr(), n, wb, h, C.c_int64(pitch), lag, back.data_ptr(), wb, C.c_int64(wb * h), side.cuda_stream)  # noqa: E731
    res = {}
    for label, call in (("pack", pack), ("unpack", unpack)):
        assert call() == 0
        side.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        for _ in range(REPS):
            call()
        b.record(side)
        side.synchronize()
        per = a.elapsed_time(b) / REPS
        gbs = n * wb * h / (per * 1e-3) / 1e9
        res[label] = {"ms_per_call": round(per, 4), "input_GB_per_s": round(gbs, 1), "of_hbm_peak": round(gbs / PEAK_GBS, 4)}
    assert torch.equal(back, t), name   # lossless, at the size that is timed
    alone[name] = res
    ratio[name] = round(float(sizes.sum().item()) / (n * wb * h), 4)
    del packed, back
out["kernels_alone"] = {"frames": NK, **alone}
out["packed_over_input"] = ratio

# ---- a pipelined step with 0, 1 and 8 recorded frames per batch
CHOSEN = {"a_off": [], "a_off2": [], "b_1": [0], "c_8": [0, 36, 72, 108, 144, 180, 216, 252]}
NAMES = list(CHOSEN)
pls, recs, counter = {}, {}, {name: 0 for name in NAMES}
for name in NAMES:
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    if CHOSEN[name]:
        recs[name] = Recorder(device=0, slots=8, max_frames=8, max_w_bytes=3 * W, max_h=H)
        pl.set_recorder(recs[name], CHOSEN[name])
    pls[name] = pl


def region(name, k):
    pl = pls[name]
    pl.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        counter[name] += 1
        pl.submit(frames[counter[name] % 2].data_ptr(), N, H, W, p, STAGE_ALL)
    pl.drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


for name in NAMES:  # warm-up: every context of the ring has bound the geometry
    region(name, 40)
ms = {name: [] for name in NAMES}
for r in range(REGIONS):
    k = r % len(NAMES)
    for name in NAMES[k:] + NAMES[:k]:
        ms[name].append(region(name, STEPS))
base = float(np.median(ms["a_off"]))
pipe = {"frames": N, "stages": "ALL"}
for name in NAMES:
    s = stats(ms[name])
    pipe[name] = {"recorded_frames": len(CHOSEN[name]), "pipeline_ms_per_step": s, "added_ms_per_step": round(s["median"] - base, 4),
                  "step_vs_a_off": round(s["median"] / base, 4), "host_blocking_calls": int(pls[name].get_info().host_blocking_calls)}
m = [pipe[k]["pipeline_ms_per_step"] for k in ("a_off", "a_off2")]
pipe["a_spread"] = round(max(abs(m[0]["median"] - m[1]["median"]) / m[0]["median"], m[0]["spread"], m[1]["spread"]), 4)
for name, rec in recs.items():   # what was recorded last is what was submitted last
    e, _ = rec.entry(len(rec) - 1)
    want = host[counter[name] % 2][CHOSEN[name]]
    assert np.array_equal(rec.frames(len(rec) - 1), want), name
    pipe[name]["packed_over_input"] = round(sum(e.sizes[k] for k in range(e.n_frames)) / float(want.nbytes), 4)
out["pipeline"] = pipe
for name in NAMES:
    pls[name].close()
for rec in recs.values():
    rec.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
