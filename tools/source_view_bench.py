"""What the source view costs, in one process with the cases alternating, written as ONE JSON line to profiles/source_view_bench.json
(or the path given) and to stdout.  256 resident 1280x1024 frames, RMCV_STAGE_ALL run once; per case REGIONS regions of REPS calls between
device events on a side stream (median, spread), the order of the cases rotating from region to region:
  source   BGR frames and their RG mosaic -> 1024x768 (the debug thread's size), 640x512 (the exact half) and 160x128 (a thumbnail: gathered),
           1, 16 and 256 views a call (k_view_overlay + k_view_source)
  resize   the operator's view (k_view_overlay + k_view_resize) at the same sizes and counts        } the two yardsticks, from the same
  copy     a device-to-device copy of the source view's bytes by contract, per source and size      } process
Bytes by contract of a view: the source bytes of the spans its tiles touch (a staged tile: its span, a mosaic's with one ring; a gathered
tile: the distinct rows x columns of its taps), 3 bits a source pixel of planes (the two colour planes read, and written by k_view_overlay),
and 3 vw vh written.  The only pass condition: the rendered views at the bench sizes equal rmcv_source_view_host (exit status 1 otherwise).
python tools/source_view_bench.py [out.json [regions reps]]"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library initialises HIP: the tensors below are torch's)

import oracle_lib as O  # noqa: E402
from rmcv_amd import BAYER_RG, CAMP_BLUE, STAGE_ALL, VIEW_ALL, Context, default_params, source_view_host, synth  # noqa: E402

argv = sys.argv[1:]
OUT = argv[0] if len(argv) > 0 else os.path.join(ROOT, "profiles", "source_view_bench.json")
REGIONS = int(argv[1]) if len(argv) > 1 else 5
REPS = int(argv[2]) if len(argv) > 2 else 10
N, W, H = 256, 1280, 1024
SIZES = [(1024, 768), (640, 512), (160, 128)]
COUNTS = [1, 16, 256]
TILE_X, TILE_Y, STAGE_BYTES, RING_BYTES = 64, 16, 24576, 10240  # source_view_plan.h (tests/test_source_view_plan.py pins them)
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
O.set_math_mode(0)
p = default_params()


def taps(n_src, n_dst):
    if n_src == n_dst:
        return [(d, d) for d in range(n_dst)]
    if n_src == 2 * n_dst:
        return [(2 * d, 2 * d + 1) for d in range(n_dst)]
    out = []
    for d in range(n_dst):
        s = int(math.floor(float(np.float32((d + 0.5) * (n_src / n_dst) - 0.5))))
        out.append((min(max(s, 0), n_src - 1), min(max(s + 1, 0), n_src - 1)))
    return out


def contract_bytes(vw, vh, mosaic):
    """(bytes by contract of one view, staged tiles, gathered tiles)"""
    tx, ty = taps(W, vw), taps(H, vh)
    src = staged = gathered = 0
    for y0 in range(0, vh, TILE_Y):
        for x0 in range(0, vw, TILE_X):
            cols_t, rows_t = tx[x0:x0 + TILE_X], ty[y0:y0 + TILE_Y]
            rows, cols = rows_t[-1][1] - rows_t[0][0] + 1, cols_t[-1][1] - cols_t[0][0] + 1
            fits = rows * ((3 * cols + 6) & ~3) <= STAGE_BYTES and (not mosaic or (rows + 2) * (cols + 2) <= RING_BYTES)
            if fits:
                staged += 1
                src += (rows + 2) * (cols + 2) if mosaic else 3 * rows * cols
            else:
                gathered += 1
                ur, uc = {r for t in rows_t for r in t}, {c for t in cols_t for c in t}
                if mosaic:
                    ur, uc = {r + k for r in ur for k in (-1, 0, 1)}, {c + k for c in uc for k in (-1, 0, 1)}
                src += len(ur) * len(uc) * (1 if mosaic else 3)
    return src + 3 * W * H // 8 + 3 * vw * vh, staged, gathered


bgr = synth.batch(1000003, N, W, H, CAMP_BLUE, 0, threads=16)
mos = np.empty((N, H, W), np.uint8)  # the RG mosaic: R at (0, 0), B at (1, 1)
mos[:, 0::2, 0::2], mos[:, 0::2, 1::2], mos[:, 1::2, 0::2], mos[:, 1::2, 1::2] = bgr[:, 0::2, 0::2, 2], bgr[:, 0::2, 1::2, 1], bgr[:, 1::2, 0::2, 1], bgr[:, 1::2, 1::2, 0]
d_frames = {"bgr": torch.from_numpy(bgr).to(dev), "rg": torch.from_numpy(mos).to(dev)}
ctxs = {}
for name in ("bgr", "rg"):
    c = Context(device=0, max_frames=N, max_width=W, max_height=H)
    if name == "rg":
        c.set_input_format(BAYER_RG)
    c.bind_device_frames(d_frames[name].data_ptr(), N, H, W, keepalive=d_frames[name])
    c.run(p, STAGE_ALL)
    c.sync()
    ctxs[name] = c


CHOSEN = {n: np.array([k * N // n for k in range(n)], np.int32) for n in COUNTS}


def chosen(n):
    return CHOSEN[n]


# ---- the pass condition: the views at the bench sizes against the host restatement, two frames a source and size
checked, ok = 0, True
for name, c in ctxs.items():
    arm, offs = c.armours()
    for f in (0, 171):
        pts, co = c.contours(f)
        blobs, _ = c.blobs(f)
        _, _, neg = O.filter_lightblobs(pts, co, O.default_params())
        negatives = [np.stack([pts["x"][co[i]:co[i + 1]], pts["y"][co[i]:co[i + 1]]], 1) for i in neg]
        src = bgr[f] if name == "bgr" else c.demosaic(mos[f], BAYER_RG)
        for size in SIZES:
            got = c.source_views([f], size=size)[0]
            same = bool(np.array_equal(got, source_view_host(src, blobs, negatives, arm[offs[f]:offs[f + 1]], size)))
            ok, checked = ok and same, checked + 1
            if not same:
                print("MISMATCH %s frame %d at %dx%d" % (name, f, size[0], size[1]), file=sys.stderr)

# ---- the timed cases
side = torch.cuda.Stream(device=dev)  # (a stream of torch's, so that its events bracket the calls)
buf = torch.empty((N, SIZES[0][1], SIZES[0][0], 3), dtype=torch.uint8, device=dev)
cases = []
for size in SIZES:
    for n in COUNTS:
        for name in ("bgr", "rg"):
            cases.append(("source_%s_%dx%d_n%d" % (name, size[0], size[1], n), ("source", name, size, n)))
        cases.append(("resize_%dx%d_n%d" % (size[0], size[1], n), ("resize", "bgr", size, n)))
        for name in ("bgr", "rg"):
            cases.append(("copy_%s_%dx%d_n%d" % (name, size[0], size[1], n), ("copy", name, size, n)))
copy_src, copy_dst, BYTES = {}, {}, {}
for size in SIZES:
    for name in ("bgr", "rg"):
        BYTES[(name, size)] = contract_bytes(size[0], size[1], name == "rg")  # (once: the timed calls do no host arithmetic of their own)
        nbytes = BYTES[(name, size)][0]
        copy_src[(name, size)] = torch.zeros(N * nbytes, dtype=torch.uint8, device=dev)
        copy_dst[(name, size)] = torch.empty(N * nbytes, dtype=torch.uint8, device=dev)


def call(kind, name, size, n):
    if kind == "source":
        ctxs[name].source_views(chosen(n), dst=buf.data_ptr(), size=size, stream=side.cuda_stream)
    elif kind == "resize":
        ctxs[name].debug_views(chosen(n), size, out=buf.data_ptr(), stream=side.cuda_stream)
    else:
        nbytes = n * BYTES[(name, size)][0]
        with torch.cuda.stream(side):
            copy_dst[(name, size)][:nbytes].copy_(copy_src[(name, size)][:nbytes], non_blocking=True)


def region(spec):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(side)
    for _ in range(REPS):
        call(*spec)
    b.record(side)
    side.synchronize()
    return a.elapsed_time(b) / REPS


for _, spec in cases:  # warm-up: every shape the timed windows use
    call(*spec)
side.synchronize()
ms = {k: [] for k, _ in cases}
for r in range(REGIONS):
    k = r % len(cases)
    for key, spec in cases[k:] + cases[:k]:
        ms[key].append(region(spec))

out = {"tool": "source_view_bench", "frames": N, "w": W, "h": H, "regions": REGIONS, "reps": REPS, "flags": VIEW_ALL, "views_checked": checked, "views_equal_host": ok,
       "cases": {}}
for key, (kind, name, size, n) in cases:
    xs = np.asarray(ms[key], np.float64)
    nbytes, staged, gathered = BYTES[(name, size)]
    med = float(np.median(xs))
    out["cases"][key] = {"ms_per_call": round(med, 5), "us_per_view": round(med * 1e3 / n, 3), "spread": round(float((xs.max() - xs.min()) / med), 4),
                         "contract_bytes_per_view": nbytes, "contract_TB_per_s": round(n * nbytes / (med * 1e-3) / 1e12, 4)}
    if kind == "source":
        out["cases"][key].update({"tiles_staged": staged, "tiles_gathered": gathered})
for c in ctxs.values():
    c.close()
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(line + "\n")
print(line, flush=True)
sys.exit(0 if ok else 1)
