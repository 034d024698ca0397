"""What the corner refinement costs, written as ONE JSON line to profiles/corner_bench.json (or the path given) and to stdout.
The shape of the reference's own calibration session (executable/calibration/hand_eye.cpp): 120 resident frames of 1280 x 1024, a board with
88 inner corners in each, cornerSubPix(win 8, 40 iterations, eps 0.001), guesses up to +-2.5 px off.
  device   rmcv_batch_refine_corners for the 120 frames into a device table of the caller's, between device events on a side stream, for BGR
           frames and for the same frames as an 8-bit RG mosaic: REGIONS regions of REPS calls, the two arms alternating from region to region.
           The corners are refined in place, so every call is preceded by a device copy that restores the guesses; the events sit behind that
           copy and behind the call, and a region's figure is the mean of its calls.
  host     rmcv_corner_subpix_host over the same 120 x 88 guesses, one thread, host clock
Reported per arm: ms per call (median over the regions, spread), the corner-iterations of a call (the sum of the status words' counts) and ns per
corner-iteration.  No threshold is set: there is no earlier device path.  The only pass condition: the device's corners and status words of
the BGR batch equal the host function's (exit status 1 otherwise).
python tools/corner_bench.py [out.json] [--regions N] [--reps N] [--frames N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NX, NY = 1280, 1024, 12, 9          # 12 x 9 squares: 11 x 8 = 88 inner corners
WIN, ZERO, ITERS, EPS = (8, 8), (-1, -1), 40, 0.001
DISTINCT = 8                              # boards rendered; the batch cycles through them with guesses of its own per frame


def options(argv):
    opt = {"out": os.path.join(ROOT, "profiles", "corner_bench.json"), "regions": 5, "reps": 20, "frames": 120}
    k = 0
    while k < len(argv):
        if argv[k] in ("--regions", "--reps", "--frames"):
            opt[argv[k][2:]] = int(argv[k + 1])
            k += 2
        else:
            opt["out"] = argv[k]
            k += 1
    return opt


def stats(xs):
    import numpy as np
    xs = np.asarray(xs, np.float64)
    med = float(np.median(xs))
    return {"ms": round(med, 5), "spread": round(float((xs.max() - xs.min()) / med), 4), "regions": [round(float(x), 5) for x in xs]}


def boards(n_frames):
    """(frames (n, H, W, 3), guesses (n, 88, 2) float32): DISTINCT boards under different homographies, cycled"""
    import numpy as np

    from rmcv_amd import synth
    rng = np.random.default_rng(20241021)
    imgs, truths = [], []
    for k in range(DISTINCT):
        s, a = 60.0 + 3.0 * k, 0.02 * (k - 3)
        Hm = np.array([[s * np.cos(a), -s * np.sin(a), 150.0 + 11.0 * k], [s * np.sin(a), s * np.cos(a), 140.0 + 7.0 * k], [2.0e-5 * k, 1.0e-5 * (k - 4), 1.0]])
        img, t = synth.chessboard(W, H, Hm, NX, NY, ss=2)
        imgs.append(img)
        truths.append(t)
    frames = np.stack([imgs[f % DISTINCT] for f in range(n_frames)])
    guesses = np.stack([truths[f % DISTINCT] + rng.uniform(-2.5, 2.5, truths[0].shape) for f in range(n_frames)]).astype(np.float32)
    return frames, guesses


def main():
    opt = options(sys.argv[1:])
    import numpy as np
    import torch  # (before the library initialises HIP: the tensors below are torch's)

    from rmcv_amd import BAYER_RG, Context, corner_subpix_host, synth
    N, REGIONS, REPS = opt["frames"], opt["regions"], opt["reps"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    frames, guesses = boards(N)
    per = guesses.shape[1]
    chosen = np.arange(N, dtype=np.int32)
    t0 = time.perf_counter()
    host = [corner_subpix_host(frames[f], guesses[f], WIN, ZERO, ITERS, EPS) for f in range(N)]
    host_ms = (time.perf_counter() - t0) * 1e3
    want, want_st = np.stack([h[0] for h in host]), np.stack([h[1] for h in host])
    stream = torch.cuda.Stream(device=dev)
    d_guess = torch.from_numpy(guesses).to(dev)
    arms = {}
    for name, fmt, data in (("bgr", 0, frames), ("mosaic_rg", BAYER_RG, synth.mosaic(frames, BAYER_RG))):
        c = Context(device=0, max_frames=N, max_width=W, max_height=H)
        if fmt:
            c.set_input_format(fmt)
        d_frames = torch.from_numpy(data).to(dev)
        c.bind_device_frames(d_frames.data_ptr(), N, H, W, keepalive=d_frames)
        arms[name] = {"ctx": c, "tab": torch.empty_like(d_guess), "status": torch.zeros((N, per), dtype=torch.int32, device=dev), "ms": []}
    torch.cuda.synchronize()

    def region(arm):
        c, tab, status = arm["ctx"], arm["tab"], arm["status"]
        pairs = []
        with torch.cuda.stream(stream):
            for _ in range(REPS):
                tab.copy_(d_guess)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                c.refine_corners(chosen, tab.data_ptr(), None, WIN, ZERO, ITERS, EPS, status=status.data_ptr(), per_frame=per, stream=stream.cuda_stream)
                b.record(stream)
                pairs.append((a, b))
        stream.synchronize()
        return sum(a.elapsed_time(b) for a, b in pairs) / REPS

    for arm in arms.values():  # warm: every shape the timed windows use
        region(arm)
    names = list(arms)
    for r in range(REGIONS):
        for name in (names if r % 2 == 0 else names[::-1]):
            arms[name]["ms"].append(region(arms[name]))
    got, got_st = arms["bgr"]["tab"].cpu().numpy(), arms["bgr"]["status"].cpu().numpy()
    ok = got.tobytes() == want.tobytes() and got_st.tolist() == want_st.tolist()
    out = {"tool": "corner_bench", "frames": N, "w": W, "h": H, "corners_per_frame": per, "win": list(WIN), "max_iters": ITERS, "eps": EPS, "regions": REGIONS, "reps": REPS,
           "device_equals_host": ok, "arms": {}}
    for name, arm in arms.items():
        iters = int((arm["status"].cpu().numpy() & 0xFF).sum())
        s = stats(arm["ms"])
        s.update({"corner_iterations": iters, "ns_per_corner_iteration": round(s["ms"] * 1e6 / max(iters, 1), 3), "us_per_corner": round(s["ms"] * 1e3 / (N * per), 4)})
        out["arms"][name] = s
        arm["ctx"].close()
    host_iters = int((want_st & 0xFF).sum())
    out["host_single_thread"] = {"ms": round(host_ms, 3), "corner_iterations": host_iters, "ns_per_corner_iteration": round(host_ms * 1e6 / max(host_iters, 1), 3)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
