"""What the chessboard detector costs, written as ONE JSON line to profiles/chess_bench.json (or the path given) and to stdout.
The shape of the reference's own calibration session (executable/calibration/hand_eye.cpp): 120 resident frames of 1280 x 1024 with an 11 x 8
board (88 inner corners) in each, the detector's default parameters.
  device   rmcv_batch_find_chessboards for the 120 frames into device tables of the caller's, between device events on a side stream, for BGR
           frames, for the same frames as an 8-bit RG mosaic, and for blank BGR frames -- no candidates, so k_chess_grid has nothing to do and
           the call is the memset, k_chess_response and an idle launch: the figure taken for the response kernel.  REGIONS regions of REPS
           calls, the arms alternating from region to region; a region's figure is the mean of its calls.
  host     rmcv_find_chessboard_host over the same 120 frames, one thread, host clock
Reported per arm: ms per call (median over the regions, spread); for the blank arm the byte bound (120 x 1280 x 1024 x 3 B at 6.3 TB/s, the
achievable HBM rate) over its time.  No threshold is set: there is no earlier device path.  The only pass condition: the device's corners,
counts and status words of the BGR batch equal the host function's (exit status 1 otherwise).
python tools/chess_bench.py [out.json] [--regions N] [--reps N] [--frames N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, COLS, ROWS = 1280, 1024, 11, 8
DISTINCT = 8                              # boards rendered; the batch cycles through them
HBM_BYTES_PER_S = 6.3e12


def options(argv):
    opt = {"out": os.path.join(ROOT, "profiles", "chess_bench.json"), "regions": 5, "reps": 20, "frames": 120}
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
    """frames (n, H, W, 3): DISTINCT boards under different homographies (tools/corner_bench.py's), cycled"""
    import numpy as np

    from rmcv_amd import synth
    imgs = []
    for k in range(DISTINCT):
        s, a = 60.0 + 3.0 * k, 0.02 * (k - 3)
        Hm = np.array([[s * np.cos(a), -s * np.sin(a), 150.0 + 11.0 * k], [s * np.sin(a), s * np.cos(a), 140.0 + 7.0 * k], [2.0e-5 * k, 1.0e-5 * (k - 4), 1.0]])
        imgs.append(synth.chessboard(W, H, Hm, COLS + 1, ROWS + 1, ss=2)[0])
    return np.stack([imgs[f % DISTINCT] for f in range(n_frames)])


def main():
    opt = options(sys.argv[1:])
    import numpy as np
    import torch  # (before the library initialises HIP: the tensors below are torch's)

    from rmcv_amd import BAYER_RG, CHESS_FOUND, Context, find_chessboard_host, synth
    N, REGIONS, REPS = opt["frames"], opt["regions"], opt["reps"]
    per = COLS * ROWS
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    frames = boards(N)
    chosen = np.arange(N, dtype=np.int32)
    t0 = time.perf_counter()
    host = [find_chessboard_host(frames[f], COLS, ROWS) for f in range(N)]
    host_ms = (time.perf_counter() - t0) * 1e3
    want = np.stack([np.full((per, 2), np.nan, np.float32) if h[0] is None else h[0] for h in host])
    want_st = np.array([h[1] for h in host], np.int32)
    want_cnt = np.where(want_st & CHESS_FOUND, per, 0).astype(np.int32)
    stream = torch.cuda.Stream(device=dev)
    arms = {}
    for name, fmt, data in (("bgr", 0, frames), ("mosaic_rg", BAYER_RG, synth.mosaic(frames, BAYER_RG)), ("blank_bgr", 0, np.full_like(frames, 215))):
        c = Context(device=0, max_frames=N, max_width=W, max_height=H)
        if fmt:
            c.set_input_format(fmt)
        d_frames = torch.from_numpy(data).to(dev)
        c.bind_device_frames(d_frames.data_ptr(), N, H, W, keepalive=d_frames)
        arms[name] = {"ctx": c, "tab": torch.full((N, per, 2), float("nan"), dtype=torch.float32, device=dev), "counts": torch.zeros(N, dtype=torch.int32, device=dev),
                      "status": torch.zeros(N, dtype=torch.int32, device=dev), "ms": []}
    torch.cuda.synchronize()

    def region(arm):
        c = arm["ctx"]
        pairs = []
        with torch.cuda.stream(stream):
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                c.find_chessboards(chosen, COLS, ROWS, corners=arm["tab"].data_ptr(), per_frame=per, counts=arm["counts"].data_ptr(), status=arm["status"].data_ptr(),
                                   stream=stream.cuda_stream)
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
    got, got_cnt, got_st = (arms["bgr"][k].cpu().numpy() for k in ("tab", "counts", "status"))
    ok = got.tobytes() == want.tobytes() and got_cnt.tolist() == want_cnt.tolist() and got_st.tolist() == want_st.tolist()
    bound_ms = N * W * H * 3 / HBM_BYTES_PER_S * 1e3
    out = {"tool": "chess_bench", "frames": N, "w": W, "h": H, "cols": COLS, "rows": ROWS, "regions": REGIONS, "reps": REPS, "device_equals_host": ok,
           "boards_found_host": int((want_cnt > 0).sum()), "byte_bound_ms_at_6.3_TB_s": round(bound_ms, 5), "arms": {}}
    for name, arm in arms.items():
        s = stats(arm["ms"])
        s.update({"boards_found": int((arm["counts"].cpu().numpy() > 0).sum()), "candidates": int((arm["status"].cpu().numpy() & 0x7FF).sum()),
                  "us_per_frame": round(s["ms"] * 1e3 / N, 4)})
        if name == "blank_bgr":
            s["byte_bound_over_time"] = round(bound_ms / s["ms"], 4)
        out["arms"][name] = s
        arm["ctx"].close()
    out["host_single_thread"] = {"ms": round(host_ms, 3), "ms_per_frame": round(host_ms / N, 3)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
