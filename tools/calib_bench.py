"""What the calibration solve costs, written as ONE JSON line to profiles/calib_bench.json (or the path given) and to stdout.
The shape of the reference's own calibration session (executable/calibration/hand_eye.cpp): 120 views of an 11 x 8 board (88 corners), square
30, a 1280 x 1024 image; the sessions are tests/calib_cases.py's recipe (the camera of executable/main.cpp, corners rounded to float32).
  device   rmcv_calibrate_cameras on device tables of the caller's, between device events on a side stream, for one camera (120 views) and
           for 16 cameras in one call (1920 views, every camera its own session).  REGIONS regions of REPS calls, the arms alternating from
           region to region; a region's figure is the mean of its calls.
  host     rmcv_calibrate_camera_host on the one camera's session, one thread, host clock, the median of 5 calls
Reported per arm: ms per call (median over the regions, spread), iterations.  No threshold is set: there is no earlier device path, one
workgroup works per camera, and a single camera need not beat the host.  The only pass condition: the device's results and view records
equal the host function's byte for byte (exit status 1 otherwise).
python tools/calib_bench.py [out.json] [--regions N] [--reps N] [--views N] [--cameras N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, COLS, ROWS, SQUARE = 1280, 1024, 11, 8, 30.0


def options(argv):
    opt = {"out": os.path.join(ROOT, "profiles", "calib_bench.json"), "regions": 5, "reps": 20, "views": 120, "cameras": 16}
    k = 0
    while k < len(argv):
        if argv[k] in ("--regions", "--reps", "--views", "--cameras"):
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


def main():
    opt = options(sys.argv[1:])
    import numpy as np
    import torch  # (before the library initialises HIP: the tensors below are torch's)

    import calib_cases as CC
    from rmcv_amd import Context, abi, calibrate_camera_host
    V, NCAM, REGIONS, REPS = opt["views"], opt["cameras"], opt["regions"], opt["reps"]
    per = COLS * ROWS
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    sessions = [CC.session(9000 + k, V, COLS, ROWS, SQUARE)[0] for k in range(NCAM)]
    counts1 = np.full(V, per, np.int32)
    host_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        calibrate_camera_host(sessions[0], counts1, COLS, ROWS, SQUARE, (W, H))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    want = [calibrate_camera_host(s, counts1, COLS, ROWS, SQUARE, (W, H)) for s in sessions]
    stream = torch.cuda.Stream(device=dev)
    c = Context(device=0, max_frames=1, max_width=W, max_height=H)
    arms = {}
    for name, ncam in (("one_camera", 1), ("%d_cameras" % NCAM, NCAM)):
        # the fleet's views interleaved: view v belongs to camera v % ncam
        cor = np.stack([sessions[v % ncam][v // ncam] for v in range(V * ncam)])
        cam = (np.arange(V * ncam) % ncam).astype(np.int32)
        res0, views0 = abi.calib_outputs(ncam, V * ncam)
        arms[name] = {"n_cameras": ncam, "cor": torch.from_numpy(cor).to(dev), "cnt": torch.full((V * ncam,), per, dtype=torch.int32, device=dev),
                      "cam": torch.from_numpy(cam).to(dev), "res": torch.from_numpy(res0.view(np.uint8)).to(dev), "views": torch.from_numpy(views0.view(np.uint8)).to(dev),
                      "ms": []}
    torch.cuda.synchronize()

    def region(arm):
        pairs = []
        with torch.cuda.stream(stream):
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                c.calibrate_cameras(arm["cor"].data_ptr(), arm["cnt"].data_ptr(), COLS, ROWS, SQUARE, (W, H), view_camera=arm["cam"].data_ptr(), n_cameras=arm["n_cameras"],
                                    results=arm["res"].data_ptr(), views=arm["views"].data_ptr(), per_frame=per, n_views=V * arm["n_cameras"], stream=stream.cuda_stream)
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
    ok = True
    out = {"tool": "calib_bench", "views_per_camera": V, "w": W, "h": H, "cols": COLS, "rows": ROWS, "square": SQUARE, "regions": REGIONS, "reps": REPS, "arms": {}}
    for name, arm in arms.items():
        ncam = arm["n_cameras"]
        res = arm["res"].cpu().numpy().view(abi.CALIB_RESULT)
        views = arm["views"].cpu().numpy().view(abi.CALIB_VIEW)
        for k in range(ncam):
            ok = ok and res[k].tobytes() == want[k][0].rec.tobytes() and views[k::ncam].tobytes() == want[k][1].tobytes()
        s = stats(arm["ms"])
        s.update({"n_cameras": ncam, "views": V * ncam, "iters": [int(i) for i in res["iters"]], "status": [int(i) for i in res["status"]],
                  "rms_max": float(res["rms"].max()), "ms_per_camera": round(s["ms"] / ncam, 5)})
        out["arms"][name] = s
    c.close()
    out["device_equals_host"] = bool(ok)
    out["host_single_thread"] = {"ms": round(float(np.median(host_ms)), 3), "calls": 5, "iters": want[0][0].iters}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
