"""What the hand-eye solve costs, written as ONE JSON line to profiles/handeye_bench.json (or the path given) and to stdout.
The sessions are tests/handeye_cases.py's recipe (the mounting of executable/main.cpp, a board 1.5 m out, clean poses).
  device   rmcv_calibrate_hand_eyes on device tables of the caller's, between device events on a side stream, for the reference's session
           shape (120 views, one camera), for 16 cameras x 120 views in one call (every camera its own session, views interleaved) and
           for one camera at the cap (256 views, 32640 pairs).  REGIONS regions of REPS calls, the arms alternating from region to region; a
           region's figure is the mean of its calls.
  host     rmcv_calibrate_hand_eye_host on the 120-view and the 256-view session, one thread, host clock, the median of 5 calls
Reported per arm: ms per call (median over the regions, spread).  No threshold is set: there is no earlier device path, one workgroup works
per camera, and a single camera need not beat the host.  The only pass condition: in every arm the device's results and view rows equal the
host function's byte for byte (exit status 1 otherwise).
python tools/handeye_bench.py [out.json] [--regions N] [--reps N] [--views N] [--cameras N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def options(argv):
    opt = {"out": os.path.join(ROOT, "profiles", "handeye_bench.json"), "regions": 5, "reps": 20, "views": 120, "cameras": 16}
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

    import handeye_cases as HC
    from rmcv_amd import Context, abi, calibrate_hand_eye_host
    V, NCAM, REGIONS, REPS, CAP = opt["views"], opt["cameras"], opt["regions"], opt["reps"], abi.CALIB_VIEWS_PER_CAMERA_MAX
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    sessions = [HC.session(9100 + k, V)[:2] for k in range(NCAM)]
    capped = HC.session(9200, CAP)[:2]

    def host_ms(s):
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            calibrate_hand_eye_host(*s)
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ms)), 4)

    host = {"%d_views" % V: host_ms(sessions[0]), "%d_views" % CAP: host_ms(capped)}
    stream = torch.cuda.Stream(device=dev)
    c = Context(device=0, max_frames=1, max_width=64, max_height=64)
    arms = {}
    for name, group in (("one_camera", sessions[:1]), ("%d_cameras" % NCAM, sessions), ("%d_views" % CAP, [capped])):
        # a fleet's views interleaved: view v belongs to camera v % ncam
        ncam, per = len(group), len(group[0][0])
        views = np.stack([group[v % ncam][0][v // ncam] for v in range(per * ncam)])
        att = np.stack([group[v % ncam][1][v // ncam] for v in range(per * ncam)])
        cam = (np.arange(per * ncam) % ncam).astype(np.int32)
        res0, rows0 = abi.handeye_outputs(ncam, per * ncam)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
        arms[name] = {"n_cameras": ncam, "n_views": per * ncam, "views": up(views), "att": up(att), "cam": torch.from_numpy(cam).to(dev), "res": up(res0), "rows": up(rows0),
                      "want": [calibrate_hand_eye_host(*s) for s in group], "ms": []}
    torch.cuda.synchronize()

    def region(arm):
        pairs = []
        with torch.cuda.stream(stream):
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                c.calibrate_hand_eyes(arm["views"].data_ptr(), arm["att"].data_ptr(), view_camera=arm["cam"].data_ptr(), n_cameras=arm["n_cameras"],
                                      results=arm["res"].data_ptr(), rows=arm["rows"].data_ptr(), n_views=arm["n_views"], stream=stream.cuda_stream)
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
    out = {"tool": "handeye_bench", "views_per_camera": V, "regions": REGIONS, "reps": REPS, "arms": {}}
    for name, arm in arms.items():
        ncam = arm["n_cameras"]
        res = arm["res"].cpu().numpy().view(abi.HANDEYE_RESULT)
        rows = arm["rows"].cpu().numpy().view(abi.HANDEYE_VIEW)
        same = True
        for k in range(ncam):
            same = same and res[k].tobytes() == np.array(arm["want"][k][0].rec).tobytes() and rows[k::ncam].tobytes() == arm["want"][k][1].tobytes()
        ok = ok and same
        s = stats(arm["ms"])
        s.update({"n_cameras": ncam, "views": arm["n_views"], "pairs": int(res["pairs_used"].sum()), "status": [int(i) for i in res["status"]],
                  "sweeps": [int(i) for i in res["sweeps"]], "ms_per_camera": round(s["ms"] / ncam, 5), "device_equals_host": bool(same)})
        out["arms"][name] = s
    c.close()
    out["device_equals_host"] = bool(ok)
    out["host_single_thread_ms"] = host
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
