"""What the icon strip and the labeler's sheet cost, written as ONE JSON line to profiles/icon_strip_bench.json (or the path
given) and to stdout.  256 resident 1280x1024 frames through RMCV_STAGE_ALL; 8 of them chosen:
  strips    rmcv_batch_icon_strips for the 8 views, cap 16, at side 20 and at side 80: REGIONS regions of REPS calls between device events on
            a side stream (median, spread), the two sides alternating from region to region
  pipeline  a pipeline step (submit .. drained, STEPS batches a region) with sheets off and with sheets on (8 sheets at 640x512, side 80),
            the two arms alternating from region to region
Every build is measured in a process of its own (a library is loaded once per process), the builds taking turns for ROUNDS rounds:
  --variant NAME=PATH   another build of librmcv_hip.so beside this tree's -- the kernel with the other store variant, or the parent commit's
                        library.  A build without the strip's entry points (the parent's) is timed with sheets off only: what a submit
                        enqueues then is what it enqueued before, so its step time has to sit within the regions' own spread.
No threshold is set.  The only pass condition: the strips of two frames equal rmcv_icon_strip_host (exit status 1 otherwise).
python tools/icon_strip_bench.py [out.json] [--variant NAME=PATH ...] [--rounds R] [--regions N] [--reps N] [--steps N]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, W, H = 256, 1280, 1024
CHOSEN = [0, 37, 74, 111, 148, 185, 222, 255]
SIDES, CAP = (20, 80), 16
SHEET_VIEW, SHEET_SIDE = (640, 512), 80


def options(argv):
    opt = {"out": os.path.join(ROOT, "profiles", "icon_strip_bench.json"), "variants": [], "rounds": 2, "regions": 5, "reps": 200, "steps": 8, "child": False}
    k = 0
    while k < len(argv):
        a = argv[k]
        if a == "--variant":
            name, path = argv[k + 1].split("=", 1)
            opt["variants"].append((name, os.path.abspath(path)))
            k += 2
        elif a in ("--rounds", "--regions", "--reps", "--steps"):
            opt[a[2:]] = int(argv[k + 1])
            k += 2
        elif a == "--child":
            opt["child"] = True
            k += 1
        else:
            opt["out"] = a
            k += 1
    return opt


def stats(xs):
    import numpy as np
    xs = np.asarray(xs, np.float64)
    med = float(np.median(xs))
    return {"ms": round(med, 5), "spread": round(float((xs.max() - xs.min()) / med), 4), "regions": [round(float(x), 5) for x in xs]}


def child(opt):
    """one build (RMCV_LIB_PATH, or this tree's), one process: a dict of raw region times"""
    import numpy as np
    import torch  # (before the library initialises HIP: the tensors below are torch's)

    from rmcv_amd import CAMP_BLUE, STAGE_ALL, VIEW_ALL, Context, Pipeline, default_params, synth
    from rmcv_amd import abi
    REGIONS, REPS, STEPS = opt["regions"], opt["reps"], opt["steps"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    p = default_params()
    has_strips = hasattr(abi.lib(), "rmcv_batch_icon_strips")
    frames = synth.batch(1000003, N, W, H, CAMP_BLUE, 0, threads=16)
    d_frames = torch.from_numpy(frames).to(dev)
    chosen = np.asarray(CHOSEN, np.int32)
    res = {"has_strips": has_strips, "strips": {}, "pipeline_step": {}}
    ok = True
    if has_strips:
        from rmcv_amd import icon_strip_host
        c = Context(device=0, max_frames=N, max_width=W, max_height=H)
        c.bind_device_frames(d_frames.data_ptr(), N, H, W, keepalive=d_frames)
        c.run(p, STAGE_ALL)
        c.sync()
        arm, offs = c.armours()
        res["armours_of_chosen"] = [int(offs[f + 1] - offs[f]) for f in CHOSEN]
        for side in SIDES:  # the pass condition
            got = c.icon_strips(chosen[:2], side, CAP)
            for k, f in enumerate(CHOSEN[:2]):
                same = bool(np.array_equal(got[k], icon_strip_host(frames[f], arm[offs[f]:offs[f + 1]], side, CAP)))
                ok = ok and same
                if not same:
                    print("MISMATCH frame %d at side %d" % (f, side), file=sys.stderr)
        stream = torch.cuda.Stream(device=dev)
        bufs = {s: torch.empty((len(CHOSEN), s, CAP * s, 3), dtype=torch.uint8, device=dev) for s in SIDES}

        def region(side):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(REPS):
                c.icon_strips(chosen, side, CAP, dst=bufs[side].data_ptr(), stream=stream.cuda_stream)
            b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b) / REPS
        for side in SIDES:  # warm: every shape the timed windows use
            region(side)
        ms = {s: [] for s in SIDES}
        for r in range(REGIONS):
            for side in (SIDES if r % 2 == 0 else SIDES[::-1]):
                ms[side].append(region(side))
        res["strips"] = {"side_%d" % s: ms[s] for s in SIDES}
        c.close()
    pl = Pipeline(device=0, max_frames=N, max_width=W, max_height=H)
    arms = [("sheets_off", False)] + ([("sheets_on", True)] if has_strips else [])

    def pipeline_region(on):
        if has_strips:
            pl.set_sheets(chosen if on else None, SHEET_VIEW, SHEET_SIDE, VIEW_ALL)  # (drains)
        for _ in range(2):  # warm: the arm's first batches
            pl.submit(d_frames.data_ptr(), N, H, W, p, STAGE_ALL)
        pl.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            pl.submit(d_frames.data_ptr(), N, H, W, p, STAGE_ALL)
        pl.drain()
        return (time.perf_counter() - t0) * 1e3 / STEPS
    step = {name: [] for name, _ in arms}
    for r in range(REGIONS):
        for name, on in (arms if r % 2 == 0 else arms[::-1]):
            step[name].append(pipeline_region(on))
    res["host_blocking_calls"] = int(pl.get_info().host_blocking_calls)
    pl.close()
    res["pipeline_step"] = step
    res["strips_equal_host"] = ok
    return res


def main():
    opt = options(sys.argv[1:])
    if opt["child"]:
        print("RESULT " + json.dumps(child(opt)), flush=True)
        return 0
    builds = [("this_tree", None)] + opt["variants"]
    raw = {name: [] for name, _ in builds}
    for _ in range(opt["rounds"]):  # the builds take turns: a drift of the machine falls on all of them
        for name, path in builds:
            env = dict(os.environ)
            if path:
                env["RMCV_LIB_PATH"] = path
            cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sum([["--" + k, str(opt[k])] for k in ("regions", "reps", "steps")], [])
            done = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
            if done.returncode or not line:
                sys.stderr.write(done.stdout + done.stderr)
                print("the run of build %s ended with status %d" % (name, done.returncode), file=sys.stderr)
                return 1
            raw[name].append(json.loads(line[0][7:]))
    out = {"tool": "icon_strip_bench", "frames": N, "w": W, "h": H, "chosen": CHOSEN, "cap": CAP, "sheet_view": list(SHEET_VIEW), "sheet_side": SHEET_SIDE,
           "rounds": opt["rounds"], "regions": opt["regions"], "reps": opt["reps"], "steps": opt["steps"], "builds": {}}
    ok = True
    for name, _ in builds:
        runs = raw[name]
        ok = ok and all(r["strips_equal_host"] for r in runs)
        b = {"has_strips": runs[0]["has_strips"], "strips_equal_host": all(r["strips_equal_host"] for r in runs),
             "host_blocking_calls": max(r["host_blocking_calls"] for r in runs), "armours_of_chosen": runs[0].get("armours_of_chosen"),
             "strips": {k: stats(sum([r["strips"][k] for r in runs], [])) for k in runs[0]["strips"]},
             "pipeline_step": {k: stats(sum([r["pipeline_step"][k] for r in runs], [])) for k in runs[0]["pipeline_step"]}}
        out["builds"][name] = b
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
