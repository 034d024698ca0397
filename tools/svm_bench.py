#!/usr/bin/env python3
"""Training the icon classifier, device against host (not bench.py): rmcv_svm_train on one GPU and rmcv_svm_train_host on the
CPU, on one seeded 7-class set of about 2000 rows at the default parameters (eps 1e-3, max_iter 1000, 10 folds, six C values: 1281 pair
problems).  Reports the wall time of both calls and the phases each reports (GPU time between events on the device, wall time on the
host), names the dominant kernel, checks that the two models agree bit for bit, and writes profiles/svm_bench.json.

    python tools/svm_bench.py [--rows-per-class 286] [--noise 110] [--repeats 3] [--out profiles/svm_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_OF = {"gram": "k_svm_gram", "search_smo": "k_svm_smo", "search_weights": "k_svm_weights", "search_predict": "k_svm_predict", "final_smo": "k_svm_smo",
             "final_weights": "k_svm_weights"}


def dataset(rows_per_class, noise, seed=1):
    rng = np.random.RandomState(seed)
    protos = rng.randint(0, 256, (7, 1200))
    rows = np.concatenate([np.clip(protos[k] + rng.randint(-noise, noise + 1, (rows_per_class, 1200)), 0, 255) for k in range(7)]).astype(np.uint8)
    return rows, np.repeat(np.arange(7), rows_per_class).astype(np.int32), rng.permutation(len(rows)).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-class", type=int, default=286)
    ap.add_argument("--noise", type=int, default=110)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svm_bench.json"))
    a = ap.parse_args()
    from rmcv_amd import OPT_WAIT_TIMEOUT_MS, Context, svm
    rows, resp, perm = dataset(a.rows_per_class, a.noise)
    ctx = Context(device=0, max_frames=1)
    ctx.set_option(OPT_WAIT_TIMEOUT_MS, 60000)                   # sets of other sizes may take longer than the default deadline
    dev_runs = []
    for _ in range(a.repeats):                                   # the first run pays for loading the kernels
        t0 = time.perf_counter()
        dev = svm.train_auto(rows, resp, perm, ctx=ctx)
        dev_runs.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "phase_ms": dev.report["phase_ms"]})
    t0 = time.perf_counter()
    host = svm.train_auto(rows, resp, perm)
    host_run = {"wall_ms": (time.perf_counter() - t0) * 1e3, "phase_ms": host.report["phase_ms"]}
    ctx.close()
    same = (dev.weights.tobytes() == host.weights.tobytes() and dev.rho.tobytes() == host.rho.tobytes() and dev.report["cv_errors"] == host.report["cv_errors"]
            and dev.report["best_index"] == host.report["best_index"])
    best = min(dev_runs[1:] or dev_runs, key=lambda r: r["wall_ms"])
    by_kernel = {}
    for phase, ms in best["phase_ms"].items():
        by_kernel[KERNEL_OF[phase]] = by_kernel.get(KERNEL_OF[phase], 0.0) + ms
    result = {"rows": len(rows), "classes": 7, "pair_problems": (6 * 10 + 1) * 21, "params": "defaults", "device_runs": dev_runs, "device_best": best, "host": host_run,
              "device_kernel_ms": by_kernel, "dominant_kernel": max(by_kernel, key=by_kernel.get),
              "gram_ms": {"device": best["phase_ms"]["gram"], "host": host_run["phase_ms"]["gram"]},
              "solver_ms": {"device": best["phase_ms"]["search_smo"] + best["phase_ms"]["final_smo"], "host": host_run["phase_ms"]["search_smo"] + host_run["phase_ms"]["final_smo"]},
              "total_ms": {"device": best["wall_ms"], "host": host_run["wall_ms"]}, "host_over_device": host_run["wall_ms"] / best["wall_ms"],
              "bit_identical": bool(same), "best_c": dev.report["best_c"], "cv_errors": dev.report["cv_errors"],
              "iterations_final": [int(v) for v in dev.report["iterations"]]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("rows", "gram_ms", "solver_ms", "total_ms", "host_over_device", "dominant_kernel", "bit_identical")}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
