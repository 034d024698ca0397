"""Writes tests/golden/track_hypot_pairs.json: the (p, beta) arguments of hypot in the Jacobi rotation over the scenarios of
tests/track_scenarios.py, recorded from the tests' reference (tests/track_ref.py); an even sample of the distinct pairs, NaN ones kept.
Run from the repository root:  python tests/golden/make_track_hypot_pairs.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import track_ref as R  # noqa: E402
import track_scenarios as S  # noqa: E402

pairs = []
for name, (over, steps) in sorted(S.scenarios().items()):
    ref = R.RefStream(R.lib(), roi_scale=(over.get("roi_scale_w", 1.0), over.get("roi_scale_h", 1.0)),
                      noise=(over.get("process_noise", 5e-5), over.get("measurement_noise", 0.5), over.get("error", 0.05)), win=(over["win_w"], over["win_h"]))
    with R.HypotRecorder() as rec:
        for arm, ids, pos, ts in steps:
            ref.step(arm, ids, pos, ts)
    print(name, len(rec.pairs))
    pairs.append(rec.pairs)
p = np.concatenate(pairs)
_, first = np.unique(p.view(np.uint64).reshape(-1, 2), axis=0, return_index=True)
p = p[np.sort(first)]
nan = ~np.isfinite(p).all(1)
keep = np.concatenate([p[nan][:100], p[~nan][:: max(1, int((~nan).sum()) // 2000)]])
with open(os.path.join(HERE, "track_hypot_pairs.json"), "w") as f:
    json.dump({"source": "tests/golden/make_track_hypot_pairs.py", "pairs": [[float(a).hex(), float(b).hex()] for a, b in keep]}, f, indent=0)
print(len(p), "distinct,", len(keep), "kept,", int(nan.sum()), "with NaN")
