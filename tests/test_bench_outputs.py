"""bench.py's plain run and --dump-outputs: a plain run times exactly --steps steps and reports the metric alone (the side
measurements are behind --full); --dump-outputs writes the last timed step's armour lists, which equal the oracle's on that
step's frames."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rmcv_amd import ARMOUR, CAMP_BLUE, STAGE_ALL, STAGE_IDENTITY, STAGE_POSE, synth  # noqa: E402


def test_plain_and_full_arguments():
    a = bench.parse_args(["--steps", "50"])
    assert (a.full, a.repeats, a.dump_outputs, a.steps) == (False, 1, None, 50)
    assert bench.parse_args(["--full"]).repeats == 7
    assert bench.parse_args(["--full", "--repeats", "3"]).repeats == 3
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--roofline-only", "--dump-outputs", "d"])


def test_write_outputs_names_and_dtypes(tmp_path):
    arm = np.zeros(3, ARMOUR)
    arm["vertices"] = np.arange(24, dtype=np.float32).reshape(3, 4, 2) + 0.5
    arm["icon"] = -arm["vertices"]
    arm["bbox"] = np.arange(12, dtype=np.float32).reshape(3, 4)
    arm["blob_i"], arm["blob_j"] = [0, 2, 1], [1, 3, 4]
    offs = np.array([0, 1, 3, 3], np.int32)
    bench.write_outputs(str(tmp_path / "a"), arm, offs, None, STAGE_ALL)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sorted(got) == ["armour_bbox", "armour_blob_i", "armour_blob_j", "armour_frame_offsets", "armour_icon", "armour_vertices"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["armour_vertices"], arm["vertices"]) and got["armour_vertices"].dtype == np.float32
    assert np.array_equal(got["armour_icon"], arm["icon"]) and np.array_equal(got["armour_bbox"], arm["bbox"])
    assert got["armour_blob_j"].tolist() == [1, 3, 4] and got["armour_frame_offsets"].tolist() == [0, 1, 3, 3]
    # a classify / pose stage: the context's identities and poses, in the order of the lists
    ctx = types.SimpleNamespace(identities=lambda: np.array([5, 0, 2], np.int32),
                                poses=lambda: tuple(np.full((3, 3), k, np.float64) for k in range(3)))
    bench.write_outputs(str(tmp_path / "b"), arm, offs, ctx, STAGE_ALL | STAGE_IDENTITY | STAGE_POSE)
    assert np.load(str(tmp_path / "b" / "armour_identity.npy")).tolist() == [5, 0, 2]
    assert np.load(str(tmp_path / "b" / "armour_position.npy")).dtype == np.float64
    assert np.load(str(tmp_path / "b" / "armour_position.npy"))[0, 0] == 2


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(oracle, tmp_path):
    """16 frames per step, 3 timed steps: the timed region starts on frame set 0, so its last step runs on frame set 2"""
    steps, n = 3, 16
    out_dir = tmp_path / "out"
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                         "--frames", str(n), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-2000:]
    line = json.loads(cp.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["timed_region"]["repeats"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - n * steps / (line["ms_per_step"] * steps * 1e-3)) < 0.01 * line["value"]
    assert not {"roofline", "stage_ms", "lone_batch_ms", "cpu_baseline", "c5", "density_sweep"} & set(line)
    frames = synth.batch(2 * 1000003, n, 1280, 1024, CAMP_BLUE, 0, threads=16)
    refs = [oracle.detect_frame(f)["armours"] for f in frames]
    offs = np.load(str(out_dir / "armour_frame_offsets.npy"))
    assert offs.tolist() == np.cumsum([0] + [len(r) for r in refs]).tolist()
    assert offs[-1] > 0
    ref = np.concatenate(refs)
    for field in ("vertices", "icon", "bbox", "blob_i", "blob_j"):
        got = np.load(str(out_dir / ("armour_%s.npy" % field)))
        assert np.array_equal(got, ref[field]), field
