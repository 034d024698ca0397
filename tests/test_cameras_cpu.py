"""Per-stream camera model and ballistics without a GPU: the rule from a raw camera index to a table entry, the refusals that
need no device, and the per-stream statements -- rmcv_attitude_step_host and rmcv_aim_step_host take ONE stream's config, so called with
stream f's matrix or config they say what the tables make k_attitude and k_aim write; here they are held against the independent
restatements tests/attitude_ref.c and tests/aim_ref.c, byte for byte."""
import numpy as np
import pytest

import aim_cases as AIMK
import aim_ref
import attitude_cases as ATTK
import attitude_ref
import camera_cases as CK
import rmcv_amd
from rmcv_amd import Tracker, abi, default_pnp_config


@pytest.mark.parametrize("n", [1, 3])
def test_frame_camera_rule(n):
    for idx in (-2**31, -1, 0, n - 1, n, 2**31 - 1):
        want = idx if 0 <= idx < n else 0
        assert rmcv_amd.frame_camera(idx, n) == want, (idx, n)
    assert rmcv_amd.Context.frame_camera(n - 1, n) == n - 1               # (the same function from the class)


def test_refusals_without_a_device():
    L = abi.lib()
    cams = (abi.PnpConfig * 2)(default_pnp_config(), CK.other_camera())
    idx = np.zeros(4, np.int32)
    mats = np.tile(np.eye(4).reshape(16), (4, 1))
    cfgs = (rmcv_amd.AimConfig * 1)(rmcv_amd.default_aim_config())
    bad = abi.ERR_BAD_ARG
    # null handles
    assert L.rmcv_pnp_load_cameras(None, cams, 2) == bad
    assert L.rmcv_batch_set_frame_cameras(None, abi.ptr(idx)) == bad
    assert L.rmcv_batch_set_device_frame_cameras(None, None) == bad
    assert L.rmcv_batch_get_frame_cameras(None, abi.ptr(idx), 4) == bad
    assert L.rmcv_pipeline_set_frame_cameras(None, None, 0) == bad
    assert L.rmcv_tracker_set_stream_cameras(None, abi.ptr(mats)) == bad
    assert L.rmcv_tracker_set_aim_configs(None, cfgs) == bad
    # n_cameras < 1 (and a null table)
    for n in (0, -1, -2**31):
        assert L.rmcv_pnp_load_cameras(None, cams, n) == bad
    assert L.rmcv_pnp_load_cameras(None, None, 1) == bad


@pytest.mark.parametrize("seed", CK.SEEDS)
def test_attitude_step_host_with_each_hand_eye_matrix(seed):
    cfg = CK.attitude_config(seed)
    n = len(ATTK.KINDS)
    pk, kinds = ATTK.packets(n, seed)
    att, camps, inp = ATTK.start_tables(n, seed + 1000)
    for f in range(n):
        for packet in (pk[f].tobytes(), None):
            got = Tracker.attitude_host(cfg, packet, att[f:f + 1], int(camps[f]), 3, inp[f:f + 1])
            want = attitude_ref.step(cfg, packet, att[f:f + 1], int(camps[f]), 3, inp[f:f + 1])
            assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2], (seed, kinds[f])
            assert got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes(), (seed, kinds[f])
    # the matrix reaches the result: the default's gives another world2camera
    other = Tracker.attitude_host(rmcv_amd.default_attitude_config(motor_angle_mode=cfg.motor_angle_mode), None, att[:1], None, 0, inp[:1])
    mine = Tracker.attitude_host(cfg, None, att[:1], None, 0, inp[:1])
    assert other[4]["world2camera"].tobytes() != mine[4]["world2camera"].tobytes()


def test_aim_step_host_with_each_aim_config():
    cfgs = [CK.aim_config(s) for s in CK.SEEDS]
    assert len(cfgs) == 5
    assert {(c.mode, c.height_mode) for c in cfgs} == {(m, h) for m in (abi.COMPENSATE_NONE, abi.COMPENSATE_CLASSIC) for h in (abi.AIM_HEIGHT_FIXED, abi.AIM_HEIGHT_DELTA)}
    lists = AIMK.lists()
    inputs = AIMK.aim_inputs(len(lists))
    records = set()
    for cfg in cfgs:
        for f, (name, tr) in enumerate(lists.items()):
            got = Tracker.aim_host(cfg, AIMK.TICK, tr, AIMK.NOW, (inputs[f]["world2camera"], float(inputs[f]["motor_angle"])))
            want = aim_ref.step(cfg, AIMK.TICK, tr, AIMK.NOW, inputs[f:f + 1])[0]
            assert got.tobytes() == want.tobytes(), (name, got, want)
            records.add(got.tobytes())
    assert len(records) > len(lists)                                       # the configs give different records for the same lists
