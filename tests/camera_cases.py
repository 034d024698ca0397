"""The case list of the per-stream camera and ballistics tests (TEST INFRASTRUCTURE), shared by tests/test_cameras_cpu.py and
tests/test_gpu_cameras.py: the cameras of a mixed fleet, seeded hand-eye matrices and seeded aim configs."""
import numpy as np

import attitude_cases as AK
from rmcv_amd import abi, default_pnp_config
from rmcv_amd.tracker import default_aim_config, default_attitude_config

SEEDS = (101, 102, 103, 104, 105)


def other_camera():
    """the "other camera" of tests/test_gpu_pnp.py::test_locate_armours_other_camera, its 13.5 x 5.5 plate included"""
    cfg = default_pnp_config()
    cfg.camera_matrix[0], cfg.camera_matrix[4], cfg.camera_matrix[2], cfg.camera_matrix[5] = 1200.0, 1210.0, 640.0, 512.0
    for i, v in enumerate((0.08, -0.2, 0.001, -0.002, 0.05)):
        cfg.dist[i] = v
    cfg.square_w, cfg.square_h = 13.5, 5.5
    return cfg


def moved_camera(seed):
    """the default lens on another mount: gripper2camera alone differs"""
    cfg = default_pnp_config()
    for i, v in enumerate(AK.gripper2camera(seed).reshape(16)):
        cfg.gripper2camera[i] = v
    return cfg


def fleet(n):
    """n different cameras: the default, the other lens, then other mounts (every second one of them with the other lens too)"""
    out = [default_pnp_config(), other_camera()]
    for k in range(2, n):
        c = moved_camera(200 + k)
        if k % 2:
            o = other_camera()
            for name in ("camera_matrix", "dist"):
                for i, v in enumerate(getattr(o, name)):
                    getattr(c, name)[i] = v
        out.append(c)
    return out[:n]


def hand_eye(seed):
    """(4, 4): a seeded rigid gripper2camera"""
    return AK.gripper2camera(seed)


def attitude_config(seed):
    """an AttitudeConfig with the seed's hand-eye matrix; the motor angle mode alternates"""
    return default_attitude_config(gripper2camera=hand_eye(seed), motor_angle_mode=abi.ATT_MOTOR_PITCH if seed % 2 else abi.ATT_MOTOR_KEEP)


def aim_config(seed):
    """a seeded AimConfig: over consecutive seeds both compensate modes and both height modes come up in every combination"""
    rng = np.random.default_rng(seed)
    return default_aim_config(
        mode=abi.COMPENSATE_CLASSIC if seed % 2 else abi.COMPENSATE_NONE,
        height_mode=abi.AIM_HEIGHT_DELTA if (seed // 2) % 2 else abi.AIM_HEIGHT_FIXED,
        g=float(rng.uniform(9.7, 9.9)), v0=float(rng.uniform(14.0, 30.0)), height=float(rng.uniform(-30.0, 40.0)),
        offset_x=float(np.float32(rng.uniform(-3, 3))), offset_y=float(np.float32(rng.uniform(-3, 3))), angle_offset=float(rng.uniform(-0.02, 0.02)),
        latency_s=float(rng.uniform(0.0, 0.03)), pick=int(rng.integers(0, 2)), source=int(rng.integers(0, 2)), lead_iterations=int(rng.integers(0, 5)),
        max_lost=int(rng.integers(2, 30)))


def to_oracle_cfg(oracle, cfg):
    o = oracle.PnpConfig()
    for name in ("camera_matrix", "dist", "gripper2camera"):
        for i, v in enumerate(getattr(cfg, name)):
            getattr(o, name)[i] = v
    o.square_w, o.square_h = cfg.square_w, cfg.square_h
    return o
