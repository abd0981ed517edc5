"""Streams under odometry poses the other cases never have: far from the odom origin, with rotation blocks that are not orthonormal, and with
NaN / inf in them. Pure numpy; every function returns a new synth.Stream and leaves its argument alone.

What the poses are for (tests/test_pose_cases_cpu.py measures each on the oracle, tests/test_gpu_pose_parity.py puts the engine against it):
  FAR_OFFSETS     a constant added to every pose translation. The cells' x, y, z are float32 in the odom frame (cc.cpp:223-225), so at
                  UTM-like coordinates they are quantised to 3 cm .. 1 m (64 m at 1e9): vertically adjacent returns of a column share x and y
                  exactly, the slopes of the segmentation divide by zero, the association sees distance 0 between different cells.
  POSE_VARIANTS   constant poses — rigid, scaled, sheared, rounded to float32, far away — under which plant_box_corners puts returns just inside
                  and just outside the ego box's corners: the one place where a too small skip_r2 (csrc/cc_k_segment.h: ego_record) would show.
  with_non_finite NaN / inf in the poses of some firings."""
from __future__ import annotations

import math

import numpy as np

from continuous_clustering_amd import synth

UTM = (4.5e5, 5.4e6, 520.0)
FAR_OFFSETS = {
    "utm": UTM,                                   # x, y quantised to 1 / 32 m and 1 / 2 m
    "3e6_-7e6": (3.0e6, -7.0e6, 0.0),             # 1 / 4 m and 1 / 2 m
    "2p24": (2.0 ** 24, 2.0 ** 24, 0.0),          # the first binade without a fraction: 1 m (2 m beyond it)
    "1e9": (1.0e9, 1.0e9, 0.0),                   # 64 m: almost every cell of a column collapses onto one point
}


def _copy(stream, **over):
    d = dict(xyz=stream.xyz, intensity=stream.intensity, poses=stream.poses, sensor=stream.sensor, hit=stream.hit)
    d.update(over)
    return synth.Stream(**d)


def with_offset(stream, offset):
    """The same firings with `offset` (3 values) added to every pose translation."""
    poses = np.array(stream.poses, dtype=np.float64, copy=True)
    poses[:, [3, 7, 11]] += np.asarray(offset, dtype=np.float64)[None, :]
    return _copy(stream, poses=poses)


def with_pose_map(stream, fn):
    """The same firings with every rotation block R [3, 3] replaced by fn(R) (scale, shear, rounding); translations stay."""
    poses = np.array(stream.poses, dtype=np.float64, copy=True)
    m = poses.reshape(-1, 3, 4)
    for k in range(m.shape[0]):
        m[k, :, :3] = np.asarray(fn(m[k, :, :3].copy()), dtype=np.float64)
    return _copy(stream, poses=poses)


def with_constant_pose(stream, pose12):
    return _copy(stream, poses=np.tile(np.asarray(pose12, dtype=np.float64).reshape(1, 12), (stream.n_firings, 1)))


def with_non_finite(stream, value, where):
    """`value` (NaN or inf) in the translation x of a run of 20 firings ("translation_run"), in one rotation entry of a single firing
    ("rotation_entry"), or in every entry of one firing ("whole_pose"). The places scale with the stream's length."""
    poses = np.array(stream.poses, dtype=np.float64, copy=True)
    n = stream.n_firings
    if where == "translation_run":
        poses[n // 4:n // 4 + 20, 3] = value
    elif where == "rotation_entry":
        poses[(n * 5) // 9, 0] = value
    elif where == "whole_pose":
        poses[(n * 7) // 10, :] = value
    else:
        raise KeyError(where)
    return _copy(stream, poses=poses)


NON_FINITE_PLACES = ("translation_run", "rotation_entry", "whole_pose")


# ---- constant poses ---------------------------------------------------------------------------------------------------------------------------
def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rx(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def pose12(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).reshape(12)


ROTATION = _rz(0.7) @ _ry(0.04) @ _rx(-0.05)
SHEAR = np.array([[1.0, 0.08, 0.0], [0.0, 1.0, 0.0], [-0.05, 0.0, 1.0]])
NEAR, FAR_1E5 = (3.0, -2.0, 0.5), (-1.2e5, 8.0e4, 30.0)
# name -> odom_from_sensor. "Near": translation below 100 m; "utm*": float32 odom coordinates are quantised coarser than the planting's margin.
POSE_VARIANTS = {
    "identity": pose12(np.eye(3), (0.0, 0.0, 0.0)),
    "rigid": pose12(ROTATION, NEAR),
    "scaled_0.9": pose12(0.9 * ROTATION, NEAR),
    "scaled_1.1": pose12(1.1 * ROTATION, NEAR),
    "scaled_0.7": pose12(0.7 * ROTATION, NEAR),                            # Gram deviation 0.88: skip_r2 = +inf
    "sheared": pose12(ROTATION @ SHEAR, NEAR),
    "f32_rotation": pose12(ROTATION.astype(np.float32).astype(np.float64), NEAR),
    "far_1e5": pose12(ROTATION, FAR_1E5),
    "utm": pose12(ROTATION, UTM),
    "utm_yaw90": pose12(_rz(math.pi / 2) @ _ry(0.04) @ _rx(-0.05), UTM),  # the sensor's x axis along odom y: the coarse coordinate is the other one
    "scaled_1.1_far_1e5": pose12(1.1 * ROTATION, FAR_1E5),
    "utm_f32_rotation": pose12(ROTATION.astype(np.float32).astype(np.float64), UTM),
}
NEAR_VARIANTS = ("identity", "rigid", "scaled_0.9", "scaled_1.1", "scaled_0.7", "sheared", "f32_rotation")
UTM_VARIANTS = ("utm", "utm_yaw90", "utm_f32_rotation")


def gram_deviation(block):
    """Frobenius distance of block^T block from the identity — ego_record's dev_t / dev_a: below 0.5 skip_r2 is finite, from 0.5 on (or NaN) +inf."""
    b = np.asarray(block, dtype=np.float64).reshape(3, -1)[:, :3]
    return float(np.sqrt(((b.T @ b - np.eye(3)) ** 2).sum()))


# ---- returns at the ego box's corners -----------------------------------------------------------------------------------------------------------
PLANT_FIRST_ROW, PLANT_ROW_STEP = 8, 3


def box_of(cfg):
    lo = np.array([cfg.length_ref_to_rear_end_, cfg.width_ref_to_right_mirror_, cfg.height_ref_to_ground_], dtype=np.float64)
    hi = np.array([cfg.length_ref_to_front_end_, cfg.width_ref_to_left_mirror_, cfg.height_ref_to_maximum_], dtype=np.float64)
    return lo, hi


def plant_box_corners(stream, T, A, cfg, eps=2e-3):
    """`stream` under the constant pose T (odom_from_sensor, 12 values) with two returns per corner of cfg's ego box and rotation: the corner of
    the box scaled about its centre by 1 - eps (inner) and by 1 + eps (outer). The segmentation maps a cell p_odom = R_T p + t_T to the robot frame
    by A * [R_T^T | -R_T^T t_T] (cc.cpp:300-301: the inverse of a RIGID pose), so the corner e is reached by the sensor-frame point
    p = (A_R R_T^T R_T)^-1 (e - A_t) — computed in float64, rounded to float32, and written into the firing whose nominal azimuth is that of p (the
    column comes from the sensor-frame azimuth, cc.cpp:142-152), on rows 8 + 3 * corner (inner) and 9 + 3 * corner (outer).
    A: robot_from_sensor (12 values) or None for the identity. Returns (stream, [(firing, row, inner?)])."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    A = np.eye(3, 4) if A is None else np.asarray(A, dtype=np.float64).reshape(3, 4)
    M = A[:, :3] @ T[:, :3].T @ T[:, :3]
    lo, hi = box_of(cfg)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    assert (half > 0).all()
    sen = stream.sensor
    cols, rows = sen.num_columns, sen.num_rows
    assert not sen.azimuth_offsets_deg and PLANT_FIRST_ROW + 8 * PLANT_ROW_STEP <= rows
    w = 2 * math.pi / cols
    xyz = stream.xyz.copy()
    planted = []
    for corner in range(8):
        sign = np.array([1.0 if corner & 1 else -1.0, 1.0 if corner & 2 else -1.0, 1.0 if corner & 4 else -1.0])
        for inner in (True, False):
            e = centre + sign * half * ((1.0 - eps) if inner else (1.0 + eps))
            p = np.linalg.solve(M, e - A[:, 3]).astype(np.float32)
            az = math.atan2(float(p[1]), float(p[0]))
            inc = (math.pi - az) if sen.clockwise else (az + math.pi)
            k0 = min(cols - 1, int(inc / w))
            row = PLANT_FIRST_ROW + PLANT_ROW_STEP * corner + (0 if inner else 1)
            for firing in range(k0, stream.n_firings, cols):
                xyz[firing, row] = p
                planted.append((firing, row, inner))
    return with_constant_pose(_copy(stream, xyz=xyz), T.reshape(12)), planted
