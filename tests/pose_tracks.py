"""The pose tracks at which the interpolation's arithmetic can go wrong, their queries, and a 50-digit mpmath evaluation of the
interpolation's formulas (tests/test_poses_cpu.py, tests/test_gpu_poses.py). Built once per process and never modified."""
from __future__ import annotations

import bisect
import functools

import numpy as np

from continuous_clustering_amd import kitti

EPOCH = 1_700_000_000_000_000_000   # ns: stamps of Unix-epoch size, 1.7e18 < 2^63
ROTATION_ENTRIES = (0, 1, 2, 4, 5, 6, 8, 9, 10)
TRANSLATION_ENTRIES = (3, 7, 11)
ONE = 1.0 - 2.220446049250313e-16


def rot(axis: int, angle: float) -> np.ndarray:
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[j, j], R[i, j], R[j, i] = c, c, -s, s
    return R


def pose(R, t) -> np.ndarray:
    return np.concatenate([np.concatenate([R[i], [t[i]]]) for i in range(3)]).astype(np.float64)


def _track(start: int, step: int, rotations, speed=(8.0, -0.7, 0.03)):
    n = len(rotations)
    stamps = np.array([start + k * step for k in range(n)], dtype=np.uint64)
    poses = np.stack([pose(R, [speed[0] * 0.1 * k + 1.5, speed[1] * 0.1 * k, speed[2] * 0.1 * k - 0.25]) for k, R in enumerate(rotations)])
    return stamps, poses


@functools.lru_cache(maxsize=None)
def tracks() -> dict:
    """name -> (stamps [N] uint64, poses [N][12]); read-only."""
    t = {}
    exact90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    tilt = rot(0, 0.1) @ rot(2, 0.3)
    # slerp's linear branch (abs_d >= 1 - eps): the same orientation again and again; exactly representable ones and a generic one
    t["identical"] = _track(1000, 100_000_000, [np.eye(3), np.eye(3), exact90, exact90, tilt, tilt, tilt])
    # 1e-9 rad between samples
    t["tiny"] = _track(EPOCH, 100_000_000, [rot(2, 0.3 + 1e-9 * k) for k in range(4)])
    # the yaw rate of kitti.synthetic_poses (0.05 rad/s, 10 Hz), as replay.Sequence builds its poses, at Unix-epoch stamps
    rows, times = kitti.synthetic_poses(6)
    t["synthetic"] = (np.array([EPOCH + int(x * 1000000000) for x in times], dtype=np.uint64),
                      np.stack([kitti.pose_from_line(r, kitti.CALIB_TR) for r in rows]))
    # about 170 degrees between samples: theta = acos(abs_d) near pi/2
    t["near170"] = _track(5_000, 100_000_000, [rot(2, 0.2 + np.deg2rad(170.0) * k) for k in range(4)] + [rot(2, 0.1), rot(2, 0.1 + np.deg2rad(179.5))])
    # yaw through +-pi; 2.0 -> -2.0 goes the long way for the quaternions: their dot is negative (d < 0)
    t["through_pi"] = _track(EPOCH + 77, 100_000_000, [rot(2, a) for a in (2.0, 2.6, 3.1, -2.9, -2.3, -2.0, 2.0, -2.0, 1.2, -1.9)])
    # beyond 120 degrees about x and about y: the other branches of the matrix -> quaternion conversion
    t["about_x"] = _track(123_456_789, 50_000_000, [rot(0, a) for a in (0.2, 2.5, 3.0, -2.8, 3.14, 0.4)])
    t["about_y"] = _track(EPOCH + 5, 50_000_000, [rot(1, a) for a in (0.2, 2.5, 3.0, -2.8, 3.14, 0.4)])
    t["mixed_axes"] = _track(10**12, 10_000_000, [rot(0, 2.9) @ rot(1, 0.3), rot(1, 2.9) @ rot(2, 0.4), rot(2, 2.9) @ rot(0, 0.5),
                                                   rot(0, 1.0) @ rot(1, 1.0) @ rot(2, 1.0)])
    t["single"] = _track(EPOCH + 12345, 1, [rot(2, 0.7) @ rot(0, 0.05)])
    # two equal neighbouring stamps
    s, p = _track(EPOCH, 100_000_000, [rot(2, 0.1 * k) @ rot(1, 0.02 * k) for k in range(5)])
    s = s.copy()
    s[2] = s[1]
    t["equal_stamps"] = (s, p)
    for s, p in t.values():
        s.setflags(write=False)
        p.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def combined():
    """All tracks one after the other as ONE track (stamps shifted so that they do not decrease; the junctions add intervals between
    unrelated orientations), at Unix-epoch stamps."""
    stamps, poses, at = [], [], EPOCH
    for s, p in tracks().values():
        stamps.append(s - s[0] + np.uint64(at))
        poses.append(p)
        at = int(stamps[-1][-1]) + 30_000_000
    s, p = np.concatenate(stamps), np.concatenate(poses)
    s.setflags(write=False)
    p.setflags(write=False)
    return s, p


def queries(stamps) -> np.ndarray:
    """Every sample stamp and 1 ns to either side, before the first sample and after the last, seven stamps inside every interval."""
    q = {int(stamps[0]) - 5, int(stamps[0]) - 10**9, int(stamps[-1]) + 10, int(stamps[-1]) + 10**9}
    for k, s in enumerate(int(v) for v in stamps):
        q.update((s - 1, s, s + 1))
        if k + 1 < len(stamps):
            d = int(stamps[k + 1]) - s
            q.update(s + (d * j) // 8 for j in range(1, 8))
    return np.array(sorted(v for v in q if v >= 0), dtype=np.uint64)


# ---- the double-precision decisions of the interpolation (numpy float64 scalars: IEEE, nothing fused) ----------------------------------

def quat_from_rotation(m, sqrt=np.sqrt):
    """Eigen's matrix -> quaternion conversion as cc_kitti.hip has it, on 12 numbers of any type; returns ([x, y, z, w], branch)."""
    r = lambda i, j: m[i * 4 + j]   # noqa: E731
    q = [None] * 4
    t = (r(0, 0) + r(1, 1)) + r(2, 2)
    if t > 0:
        t = sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (r(2, 1) - r(1, 2)) * t, (r(0, 2) - r(2, 0)) * t, (r(1, 0) - r(0, 1)) * t
        return q, "w"
    i = 0
    if r(1, 1) > r(0, 0):
        i = 1
    if r(2, 2) > r(i, i):
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = sqrt(r(i, i) - r(j, j) - r(k, k) + 1)
    q[i] = t / 2
    t = 1 / (2 * t)
    q[3] = (r(k, j) - r(j, k)) * t
    q[j] = (r(j, i) + r(i, j)) * t
    q[k] = (r(k, i) + r(i, k)) * t
    return q, "xyz"[i]


def double_dot(pb, pa) -> float:
    """The quaternion dot product of two samples exactly as the double code computes it (0.5 * t and 0.5 / t are t / 2 and 1 / (2 t) bit
    for bit: scaling by 2 is exact)."""
    a, _ = quat_from_rotation([np.float64(v) for v in pb])
    b, _ = quat_from_rotation([np.float64(v) for v in pa])
    return float((a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3]))


def classify(stamps, poses, stamp: int) -> str:
    """Which path the double code takes for this query: "clamped" (raw sample), "linear" (slerp's linear branch) or "slerp"."""
    ia = bisect.bisect_left([int(s) for s in stamps], int(stamp))
    if ia == 0 or ia == len(stamps):
        return "clamped"
    return "linear" if abs(double_dot(poses[ia - 1], poses[ia])) >= ONE else "slerp"


# ---- 50-digit evaluation of the same formulas ----------------------------------------------------------------------------------------------

def mp_interpolate(stamps, poses, stamp: int, seen: set | None = None):
    """cc_kitti.hip's interpolate from the same double inputs in 50-digit arithmetic: 12 mpf. `seen` collects the branches taken."""
    import mpmath as mp
    mp.mp.dps = 50
    seen = set() if seen is None else seen
    st = [int(s) for s in stamps]
    ia = bisect.bisect_left(st, int(stamp))
    if ia == 0 or ia == len(st):
        seen.add("clamped")
        return [mp.mpf(float(v)) for v in poses[min(ia, len(st) - 1)]]
    pb = [mp.mpf(float(v)) for v in poses[ia - 1]]
    pa = [mp.mpf(float(v)) for v in poses[ia]]
    f = mp.mpf(int(stamp) - st[ia - 1]) / mp.mpf(st[ia] - st[ia - 1])
    a, ba = quat_from_rotation(pb, mp.sqrt)
    b, bb = quat_from_rotation(pa, mp.sqrt)
    seen.update(("quat_" + ba, "quat_" + bb))
    d = (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3])
    if abs(d) >= mp.mpf(ONE):
        seen.add("linear")
        s0, s1 = 1 - f, f
    else:
        seen.add("slerp")
        theta = mp.acos(abs(d))
        if theta > mp.mpf("1.4"):
            seen.add("theta_near_pi_2")
        s0, s1 = mp.sin((1 - f) * theta) / mp.sin(theta), mp.sin(f * theta) / mp.sin(theta)
    if d < 0:
        seen.add("negative_dot")
        s1 = -s1
    x, y, z, w = [s0 * a[i] + s1 * b[i] for i in range(4)]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    out = [None] * 12
    out[0], out[1], out[2] = 1 - (tyy + tzz), txy - twz, txz + twy
    out[4], out[5], out[6] = txy + twz, 1 - (txx + tzz), tyz - twx
    out[8], out[9], out[10] = txz - twy, tyz + twx, 1 - (txx + tyy)
    for i in range(3):
        out[i * 4 + 3] = (1 - f) * pb[i * 4 + 3] + f * pa[i * 4 + 3]
    return out


def rotation_error_units(pose12, ref12) -> float:
    """Largest |double - mpmath| over the nine rotation entries, in units of 2^-53."""
    import mpmath as mp
    return float(max(abs(mp.mpf(float(pose12[i])) - ref12[i]) for i in ROTATION_ENTRIES) * mp.mpf(2) ** 53)
