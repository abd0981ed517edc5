"""CPU: the host twin of the device pose interpolation (include/cc_poses.h) against the existing host path and against a
50-digit mpmath evaluation of the same formulas, over the track table of tests/pose_tracks.py; the C-ABI's refusals; replay's `poses`
parameter. Nothing here needs a GPU.

Measured over the table (units of 2^-53, largest absolute error of a rotation entry): existing host path E_ref = 9.75, twin 9.75; the bound
2 * E_ref + 2 is 21.5.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import pose_tracks as pt
from continuous_clustering_amd import EngineError, capi, kitti, poses, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    load_library()
    return poses._lib()


@pytest.fixture(scope="module")
def table(lib):
    """name -> (stamps, poses, queries, twin poses [Q][12], host-path poses [Q][12], path of each query)."""
    out = {}
    named = dict(pt.tracks())
    named["combined"] = pt.combined()
    for name, (s, p) in named.items():
        q = pt.queries(s)
        twin = poses.host_lookup(s, p, q)
        host = np.stack([kitti.pose_interpolate(s, p, int(x)) for x in q])
        path = [pt.classify(s, p, int(x)) for x in q]
        out[name] = (s, p, q, twin, host, path)
    return out


def test_table_reaches_every_branch(table):
    seen = set()
    for name, (s, p, q, _, _, path) in table.items():
        if name != "combined":
            for x in q:
                pt.mp_interpolate(s, p, int(x), seen)
    assert seen >= {"clamped", "linear", "slerp", "negative_dot", "theta_near_pi_2", "quat_w", "quat_x", "quat_y", "quat_z"}, seen
    assert {"clamped", "linear", "slerp"} == {v for row in table.values() for v in row[5]}
    # (a generic orientation met twice may have a dot product one rounding below 1 - eps and take the slerp with a theta near 1e-8)
    print({name: sorted(set(row[5])) for name, row in table.items()})
    assert "linear" in table["identical"][5] and "linear" in table["tiny"][5]
    assert set(table["single"][5]) == {"clamped"}
    assert int(table["synthetic"][0][0]) > 2 ** 60


def test_clamped_and_linear_poses_and_all_translations_equal_the_host_path_bit_for_bit(table):
    n_exact = 0
    for name, (s, p, q, twin, host, path) in table.items():
        t = list(pt.TRANSLATION_ENTRIES)
        assert np.array_equal(twin[:, t].view(np.uint64), host[:, t].view(np.uint64)), name
        exact = np.array([v != "slerp" for v in path])
        n_exact += int(exact.sum())
        assert np.array_equal(twin[exact].view(np.uint64), host[exact].view(np.uint64)), name
        for k in np.nonzero(np.array([v == "clamped" for v in path]))[0]:   # the raw sample, copied
            raw = p[0] if q[k] <= s[0] else p[-1]
            assert np.array_equal(twin[k].view(np.uint64), raw.view(np.uint64)), (name, k)
    assert n_exact > 200


def test_sweep_stamps_equal_the_host_path_and_sweep_poses_equal_lookup(table):
    s, p = table["synthetic"][:2]
    start, end = kitti.start_end_stamps(s)
    for f in (0, 2, 5):
        hs, hp = kitti.firing_stamps_and_poses(s, p, start[f], end[f])
        ts, tp = poses.host_sweep(s, p, kitti.COLS, start[f], end[f])
        assert ts.dtype == np.uint64 and np.array_equal(ts, hs)
        assert np.array_equal(tp[:, list(pt.TRANSLATION_ENTRIES)].view(np.uint64), hp[:, list(pt.TRANSLATION_ENTRIES)].view(np.uint64))
        assert np.array_equal(tp.view(np.uint64), poses.host_lookup(s, p, ts).view(np.uint64))
        clamped = (ts <= s[0]) | (ts > s[-1])
        assert np.array_equal(tp[clamped].view(np.uint64), hp[clamped].view(np.uint64))
        assert np.abs(tp - hp).max() < 1e-14
    # any n >= 2; the stamps are start + (uint64)((double)(end - start) * ((double)c / (n - 1)))
    for n in (2, 3, 65):
        ts, tp = poses.host_sweep(s, p, n, int(s[1]) + 7, int(s[4]) + 1)
        want = [int(s[1]) + 7 + int(float(int(s[4]) + 1 - int(s[1]) - 7) * (float(c) / (n - 1))) for c in range(n)]
        assert ts.tolist() == want and tp.shape == (n, 12)
    ts, tp = poses.host_sweep(s, p, 4, int(s[2]), int(s[2]))   # an empty sweep: n times the same stamp
    assert ts.tolist() == [int(s[2])] * 4 and np.array_equal(tp, np.tile(poses.host_lookup(s, p, s[2:3]), (4, 1)))


def test_rotation_error_against_mpmath_is_within_twice_the_host_paths_plus_two_units(table):
    e_ref = e_twin = 0.0
    for name, (s, p, q, twin, host, _) in table.items():
        for k, x in enumerate(q):
            ref = pt.mp_interpolate(s, p, int(x))
            e_ref = max(e_ref, pt.rotation_error_units(host[k], ref))
            e_twin = max(e_twin, pt.rotation_error_units(twin[k], ref))
    print(f"rotation entries against mpmath, units of 2^-53: host path E_ref = {e_ref:.3f}, twin = {e_twin:.3f}, bound {2 * e_ref + 2:.3f}")
    assert e_twin <= 2 * e_ref + 2, (e_twin, e_ref)


def test_twin_rotations_are_orthonormal_and_reach_the_samples(table):
    for name, (s, p, q, twin, _, _) in table.items():
        R = twin.reshape(-1, 3, 4)[:, :, :3]
        assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12), name   # the bound of test_oracle_interpolate_endpoints_and_rigidity
        assert np.allclose(np.linalg.det(R), 1.0, atol=1e-12), name
        at = {int(x): k for k, x in enumerate(q)}
        for k in range(len(s)):   # an interior sample is reached with f == 1 through the quaternion round trip
            if k > 0 and s[k] == s[k - 1]:   # (of equal stamps a query meets the first)
                continue
            assert np.allclose(twin[at[int(s[k])]], p[k], atol=1e-12), (name, k)


def test_equal_neighbouring_stamps_meet_the_first_of_them_and_never_divide_by_zero(table):
    s, p, q, twin, host, _ = table["equal_stamps"]
    assert s[1] == s[2] and np.isfinite(twin).all()
    k = int(np.nonzero(q == s[1])[0][0])
    assert np.allclose(twin[k], p[1], atol=1e-12) and not np.allclose(twin[k], p[2], atol=1e-6)
    after = poses.host_lookup(s, p, [int(s[2]) + 1])[0]   # 1 ns later: between sample 2 and sample 3
    assert np.allclose(after, p[2], atol=1e-7)
    assert np.array_equal(twin.view(np.uint64)[np.array(table["equal_stamps"][5]) != "slerp"],
                          host.view(np.uint64)[np.array(table["equal_stamps"][5]) != "slerp"])


def test_header_symbols_are_exported_and_bad_arguments_are_refused_before_the_device_is_looked_for(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_poses.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    for n in ("cc_poses_last_error", "cc_poses_host_lookup", "cc_poses_host_sweep", "cc_pose_tracks_create", "cc_pose_tracks_destroy",
              "cc_pose_tracks_set", "cc_pose_tracks_sweep", "cc_pose_tracks_lookup"):
        assert n in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_poses.h but not exported by libcc_hip.so"
    bad = capi.CC_ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.cc_pose_tracks_create(None, 0, 1, 4, None) == bad and b"cc_pose_tracks_create" in lib.cc_poses_last_error()
    assert lib.cc_pose_tracks_create(ctypes.byref(h), 0, 0, 4, None) == bad
    assert lib.cc_pose_tracks_create(ctypes.byref(h), 0, 1, 0, None) == bad
    assert lib.cc_pose_tracks_create(ctypes.byref(h), 0, 65536, 4, None) == bad and b"cc_pose_tracks_create" in lib.cc_poses_last_error()
    s = np.array([1, 2], dtype=np.uint64)
    p = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64), (2, 1))
    one = np.zeros(1, dtype=np.uint64)
    calls = {"cc_pose_tracks_set": lambda: lib.cc_pose_tracks_set(None, 0, 2, s.ctypes.data, p.ctypes.data),
             "cc_pose_tracks_sweep": lambda: lib.cc_pose_tracks_sweep(None, 2, one.ctypes.data, one.ctypes.data, None, 16, None),
             "cc_pose_tracks_lookup": lambda: lib.cc_pose_tracks_lookup(None, 1, 16, 1, 16),
             "cc_pose_tracks_sync": lambda: lib.cc_pose_tracks_sync(None)}
    for name, call in calls.items():   # a NULL handle
        assert call() == bad and name.encode() in lib.cc_poses_last_error(), name
    assert lib.cc_pose_tracks_hip_stream(None) is None
    lib.cc_pose_tracks_destroy(None)
    import torch
    rc = lib.cc_pose_tracks_create(ctypes.byref(h), 0, 2, 8, None)
    if torch.cuda.is_available():
        assert rc == capi.CC_OK
        lib.cc_pose_tracks_destroy(h)
    else:
        assert rc == capi.CC_ERR_NO_DEVICE and not h.value
        assert b"no gfx950 device" in lib.cc_poses_last_error()
        with pytest.raises(EngineError) as e:
            poses.PoseTracks(2, 8)
        assert e.value.code == capi.CC_ERR_NO_DEVICE


def test_host_twin_refuses_bad_arguments(lib):
    s, p = pt.tracks()["synthetic"]
    for n in (-1, 0, 1):
        with pytest.raises(EngineError) as e:
            poses.host_sweep(s, p, n, int(s[0]), int(s[1]))
        assert e.value.code == capi.CC_ERR_INVALID_ARGUMENT and "cc_poses_host_sweep" in str(e.value)
    with pytest.raises(EngineError) as e:
        poses.host_sweep(s, p, 4, int(s[1]), int(s[0]))
    assert "cc_poses_host_sweep" in str(e.value)
    with pytest.raises(EngineError) as e:
        poses.host_lookup(s[:0], p[:0], [1, 2])
    assert e.value.code == capi.CC_ERR_INVALID_ARGUMENT and "cc_poses_host_lookup" in str(e.value)
    with pytest.raises(ValueError):
        poses.host_lookup(s, p[:-1], [1])
    assert poses.host_lookup(s, p, []).shape == (0, 12)
    assert lib.cc_poses_host_lookup(2, None, p.ctypes.data, 0, None, None) == capi.CC_ERR_INVALID_ARGUMENT


def test_replay_takes_poses_and_refuses_unknown_values(tmp_path):
    import continuous_clustering_amd as cca
    assert cca.poses is poses and cca.PoseTracks is poses.PoseTracks and "PoseTracks" in cca.__all__
    assert inspect.signature(replay.replay).parameters["poses"].default == "host"
    with pytest.raises(ValueError):
        replay.replay(str(tmp_path), [], poses="gpu")
    with pytest.raises(ValueError):
        replay.replay(str(tmp_path), [0], poses=None)
    for v in ("host", "device", "twin"):
        assert replay.replay(str(tmp_path), [], poses=v) == ([], dict(streams=0, frames=0, cells_published=0))
