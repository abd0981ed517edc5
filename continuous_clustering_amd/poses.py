"""ctypes host mirror of include/cc_poses.h — per-firing odometry poses interpolated on the GPU from pose tracks.

`PoseTracks` keeps the stamped odometry samples of every stream in device memory and writes `d_poses [S][n][12]`, the third input of
`Engine.add_firings_device`, without a host round trip: `sweep` for the firings of one rotation per stream (what
`kitti.firing_stamps_and_poses` computes on the host), `lookup` for arbitrary stamps in device memory (packet or message stamps, each
pose repeated for the columns of its packet). `host_lookup` / `host_sweep` are the CPU twin: the same arithmetic compiled for the host,
bit-equal to the device results on every host. There is no CPU variant of the device path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, load_library

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
        L.cc_poses_last_error.restype = C.c_char_p
        L.cc_poses_host_lookup.argtypes = [i64, vp, vp, i64, vp, vp]
        L.cc_poses_host_sweep.argtypes = [i64, vp, vp, C.c_int32, u64, u64, vp, vp]
        L.cc_pose_tracks_create.argtypes = [C.POINTER(vp), i32, i32, i32, vp]
        L.cc_pose_tracks_destroy.argtypes = [vp]
        L.cc_pose_tracks_destroy.restype = None
        L.cc_pose_tracks_hip_stream.argtypes = [vp]
        L.cc_pose_tracks_hip_stream.restype = vp
        L.cc_pose_tracks_sync.argtypes = [vp]
        L.cc_pose_tracks_set.argtypes = [vp, i32, i32, vp, vp]
        L.cc_pose_tracks_sweep.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.cc_pose_tracks_lookup.argtypes = [vp, i32, vp, i32, vp]
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_poses_last_error().decode())


def _track_args(stamps, poses):
    stamps = np.ascontiguousarray(stamps, dtype=np.uint64).reshape(-1)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    if stamps.shape[0] != poses.shape[0]:
        raise ValueError(f"{stamps.shape[0]} stamps for {poses.shape[0]} poses")
    return stamps, poses


# ---- host twin ---------------------------------------------------------------------------------------------------------------

def host_lookup(stamps, poses, query_stamps) -> np.ndarray:
    """The pose [Q][12] at each of `query_stamps` of the track (stamps [N] non-decreasing, poses [N][12]), on the CPU."""
    stamps, poses = _track_args(stamps, poses)
    q = np.ascontiguousarray(query_stamps, dtype=np.uint64).reshape(-1)
    out = np.zeros((q.shape[0], 12), dtype=np.float64)
    _check(_lib().cc_poses_host_lookup(stamps.shape[0], stamps.ctypes.data, poses.ctypes.data, q.shape[0], q.ctypes.data, out.ctypes.data))
    return out


def host_sweep(stamps, poses, n: int, start: int, end: int):
    """(stamps [n], poses [n][12]) of the n firings of the sweep [start, end], on the CPU: `kitti.firing_stamps_and_poses` for any n,
    with this library's acos / sin."""
    stamps, poses = _track_args(stamps, poses)
    out_s = np.zeros(max(int(n), 0), dtype=np.uint64)
    out_p = np.zeros((max(int(n), 0), 12), dtype=np.float64)
    _check(_lib().cc_poses_host_sweep(stamps.shape[0], stamps.ctypes.data, poses.ctypes.data, int(n), int(start), int(end),
                                      out_s.ctypes.data, out_p.ctypes.data))
    return out_s, out_p


# ---- device ------------------------------------------------------------------------------------------------------------------

class PoseTracks:
    """One cc_pose_tracks handle: the pose tracks of `num_streams` streams, up to `max_samples` samples each. Pass
    hip_stream=engine.hip_stream() (and set the engine option "input_on_engine_stream") to chain with an engine; close the handle before
    that engine. Every call is asynchronous on the handle's HIP stream; host arrays are copied before a call returns."""

    def __init__(self, num_streams: int, max_samples: int, device: int = 0, hip_stream: int | None = None):
        self.L = _lib()
        self.num_streams, self.max_samples, self.device = num_streams, max_samples, device
        self.h = C.c_void_p()
        rc = self.L.cc_pose_tracks_create(C.byref(self.h), device, num_streams, max_samples, hip_stream)
        if rc != 0:
            self.h = None
            _check(rc)

    def close(self):
        if getattr(self, "h", None):
            self.L.cc_pose_tracks_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hip_stream(self) -> int:
        return self.L.cc_pose_tracks_hip_stream(self.h)

    def sync(self):
        _check(self.L.cc_pose_tracks_sync(self.h))

    def set(self, stream: int, stamps, poses):
        """Replace the track of `stream`: stamps [N] uint64 non-decreasing, poses [N][12] (host arrays), 1 <= N <= max_samples."""
        stamps, poses = _track_args(stamps, poses)
        _check(self.L.cc_pose_tracks_set(self.h, int(stream), stamps.shape[0], stamps.ctypes.data, poses.ctypes.data))

    def sweep_raw(self, n: int, start, end, d_poses, hold=None, d_stamps=None) -> int:
        """cc_pose_tracks_sweep; returns the status code without raising. start / end / hold: one value per stream."""
        S = self.num_streams
        start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
        end = np.ascontiguousarray(end, dtype=np.uint64).reshape(-1)
        if hold is not None:
            hold = np.ascontiguousarray(hold, dtype=np.int32).reshape(-1)
        if start.shape[0] != S or end.shape[0] != S or (hold is not None and hold.shape[0] != S):
            raise ValueError(f"start, end and hold need one value for each of the {S} streams")
        return self.L.cc_pose_tracks_sweep(self.h, int(n), start.ctypes.data, end.ctypes.data, None if hold is None else hold.ctypes.data,
                                           _ptr(d_poses), _ptr(d_stamps))

    def sweep(self, n: int, start, end, d_poses, hold=None, d_stamps=None):
        """d_poses [S][n][12] float64 on the device (16-byte aligned) = the poses of the n firings of the sweep [start[s], end[s]] of every
        stream; hold[s] = k >= 0: raw sample k, n times (a stream that has ended), -1: sweep. d_stamps [S][n] uint64 gets the firing stamps
        when given."""
        _check(self.sweep_raw(n, start, end, d_poses, hold, d_stamps))

    def lookup_raw(self, n: int, d_stamps, d_poses, repeat: int = 1) -> int:
        return self.L.cc_pose_tracks_lookup(self.h, int(n), _ptr(d_stamps), int(repeat), _ptr(d_poses))

    def lookup(self, n: int, d_stamps, d_poses, repeat: int = 1):
        """d_poses [S][n * repeat][12] float64 on the device = the pose at each of d_stamps [S][n] uint64 (on the device), written `repeat`
        times in a row: repeat = columns per packet for per-packet stamps, 1 to fill a decoder's packet poses."""
        _check(self.lookup_raw(n, d_stamps, d_poses, repeat))


__all__ = ["PoseTracks", "host_lookup", "host_sweep"]
