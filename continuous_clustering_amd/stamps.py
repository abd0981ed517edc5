"""ctypes host mirror of include/cc_stamps.h — the firing-stamp log: time stamps of taken points, columns and clusters, resolved in device
memory.

`FiringStamps` keeps the stamps (uint64 ns, one per firing) of the recent firings of every stream in device memory, keyed by the firing
index the engine counts (`source_firing`). `push` appends what a sweep (`PoseTracks.sweep(..., d_stamps=)`) or a packet front end left in
device memory, `of_points` / `of_columns` / `of_clusters` turn the records of `Engine.take_points` / `Engine.take_clusters` into the
reference's point stamps (with time_sec / time_nsec), column and message header stamps and cluster stamps. `HostFiringStamps` is the CPU
twin over numpy arrays: the same arithmetic compiled for the host, bit-equal to the device results. torch is imported only where a tensor
is allocated. There is no CPU variant of the device path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, load_library
from .take import TAKE_CLUSTER_DTYPE, TAKE_POINT_DTYPE, TAKE_STREAM_DTYPE


class ClusterStamp(C.Structure):
    """cc_cluster_stamp."""
    _fields_ = [("stamp", C.c_uint64), ("min_stamp", C.c_uint64), ("max_stamp", C.c_uint64), ("n_missing", C.c_uint32), ("pad", C.c_uint32)]


class HostLog(C.Structure):
    """cc_stamps_host_log."""
    _fields_ = [("num_streams", C.c_int32), ("pad", C.c_int32), ("capacity", C.c_int64), ("rings", C.c_void_p), ("heads", C.c_void_p),
                ("floors", C.c_void_p), ("missing", C.c_void_p)]


CLUSTER_STAMP_DTYPE = np.dtype([("stamp", "<u8"), ("min_stamp", "<u8"), ("max_stamp", "<u8"), ("n_missing", "<u4"), ("pad", "<u4")])
assert CLUSTER_STAMP_DTYPE.itemsize == C.sizeof(ClusterStamp) == 32

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
        log = C.POINTER(HostLog)
        L.cc_firing_stamps_last_error.restype = C.c_char_p
        L.cc_stamps_round_capacity.argtypes = [i64]
        L.cc_stamps_round_capacity.restype = i64
        L.cc_stamps_host_push.argtypes = [log, i32, i64, vp, i32]
        L.cc_stamps_host_resolve.argtypes = [log, i32, i64, vp, vp, vp]
        L.cc_stamps_host_sec_nsec.argtypes = [i64, vp, vp]
        L.cc_stamps_host_of_points.argtypes = [log, i64, vp, vp, vp, vp]
        L.cc_stamps_host_of_columns.argtypes = [log, i64, vp, vp, vp, vp]
        L.cc_stamps_host_of_clusters.argtypes = [log, i32, i64, vp, i64, vp, vp, vp]
        L.cc_firing_stamps_create.argtypes = [C.POINTER(vp), i32, i32, i64, vp]
        L.cc_firing_stamps_destroy.argtypes = [vp]
        L.cc_firing_stamps_destroy.restype = None
        L.cc_firing_stamps_hip_stream.argtypes = [vp]
        L.cc_firing_stamps_hip_stream.restype = vp
        L.cc_firing_stamps_sync.argtypes = [vp]
        L.cc_firing_stamps_capacity.argtypes = [vp]
        L.cc_firing_stamps_capacity.restype = i64
        L.cc_firing_stamps_push.argtypes = [vp, i64, vp, i32]
        L.cc_firing_stamps_push_host.argtypes = [vp, i32, i64, vp]
        L.cc_firing_stamps_seek.argtypes = [vp, i32, u64]
        L.cc_firing_stamps_reset_streams.argtypes = [vp, i32, vp]
        L.cc_firing_stamps_counters.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(u64)]
        L.cc_firing_stamps_of_points.argtypes = [vp, i64, vp, vp, vp, vp]
        L.cc_firing_stamps_of_columns.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        L.cc_firing_stamps_of_clusters.argtypes = [vp, i32, i64, vp, i64, vp, vp, vp]
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_firing_stamps_last_error().decode())


def last_error() -> str:
    return _lib().cc_firing_stamps_last_error().decode()


def _stream_list(streams) -> np.ndarray:
    if isinstance(streams, (int, np.integer)):
        streams = [streams]
    return np.ascontiguousarray(list(streams), dtype=np.int32)


def _columns_of(table: np.ndarray) -> int:
    return int(np.maximum(table["col_to"] - table["col_from"], 0).sum())


def _n_records(records) -> int:
    """records: a [n, 32] uint8 array / tensor, or a structured numpy array of TAKE_POINT_DTYPE"""
    return 0 if records is None else int(records.shape[0])


# ---- host twins --------------------------------------------------------------------------------------------------------------

def round_capacity(capacity: int) -> int:
    """`capacity` rounded up to a power of two; 0 if it is not in 1 .. 2^31."""
    return int(_lib().cc_stamps_round_capacity(int(capacity)))


def host_sec_nsec(stamps) -> np.ndarray:
    """[n][2] uint32: seconds (truncated to 32 bits) and nanoseconds of stamps [n] (ros::Time::fromNSec)."""
    stamps = np.ascontiguousarray(stamps, dtype=np.uint64).reshape(-1)
    out = np.zeros((stamps.shape[0], 2), dtype=np.uint32)
    _check(_lib().cc_stamps_host_sec_nsec(stamps.shape[0], stamps.ctypes.data, out.ctypes.data))
    return out


def _host_records(records) -> np.ndarray:
    a = np.ascontiguousarray(records)
    if a.dtype != TAKE_POINT_DTYPE:
        a = a.reshape(-1).view(TAKE_POINT_DTYPE)
    return a.reshape(-1)


class HostFiringStamps:
    """The log and the three resolve rules on the CPU, over numpy arrays: what `FiringStamps` computes, bit for bit."""

    def __init__(self, num_streams: int, capacity: int):
        self.L = _lib()
        self.num_streams, self.capacity = int(num_streams), round_capacity(capacity)
        if self.num_streams < 1 or self.capacity == 0:
            raise ValueError("num_streams >= 1 and a capacity of 1 .. 2^31 firings are required")
        self.rings = np.zeros((self.num_streams, self.capacity), dtype=np.uint64)
        self.heads = np.zeros(self.num_streams, dtype=np.uint64)
        self.floors = np.zeros(self.num_streams, dtype=np.uint64)
        self.missing = np.zeros(self.num_streams, dtype=np.uint64)
        self._log = HostLog(self.num_streams, 0, self.capacity, self.rings.ctypes.data, self.heads.ctypes.data, self.floors.ctypes.data,
                            self.missing.ctypes.data)

    def push(self, stamps, repeat: int = 1):
        """stamps [S][n]: every stream advances by n * repeat firings."""
        stamps = np.ascontiguousarray(stamps, dtype=np.uint64).reshape(self.num_streams, -1)
        _check(self.L.cc_stamps_host_push(C.byref(self._log), -1, stamps.shape[1], stamps.ctypes.data, int(repeat)))

    def push_host(self, stream: int, stamps):
        stamps = np.ascontiguousarray(stamps, dtype=np.uint64).reshape(-1)
        _check(self.L.cc_stamps_host_push(C.byref(self._log), int(stream), stamps.shape[0], stamps.ctypes.data, 1))

    def seek(self, stream: int, next_firing: int):
        self.heads[stream] = self.floors[stream] = np.uint64(next_firing)

    def reset_streams(self, streams):
        for s in _stream_list(streams):
            self.heads[s] = self.floors[s] = self.missing[s] = 0

    def counters(self, stream: int = 0) -> tuple:
        return int(self.heads[stream]), int(self.missing[stream])

    def resolve(self, stream: int, firings):
        """(stamps [n], missing [n] bool) of the low-32-bit firing keys `firings` of `stream`; counts nothing."""
        f = np.ascontiguousarray(firings, dtype=np.uint32).reshape(-1)
        out, miss = np.zeros(f.shape[0], dtype=np.uint64), np.zeros(f.shape[0], dtype=np.uint8)
        _check(self.L.cc_stamps_host_resolve(C.byref(self._log), int(stream), f.shape[0], f.ctypes.data, out.ctypes.data, miss.ctypes.data))
        return out, miss.astype(bool)

    def of_points(self, records, table):
        """(stamps [n], sec_nsec [n][2]) of the records of a take_points and its table (TAKE_STREAM_DTYPE)."""
        rec, table = _host_records(records), np.ascontiguousarray(table, dtype=TAKE_STREAM_DTYPE)
        out, sn = np.zeros(len(rec), dtype=np.uint64), np.zeros((len(rec), 2), dtype=np.uint32)
        _check(self.L.cc_stamps_host_of_points(C.byref(self._log), len(rec), rec.ctypes.data, table.ctypes.data, out.ctypes.data, sn.ctypes.data))
        return out, sn

    def of_columns(self, records, table):
        """(column stamps [all columns of the table, by stream then column], stream stamps [S])."""
        rec, table = _host_records(records), np.ascontiguousarray(table, dtype=TAKE_STREAM_DTYPE)
        cols, streams = np.zeros(_columns_of(table), dtype=np.uint64), np.zeros(self.num_streams, dtype=np.uint64)
        _check(self.L.cc_stamps_host_of_columns(C.byref(self._log), len(rec), rec.ctypes.data, table.ctypes.data, cols.ctypes.data,
                                                streams.ctypes.data))
        return cols, streams

    def of_clusters(self, clusters, records, use_last_point: bool = False):
        """(cluster stamps [n_clusters] CLUSTER_STAMP_DTYPE, point stamps [n_records]) of the output of a take_clusters."""
        cl = np.ascontiguousarray(clusters)
        if cl.dtype != TAKE_CLUSTER_DTYPE:
            cl = cl.reshape(-1).view(TAKE_CLUSTER_DTYPE)
        cl, rec = cl.reshape(-1), _host_records(records)
        out, pts = np.zeros(len(cl), dtype=CLUSTER_STAMP_DTYPE), np.zeros(len(rec), dtype=np.uint64)
        _check(self.L.cc_stamps_host_of_clusters(C.byref(self._log), 1 if use_last_point else 0, len(cl), cl.ctypes.data, len(rec),
                                                 rec.ctypes.data, out.ctypes.data, pts.ctypes.data))
        return out, pts


# ---- device ------------------------------------------------------------------------------------------------------------------

class FiringStamps:
    """One cc_firing_stamps handle: the stamps of the last `capacity` firings (rounded up to a power of two) of `num_streams` streams in
    device memory. Push what you add to the engine, in the same order; reset what you reset. Pass hip_stream=engine.hip_stream() to chain
    with an engine; close the handle before that engine. Every call is asynchronous on the handle's HIP stream except `counters`; the
    resolve calls take torch CUDA tensors or raw device addresses and, where an output is None, allocate it with torch.empty. That
    stream is not torch's: call `sync()` before torch reads an output, and hand in only tensors torch has finished writing."""

    def __init__(self, num_streams: int, capacity: int, device: int = 0, hip_stream: int | None = None):
        self.L = _lib()
        self.num_streams, self.device = num_streams, device
        self.h = C.c_void_p()
        rc = self.L.cc_firing_stamps_create(C.byref(self.h), device, num_streams, int(capacity), hip_stream)
        if rc != 0:
            self.h = None
            _check(rc)
        self.capacity = int(self.L.cc_firing_stamps_capacity(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.cc_firing_stamps_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hip_stream(self) -> int:
        return self.L.cc_firing_stamps_hip_stream(self.h)

    def sync(self):
        _check(self.L.cc_firing_stamps_sync(self.h))

    # ---- the log
    def push_raw(self, n: int, d_stamps, repeat: int = 1) -> int:
        """cc_firing_stamps_push; returns the status code without raising."""
        return self.L.cc_firing_stamps_push(self.h, int(n), _ptr(d_stamps), int(repeat))

    def push(self, n: int, d_stamps, repeat: int = 1):
        """d_stamps [S][n] uint64 on the device: every stream advances by n * repeat firings, each stamp written `repeat` times in a row
        (repeat = columns per packet for packet stamps; 1 for a sweep's d_stamps). n * repeat must not exceed the capacity."""
        _check(self.push_raw(n, d_stamps, repeat))

    def push_host(self, stream: int, stamps):
        """stamps [n] (host): `stream` advances by n firings; for callers of the single-stream `Engine.add_firings`."""
        stamps = np.ascontiguousarray(stamps, dtype=np.uint64).reshape(-1)
        _check(self.L.cc_firing_stamps_push_host(self.h, int(stream), stamps.shape[0], stamps.ctypes.data))

    def seek(self, stream: int, next_firing: int):
        """head = next_firing, nothing held: attach to an engine stream that has consumed firings already."""
        _check(self.L.cc_firing_stamps_seek(self.h, int(stream), int(next_firing)))

    def reset_streams(self, streams):
        """head = 0, nothing held, missing = 0 for an int or an iterable of ints; call it with `Engine.reset_streams` / `Engine.reset`."""
        idx = _stream_list(streams)
        _check(self.L.cc_firing_stamps_reset_streams(self.h, len(idx), idx.ctypes.data if len(idx) else None))

    def counters(self, stream: int = 0) -> tuple:
        """(head, missing) of `stream`; synchronises."""
        head, missing = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.cc_firing_stamps_counters(self.h, int(stream), C.byref(head), C.byref(missing)))
        return int(head.value), int(missing.value)

    # ---- resolve
    def of_points_raw(self, n_records: int, d_records, d_table, d_stamps, d_sec_nsec=None) -> int:
        return self.L.cc_firing_stamps_of_points(self.h, int(n_records), _ptr(d_records), _ptr(d_table), _ptr(d_stamps), _ptr(d_sec_nsec))

    def of_points(self, records, d_table, stamps=None, sec_nsec=None, with_sec_nsec: bool = True):
        """records: what `Engine.take_points(..., d_table=d_table)` returned ([n, 32] uint8 CUDA tensor), d_table: the CUDA tensor that take
        filled. Returns (stamps [n] int64 CUDA tensor holding the uint64 bits, sec_nsec [n, 2] int32 CUDA tensor holding uint32 bits or
        None)."""
        import torch
        n = _n_records(records)
        if stamps is None:
            stamps = torch.empty(n, dtype=torch.int64, device="cuda")
        if sec_nsec is None and with_sec_nsec:
            sec_nsec = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        _check(self.of_points_raw(n, records, d_table, stamps, sec_nsec))
        return stamps[:n], (sec_nsec[:n] if sec_nsec is not None else None)

    def of_columns_raw(self, n_records: int, d_records, d_table, h_table, d_column_stamps, d_stream_stamps) -> int:
        h = None if h_table is None else np.ascontiguousarray(h_table, dtype=TAKE_STREAM_DTYPE)
        return self.L.cc_firing_stamps_of_columns(self.h, int(n_records), _ptr(d_records), _ptr(d_table), None if h is None else h.ctypes.data,
                                                  _ptr(d_column_stamps), _ptr(d_stream_stamps))

    def of_columns(self, records, d_table, table, column_stamps=None, stream_stamps=None):
        """table: the host table of the same take (sizes the output). Returns (column stamps, ordered by stream then column, one per column
        of every stream's [col_from, col_to); stream stamps [S]) as int64 CUDA tensors holding the uint64 bits: the minimum non-zero stamp,
        0 where there is none."""
        import torch
        n_cols = _columns_of(np.asarray(table))
        if column_stamps is None:
            column_stamps = torch.empty(max(n_cols, 1), dtype=torch.int64, device="cuda")
        if stream_stamps is None:
            stream_stamps = torch.empty(self.num_streams, dtype=torch.int64, device="cuda")
        _check(self.of_columns_raw(_n_records(records), records, d_table, table, column_stamps, stream_stamps))
        return column_stamps[:n_cols], stream_stamps

    def of_clusters_raw(self, use_last_point, n_clusters: int, d_clusters, n_records: int, d_records, d_out, d_point_stamps=None) -> int:
        return self.L.cc_firing_stamps_of_clusters(self.h, 1 if use_last_point else 0, int(n_clusters), _ptr(d_clusters), int(n_records),
                                                   _ptr(d_records), _ptr(d_out), _ptr(d_point_stamps))

    def of_clusters(self, clusters, records, use_last_point: bool = False, out=None, point_stamps=None, with_point_stamps: bool = False):
        """clusters [n, 64], records [m, 32]: what `Engine.take_clusters` returned. Returns (out [n, 32] uint8 CUDA tensor: view it through
        CLUSTER_STAMP_DTYPE after `.cpu().numpy()`; point stamps [m] int64 CUDA tensor or None). Stamps need the records: a take with
        `descriptors_only` has none."""
        import torch
        n, m = _n_records(clusters), _n_records(records)
        if out is None:
            out = torch.empty((max(n, 1), 32), dtype=torch.uint8, device="cuda")
        if point_stamps is None and with_point_stamps:
            point_stamps = torch.empty(max(m, 1), dtype=torch.int64, device="cuda")
        _check(self.of_clusters_raw(use_last_point, n, clusters, m, records, out, point_stamps))
        return out[:n], (point_stamps[:m] if point_stamps is not None else None)


__all__ = ["FiringStamps", "HostFiringStamps", "ClusterStamp", "HostLog", "CLUSTER_STAMP_DTYPE", "round_capacity", "host_sec_nsec", "last_error"]
