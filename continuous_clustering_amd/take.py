"""ctypes host mirror of the hand-over functions of include/cc_hip.h (cc_engine_take_points / _take_cursor / _take_seek, DESIGN.md §15;
cc_engine_take_clusters / _take_clusters_cursor).

A take hands over, for all streams at once, the points of the columns that were published (stage CLUSTERED) or segmented (stage SEGMENTED)
since the previous take: compacted 32-byte records in DEVICE memory, ordered by stream, global column, row, plus one table entry per stream.
`Engine.take_points`, `Engine.take_cursor` and `Engine.take_seek` are these functions as methods. `take_clusters` hands over, again for all
streams at once, the clusters FINISHED since the previous one, published or not: one 64-byte descriptor per cluster ordered by stream and
id, and the member points as the same 32-byte records grouped by cluster (`Engine.take_clusters`, `_size`, `_cursor`). torch is imported only where a record
tensor has to be allocated; the package stays importable without it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, capi, load_library

TAKE_CLUSTERED, TAKE_SEGMENTED = 0, 1
TAKE_ALL_RETURNS, TAKE_NOT_GROUND, TAKE_WITH_ID = 0, 1, 2
TAKE_CLUSTERS_WITH_POINTS, TAKE_CLUSTERS_DESCRIPTORS_ONLY = 0, 1


class TakePoint(C.Structure):
    """cc_take_point."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("distance", C.c_float), ("id", C.c_uint32),
                ("source_firing", C.c_uint32), ("row", C.c_uint16), ("ground_point_label", C.c_uint8), ("intensity", C.c_uint8),
                ("column", C.c_uint32)]


class TakeStream(C.Structure):
    """cc_take_stream."""
    _fields_ = [("col_from", C.c_int64), ("col_to", C.c_int64), ("lost_columns", C.c_int64), ("first_record", C.c_int64),
                ("n_records", C.c_int64), ("error", C.c_int32), ("pad", C.c_int32)]


class TakeCluster(C.Structure):
    """cc_take_cluster."""
    _fields_ = [("stream", C.c_int32), ("id", C.c_uint32), ("col_from", C.c_int64), ("first_record", C.c_int64), ("n_points", C.c_uint32),
                ("n_columns", C.c_uint32), ("firing_min", C.c_uint32), ("firing_max", C.c_uint32), ("min_x", C.c_float),
                ("min_y", C.c_float), ("min_z", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float), ("max_z", C.c_float)]


class TakeClusterStream(C.Structure):
    """cc_take_cluster_stream."""
    _fields_ = [("id_from", C.c_int64), ("id_to", C.c_int64), ("lost_columns", C.c_int64), ("first_record", C.c_int64),
                ("n_records", C.c_int64), ("first_cluster", C.c_int32), ("n_clusters", C.c_int32), ("error", C.c_int32), ("pad", C.c_int32)]


TAKE_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("distance", "<f4"), ("id", "<u4"), ("source_firing", "<u4"),
                             ("row", "<u2"), ("ground_point_label", "u1"), ("intensity", "u1"), ("column", "<u4")])
TAKE_STREAM_DTYPE = np.dtype([("col_from", "<i8"), ("col_to", "<i8"), ("lost_columns", "<i8"), ("first_record", "<i8"),
                              ("n_records", "<i8"), ("error", "<i4"), ("pad", "<i4")])
TAKE_CLUSTER_DTYPE = np.dtype([("stream", "<i4"), ("id", "<u4"), ("col_from", "<i8"), ("first_record", "<i8"), ("n_points", "<u4"),
                               ("n_columns", "<u4"), ("firing_min", "<u4"), ("firing_max", "<u4"), ("min_x", "<f4"), ("min_y", "<f4"),
                               ("min_z", "<f4"), ("max_x", "<f4"), ("max_y", "<f4"), ("max_z", "<f4")])
TAKE_CLUSTER_STREAM_DTYPE = np.dtype([("id_from", "<i8"), ("id_to", "<i8"), ("lost_columns", "<i8"), ("first_record", "<i8"),
                                      ("n_records", "<i8"), ("first_cluster", "<i4"), ("n_clusters", "<i4"), ("error", "<i4"), ("pad", "<i4")])
assert TAKE_POINT_DTYPE.itemsize == C.sizeof(TakePoint) == 32
assert TAKE_CLUSTER_DTYPE.itemsize == C.sizeof(TakeCluster) == 64
assert TAKE_CLUSTER_STREAM_DTYPE.itemsize == C.sizeof(TakeClusterStream) == 56
assert TAKE_STREAM_DTYPE.itemsize == C.sizeof(TakeStream) == 48

# sensor_msgs/PointField datatypes
_PF_UINT8, _PF_UINT16, _PF_UINT32, _PF_FLOAT32 = 2, 4, 6, 7
_PF_OF = {"<f4": _PF_FLOAT32, "<u4": _PF_UINT32, "<u2": _PF_UINT16, "|u1": _PF_UINT8}


def pointcloud2_fields() -> list:
    """(name, offset, datatype, count) per field of cc_take_point: the `fields` of a sensor_msgs/PointCloud2 with point_step 32 whose
    `data` is a record array as it is."""
    return [(name, int(TAKE_POINT_DTYPE.fields[name][1]), _PF_OF[TAKE_POINT_DTYPE.fields[name][0].str], 1) for name in TAKE_POINT_DTYPE.names]


class TakeCapacityError(EngineError):
    """CC_ERR_CAPACITY of a take: `needed` records (of a cluster take also `needed_clusters` descriptors) do not fit the tensors that were
    passed; nothing was written, no cursor moved."""

    def __init__(self, msg: str, needed: int, table: np.ndarray, needed_clusters: int = 0):
        super().__init__(capi.CC_ERR_CAPACITY, msg)
        self.needed = needed
        self.table = table
        self.needed_clusters = needed_clusters


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
        L.cc_engine_take_points.argtypes = [vp, i32, i32, vp, i64, vp, vp, C.POINTER(i64)]
        L.cc_engine_take_cursor.argtypes = [vp, i32, i32, C.POINTER(i64), C.POINTER(i64)]
        L.cc_engine_take_seek.argtypes = [vp, i32, i32, i64]
        L.cc_engine_take_clusters.argtypes = [vp, C.c_uint32, i32, vp, i64, vp, i64, vp, vp, C.POINTER(i64), C.POINTER(i64)]
        L.cc_engine_take_clusters_cursor.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        _bound = True
    return L


def _take(engine, stage: int, select: int, ptr, capacity: int, d_table=None):
    L = _lib()
    table = np.zeros(engine.num_streams, dtype=TAKE_STREAM_DTYPE)
    n = C.c_int64(0)
    rc = L.cc_engine_take_points(engine.h, stage, select, ptr, capacity, _ptr(d_table), table.ctypes.data, C.byref(n))
    return rc, int(n.value), table


def take_size(engine, stage: int = TAKE_CLUSTERED, select: int = TAKE_ALL_RETURNS):
    """(records, table) the next take would hand over; moves no cursor."""
    rc, n, table = _take(engine, stage, select, None, 0)
    if rc not in (capi.CC_OK, capi.CC_ERR_CAPACITY):
        engine._check(rc)
    return n, table


def take_points(engine, stage: int = TAKE_CLUSTERED, select: int = TAKE_ALL_RETURNS, records=None, d_table=None):
    """Hand over what `stage` finished since the last take, of all streams. `records`: a contiguous torch uint8 CUDA tensor [capacity, 32],
    or None (a size query, an allocation of that size, the take). Returns (records[:n], table): the records viewed through
    TAKE_POINT_DTYPE after `.cpu().numpy().view(TAKE_POINT_DTYPE)`, the table a structured array (TAKE_STREAM_DTYPE) with one entry per
    stream. `d_table`: optional CUDA tensor of num_streams * 48 bytes that receives the table as well. Raises TakeCapacityError (an
    EngineError with `.needed`) when the tensor is too small; nothing has been taken then."""
    if records is None:
        import torch
        n, _ = take_size(engine, stage, select)
        records = torch.empty((max(n, 1), 32), dtype=torch.uint8, device="cuda")
    if records.dim() != 2 or records.shape[1] != 32 or records.element_size() != 1 or not records.is_contiguous() or not records.is_cuda:
        raise ValueError("records must be a contiguous uint8 CUDA tensor of shape [capacity, 32]")
    rc, n, table = _take(engine, stage, select, records.data_ptr(), int(records.shape[0]), d_table)
    if rc == capi.CC_ERR_CAPACITY:
        raise TakeCapacityError(engine.last_error(), n, table)
    engine._check(rc)
    return records[:n], table


def take_cursor(engine, stage: int = TAKE_CLUSTERED, stream: int = 0) -> tuple:
    """(cursor, readable_from) of (stage, stream): the first column the next take hands over unless it has been cleared, and the lowest
    column that has not been."""
    cur, lo = C.c_int64(0), C.c_int64(0)
    engine._check(_lib().cc_engine_take_cursor(engine.h, stage, stream, C.byref(cur), C.byref(lo)))
    return int(cur.value), int(lo.value)


def take_seek(engine, column: int, stage: int = TAKE_CLUSTERED, stream: int = -1):
    """Set the cursor of (stage, stream), stream -1: of all streams."""
    engine._check(_lib().cc_engine_take_seek(engine.h, stage, stream, int(column)))


# ---- finished clusters -----------------------------------------------------------------------------------------------------
def _take_clusters(engine, min_points: int, flags: int, cl_ptr, cl_cap: int, rec_ptr, rec_cap: int, d_table=None):
    L = _lib()
    table = np.zeros(engine.num_streams, dtype=TAKE_CLUSTER_STREAM_DTYPE)
    n, m = C.c_int64(0), C.c_int64(0)
    rc = L.cc_engine_take_clusters(engine.h, int(min_points), flags, cl_ptr, cl_cap, rec_ptr, rec_cap, _ptr(d_table), table.ctypes.data,
                                   C.byref(n), C.byref(m))
    return rc, int(n.value), int(m.value), table


def take_clusters_size(engine, min_points: int = 21):
    """(clusters, records, table) the next cluster take with this threshold would hand over; moves no cursor."""
    rc, n, m, table = _take_clusters(engine, min_points, TAKE_CLUSTERS_WITH_POINTS, None, 0, None, 0)
    if rc not in (capi.CC_OK, capi.CC_ERR_CAPACITY):
        engine._check(rc)
    return n, m, table


def take_clusters(engine, min_points: int = 21, descriptors_only: bool = False, clusters=None, records=None, d_table=None):
    """Hand over the clusters finished since the last cluster take, of all streams, that have at least `min_points` points (21: the
    reference's callback threshold; <= 6: every cluster that got an id). `clusters`: a contiguous torch uint8 CUDA tensor [capacity, 64],
    `records`: one of [capacity, 32]; None: a size query, an allocation of that size, the take (no record tensor with `descriptors_only`).
    Returns (clusters[:n], records[:m], table): view them through TAKE_CLUSTER_DTYPE / TAKE_POINT_DTYPE after `.cpu().numpy()`; cluster i
    owns records[first_record : first_record + n_points], ordered by (column, row), `column` counted from the cluster's col_from. With
    `descriptors_only` nothing is written to `records` and an empty slice comes back. `table`: a structured array
    (TAKE_CLUSTER_STREAM_DTYPE), one entry per stream; `d_table`: optional CUDA tensor of num_streams * 56 bytes that receives it as well.
    Raises TakeCapacityError (`.needed_clusters`, `.needed`) when either tensor is too small; nothing has been taken then."""
    flags = TAKE_CLUSTERS_DESCRIPTORS_ONLY if descriptors_only else TAKE_CLUSTERS_WITH_POINTS
    if clusters is None or (records is None and not descriptors_only):
        import torch
        n, m, _ = take_clusters_size(engine, min_points)
        if clusters is None:
            clusters = torch.empty((max(n, 1), 64), dtype=torch.uint8, device="cuda")
        if records is None and not descriptors_only:
            records = torch.empty((max(m, 1), 32), dtype=torch.uint8, device="cuda")
    for name, t, width in (("clusters", clusters, 64), ("records", records, 32)):
        if t is not None and (t.dim() != 2 or t.shape[1] != width or t.element_size() != 1 or not t.is_contiguous() or not t.is_cuda):
            raise ValueError(f"{name} must be a contiguous uint8 CUDA tensor of shape [capacity, {width}]")
    rec_ptr, rec_cap = (records.data_ptr(), int(records.shape[0])) if records is not None else (None, 0)
    rc, n, m, table = _take_clusters(engine, min_points, flags, clusters.data_ptr(), int(clusters.shape[0]), rec_ptr, rec_cap, d_table)
    if rc == capi.CC_ERR_CAPACITY:
        raise TakeCapacityError(engine.last_error(), m, table, needed_clusters=n)
    engine._check(rc)
    if descriptors_only:
        m = 0
    return clusters[:n], (records[:m] if records is not None else None), table


def take_clusters_cursor(engine, stream: int = 0) -> tuple:
    """(next_id, floor_column, readable_from) of `stream`: the first id the next cluster take examines, the lowest column it looks at unless
    that has been cleared, and the lowest column that has not been."""
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    engine._check(_lib().cc_engine_take_clusters_cursor(engine.h, stream, C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)
