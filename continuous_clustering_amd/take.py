"""ctypes host mirror of the hand-over functions of include/cc_hip.h (cc_engine_take_points / _take_cursor / _take_seek).

A take hands over, for all streams at once, the points of the columns that were published (stage CLUSTERED) or segmented (stage SEGMENTED)
since the previous take: compacted 32-byte records in DEVICE memory, ordered by stream, global column, row, plus one table entry per stream.
`Engine.take_points`, `Engine.take_cursor` and `Engine.take_seek` are these functions as methods. torch is imported only where a record
tensor has to be allocated; the package stays importable without it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, capi, load_library

TAKE_CLUSTERED, TAKE_SEGMENTED = 0, 1
TAKE_ALL_RETURNS, TAKE_NOT_GROUND, TAKE_WITH_ID = 0, 1, 2


class TakePoint(C.Structure):
    """cc_take_point."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("distance", C.c_float), ("id", C.c_uint32),
                ("source_firing", C.c_uint32), ("row", C.c_uint16), ("ground_point_label", C.c_uint8), ("intensity", C.c_uint8),
                ("column", C.c_uint32)]


class TakeStream(C.Structure):
    """cc_take_stream."""
    _fields_ = [("col_from", C.c_int64), ("col_to", C.c_int64), ("lost_columns", C.c_int64), ("first_record", C.c_int64),
                ("n_records", C.c_int64), ("error", C.c_int32), ("pad", C.c_int32)]


TAKE_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("distance", "<f4"), ("id", "<u4"), ("source_firing", "<u4"),
                             ("row", "<u2"), ("ground_point_label", "u1"), ("intensity", "u1"), ("column", "<u4")])
TAKE_STREAM_DTYPE = np.dtype([("col_from", "<i8"), ("col_to", "<i8"), ("lost_columns", "<i8"), ("first_record", "<i8"),
                              ("n_records", "<i8"), ("error", "<i4"), ("pad", "<i4")])
assert TAKE_POINT_DTYPE.itemsize == C.sizeof(TakePoint) == 32
assert TAKE_STREAM_DTYPE.itemsize == C.sizeof(TakeStream) == 48

# sensor_msgs/PointField datatypes
_PF_UINT8, _PF_UINT16, _PF_UINT32, _PF_FLOAT32 = 2, 4, 6, 7
_PF_OF = {"<f4": _PF_FLOAT32, "<u4": _PF_UINT32, "<u2": _PF_UINT16, "|u1": _PF_UINT8}


def pointcloud2_fields() -> list:
    """(name, offset, datatype, count) per field of cc_take_point: the `fields` of a sensor_msgs/PointCloud2 with point_step 32 whose
    `data` is a record array as it is."""
    return [(name, int(TAKE_POINT_DTYPE.fields[name][1]), _PF_OF[TAKE_POINT_DTYPE.fields[name][0].str], 1) for name in TAKE_POINT_DTYPE.names]


class TakeCapacityError(EngineError):
    """CC_ERR_CAPACITY of a take: `needed` records do not fit the tensor that was passed; nothing was written, no cursor moved."""

    def __init__(self, msg: str, needed: int, table: np.ndarray):
        super().__init__(capi.CC_ERR_CAPACITY, msg)
        self.needed = needed
        self.table = table


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
        L.cc_engine_take_points.argtypes = [vp, i32, i32, vp, i64, vp, vp, C.POINTER(i64)]
        L.cc_engine_take_cursor.argtypes = [vp, i32, i32, C.POINTER(i64), C.POINTER(i64)]
        L.cc_engine_take_seek.argtypes = [vp, i32, i32, i64]
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
