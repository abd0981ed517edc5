"""ctypes host mirror of include/cc_points.h — generic PointCloud2 firings decoded on the GPU into engine firings.

`PointsDecoder` runs the field reads of the reference's GenericPointsInput (ros/generic_points_input.hpp:21-53) as a HIP kernel and
writes the firings in the layout `Engine.add_firings_device` reads. The message layout is a run-time description (`Layout`, the
mirror of cc_points_layout): `layout_from_pointcloud2` derives it from the header of a sensor_msgs/PointCloud2, `raw_firing_layout` is
the reference's own RAW_POINT firing message. `write_messages` packs firings into message bytes (tests, and callers who replay recorded
firings). No ROS dependency, no CPU variant of the device decode.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, load_library

INTENSITY_REFERENCE, INTENSITY_U8, INTENSITY_F32_UNIT, INTENSITY_F32_255 = 0, 1, 2, 3
# sensor_msgs/PointField datatypes
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8
DATATYPE_BYTES = {INT8: 1, UINT8: 1, INT16: 2, UINT16: 2, INT32: 4, UINT32: 4, FLOAT32: 4, FLOAT64: 8}
PATH_GATHER, PATH_ROWS, PATH_MESSAGES = 0, 1, 2


class Layout(C.Structure):
    """cc_points_layout."""
    _fields_ = [("rows", C.c_int32), ("columns", C.c_int32), ("row_stride", C.c_int64), ("column_stride", C.c_int64),
                ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32), ("off_intensity", C.c_int32),
                ("intensity_mode", C.c_int32), ("reverse_rows", C.c_int32), ("message_bytes", C.c_int64)]

    def copy(self, **changes) -> "Layout":
        out = Layout.from_buffer_copy(bytes(self))
        for k, v in changes.items():
            setattr(out, k, v)
        return out

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}

    def __repr__(self):
        return "Layout(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32, lp = C.c_void_p, C.c_int, C.POINTER(Layout)
        L.cc_points_layout_check.argtypes = [lp]
        L.cc_points_path.argtypes = [lp]
        L.cc_points_column_tile.argtypes = [lp]
        L.cc_points_create.argtypes = [C.POINTER(vp), i32, i32, lp, i32, vp]
        L.cc_points_destroy.argtypes = [vp]
        L.cc_points_destroy.restype = None
        L.cc_points_last_error.restype = C.c_char_p
        L.cc_points_hip_stream.argtypes = [vp]
        L.cc_points_hip_stream.restype = vp
        L.cc_points_sync.argtypes = [vp]
        L.cc_points_check_engine.argtypes = [vp, vp]
        L.cc_points_decode.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp]
        L.cc_points_counters.argtypes = [vp, i32] + [C.POINTER(C.c_uint64)] * 2
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_points_last_error().decode())


# ---- layouts -----------------------------------------------------------------------------------------------------------------

def check_layout(layout: Layout):
    """Raise EngineError unless cc_points_create would take `layout` (cc_points_layout_check; needs no device)."""
    _check(_lib().cc_points_layout_check(C.byref(layout)))


def kernel_path(layout: Layout) -> int:
    """How the kernel walks `layout`: PATH_MESSAGES, PATH_ROWS or PATH_GATHER (cc_points_path); results never depend on it."""
    return int(_lib().cc_points_path(C.byref(layout)))


def column_tile(layout: Layout) -> int:
    """Firings one workgroup produces for `layout` (cc_points_column_tile): the column tile of a row-major organised cloud."""
    return int(_lib().cc_points_column_tile(C.byref(layout)))


def _intensity_bytes(mode: int) -> int:
    return 4 if mode in (INTENSITY_F32_UNIT, INTENSITY_F32_255) else 1


def layout_from_pointcloud2(height: int, width: int, point_step: int, row_step: int, fields, is_bigendian: bool = False,
                            intensity_mode: int = INTENSITY_REFERENCE, reverse_rows: bool = False) -> Layout:
    """The layout of an organised sensor_msgs/PointCloud2: `height` rows (lasers), `width` columns (firings; the reference's message has
    1). `fields`: [(name, offset, datatype, count), ...] as in sensor_msgs/PointField; "x", "y", "z" and "intensity" are found by name,
    as the iterators find them. Refused (ValueError): a missing or non-FLOAT32 x / y / z (the reference would reinterpret the bytes),
    a big-endian message, an intensity field whose datatype does not fit `intensity_mode` (UINT8 for INTENSITY_U8, FLOAT32 for the two
    F32 modes; INTENSITY_REFERENCE reads the first byte of any datatype, as the reference does). No intensity field: offset -1."""
    if is_bigendian:
        raise ValueError("big-endian PointCloud2 messages are not decoded")
    if intensity_mode not in (INTENSITY_REFERENCE, INTENSITY_U8, INTENSITY_F32_UNIT, INTENSITY_F32_255):
        raise ValueError(f"unknown intensity mode {intensity_mode}")
    by_name = {}
    for name, offset, datatype, count in fields:
        by_name.setdefault(name, (int(offset), int(datatype), int(count)))       # the iterator takes the first field of that name
    off = {}
    for name in ("x", "y", "z"):
        if name not in by_name:
            raise ValueError(f"the message has no field {name!r}")
        offset, datatype, _ = by_name[name]
        if datatype != FLOAT32:
            raise ValueError(f"field {name!r} has datatype {datatype}, not FLOAT32 ({FLOAT32})")
        off[name] = offset
    off_i = -1
    if "intensity" in by_name:
        off_i, datatype, _ = by_name["intensity"]
        want = {INTENSITY_U8: UINT8, INTENSITY_F32_UNIT: FLOAT32, INTENSITY_F32_255: FLOAT32}.get(intensity_mode)
        if want is not None and datatype != want:
            raise ValueError(f"field 'intensity' has datatype {datatype}; intensity mode {intensity_mode} reads datatype {want}")
    sizes = [4, 4, 4] + ([_intensity_bytes(intensity_mode)] if off_i >= 0 else [])
    offs = [off["x"], off["y"], off["z"]] + ([off_i] if off_i >= 0 else [])
    if any(o < 0 or o + n > point_step for o, n in zip(offs, sizes)):
        raise ValueError(f"a field does not lie inside point_step {point_step}")
    if height < 1 or width < 1 or row_step < width * point_step:
        raise ValueError("height and width must be >= 1 and row_step >= width * point_step")
    layout = Layout(rows=height, columns=width, row_stride=row_step, column_stride=point_step, off_x=off["x"], off_y=off["y"],
                    off_z=off["z"], off_intensity=off_i, intensity_mode=intensity_mode, reverse_rows=1 if reverse_rows else 0,
                    message_bytes=(height - 1) * row_step + width * point_step)
    try:
        check_layout(layout)
    except EngineError as e:
        raise ValueError(str(e)) from None
    return layout


# The reference's RAW_POINT message (prepareMessageAndCreateIterators with up_to_field 8, ros_utils.cpp:114-156; addRawPointToMessage,
# :300-317): what firingToPointCloud publishes per firing, height = number of lasers, width 1.
RAW_FIRING_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("firing_index", 12, FLOAT64, 1),
                     ("intensity", 20, UINT8, 1), ("globally_unique_point_index", 21, FLOAT64, 1), ("time_sec", 29, UINT32, 1),
                     ("time_nsec", 33, UINT32, 1)]
RAW_FIRING_POINT_STEP = 37


def raw_firing_layout(rows: int, intensity_mode: int = INTENSITY_REFERENCE) -> Layout:
    """The layout of the reference's own firing message: `rows` points of 37 bytes, width 1."""
    return layout_from_pointcloud2(rows, 1, RAW_FIRING_POINT_STEP, RAW_FIRING_POINT_STEP, RAW_FIRING_FIELDS, intensity_mode=intensity_mode)


def write_messages(xyz, intensity, layout: Layout, stride: int | None = None, fill=None) -> np.ndarray:
    """Firings -> message bytes, the inverse of the decode. xyz: float32 (or uint32 bit patterns) [..., F, H, 3], written bit for bit;
    F is a multiple of layout.columns and firing m * C + c becomes column c of message m. intensity [..., F, H]: uint8 = the value the
    decoder is to return (mode 0 stores the byte b with (b * 255) & 0xFF == value, mode 2 the float (value + 0.5) / 255, mode 3 the float
    value); a float32 array (modes 2 and 3 only) is written verbatim. Rows are written where the decoder reads them (reverse_rows).
    Every byte that is not x, y, z or intensity is filler: `fill` None = 0, an int = that byte, a numpy Generator = random bytes, a
    uint8 array of the result's shape = those bytes. Returns uint8 [..., F / C, stride], stride >= layout.message_bytes (default)."""
    H, Cn, mode = layout.rows, layout.columns, layout.intensity_mode
    bits = np.ascontiguousarray(xyz)
    if bits.dtype == np.float32:
        bits = bits.view(np.uint32)
    if bits.dtype != np.uint32 or bits.ndim < 3 or bits.shape[-2:] != (H, 3) or bits.shape[-3] % Cn:
        raise ValueError(f"xyz must be float32 / uint32 [..., F, {H}, 3] with F a multiple of {Cn}")
    lead, F = bits.shape[:-3], bits.shape[-3]
    M = F // Cn
    stride = int(layout.message_bytes if stride is None else stride)
    if stride < layout.message_bytes:
        raise ValueError(f"stride must be >= message_bytes ({layout.message_bytes})")
    shape = (*lead, M, stride)
    if fill is None or isinstance(fill, (int, np.integer)):
        out = np.full(shape, 0 if fill is None else int(fill), dtype=np.uint8)
    elif isinstance(fill, np.random.Generator):
        out = fill.integers(0, 256, shape, dtype=np.uint8)
    else:
        out = np.array(fill, dtype=np.uint8)
        if out.shape != shape:
            raise ValueError(f"fill must have the shape of the result, {shape}")
    inten = np.asarray(intensity)
    if inten.shape != (*lead, F, H):
        raise ValueError(f"intensity must be [..., F, {H}]")
    if np.issubdtype(inten.dtype, np.floating):
        if _intensity_bytes(mode) != 4:
            raise ValueError("a float intensity array needs intensity mode 2 or 3")
        ibytes = np.ascontiguousarray(inten, dtype=np.float32).view(np.uint8).reshape(*lead, F, H, 4)
    else:
        val = inten.astype(np.uint8)
        if mode == INTENSITY_REFERENCE:
            ibytes = ((256 - val.astype(np.int64)) & 0xFF).astype(np.uint8)[..., None]
        elif mode == INTENSITY_U8:
            ibytes = val[..., None]
        else:
            f = (val.astype(np.float64) + 0.5) / 255.0 if mode == INTENSITY_F32_UNIT else val.astype(np.float64)
            ibytes = np.ascontiguousarray(f.astype(np.float32)).view(np.uint8).reshape(*lead, F, H, 4)
    xbytes = bits.view(np.uint8).reshape(*lead, F, H, 3, 4)
    # byte position of (message row r, column c) inside a message; engine row e is message row r (H - 1 - r with reverse_rows)
    r = np.arange(H)[::-1] if layout.reverse_rows else np.arange(H)
    base = (r[None, :] * layout.row_stride + np.arange(Cn)[:, None] * layout.column_stride)             # [C][H(engine row)]
    flat = out.reshape(-1, M, stride)
    xb = xbytes.reshape(-1, M, Cn, H, 3, 4)
    ib = ibytes.reshape(-1, M, Cn, H, ibytes.shape[-1])
    for axis, off in enumerate((layout.off_x, layout.off_y, layout.off_z)):
        for b in range(4):
            flat[:, :, base + off + b] = xb[:, :, :, :, axis, b]
    if layout.off_intensity >= 0:
        for b in range(ib.shape[-1]):
            flat[:, :, base + layout.off_intensity + b] = ib[..., b]
    return out


# ---- device decode -----------------------------------------------------------------------------------------------------------

class PointsDecoder:
    """One cc_points handle: `num_streams` streams of messages that share `layout`, up to `max_messages` messages per stream and call.
    Pass hip_stream=engine.hip_stream() (and set the engine option "input_on_engine_stream") to chain the decode with an engine; close
    the decoder before that engine."""

    def __init__(self, num_streams: int, layout: Layout, max_messages: int = 64, device: int = 0, hip_stream: int | None = None):
        self.L = _lib()
        self.num_streams, self.max_messages, self.device = num_streams, max_messages, device
        self.layout = layout.copy()
        self.rows, self.columns = int(layout.rows), int(layout.columns)
        self.h = C.c_void_p()
        rc = self.L.cc_points_create(C.byref(self.h), device, num_streams, C.byref(self.layout), max_messages, hip_stream)
        if rc != 0:
            self.h = None
            _check(rc)

    def close(self):
        if getattr(self, "h", None):
            self.L.cc_points_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hip_stream(self) -> int:
        return self.L.cc_points_hip_stream(self.h)

    def check_engine(self, engine):
        """Raise unless the firings fit `engine` (same streams, the layout's rows)."""
        _check(self.L.cc_points_check_engine(self.h, engine.h))

    def decode_raw(self, n_messages: int, d_messages, message_stride: int, d_message_poses=None, d_skip=None, d_xyz=None,
                   d_intensity=None, d_poses=None) -> int:
        """cc_points_decode on device pointers / tensors; returns the status code without raising."""
        return self.L.cc_points_decode(self.h, n_messages, _ptr(d_messages), message_stride, _ptr(d_message_poses), _ptr(d_skip),
                                       _ptr(d_xyz), _ptr(d_intensity), _ptr(d_poses))

    def decode(self, messages, message_poses=None, skip=None, out: dict | None = None, n_messages: int | None = None,
               message_stride: int | None = None) -> dict:
        """messages: torch uint8 [S][M][stride] on the device, stride >= layout.message_bytes — or, for message bytes at an arbitrary
        byte offset of a buffer, any uint8 tensor that starts at the first message, with `n_messages` and `message_stride` given;
        message_poses: float64 [S][M][12] (None: out["poses"] is left as it is); skip: uint8 / bool [S][M]. Returns `out` (allocated when
        None): xyz [S][M*C][H][3], intensity [S][M*C][H], poses [S][M*C][12]. Asynchronous on the decoder's HIP stream: the inputs must
        be ready on the device."""
        import torch
        S = self.num_streams
        if n_messages is None:
            if messages.dim() != 3 or messages.shape[0] != S or messages.dtype != torch.uint8 or not messages.is_contiguous():
                raise ValueError(f"messages must be a contiguous uint8 tensor [{S}][M][stride]")
            M, stride = int(messages.shape[1]), int(messages.shape[2])
        else:
            M, stride = int(n_messages), int(message_stride)
            if messages.dtype != torch.uint8 or not messages.is_contiguous() or messages.numel() < S * M * stride:
                raise ValueError(f"messages must be a contiguous uint8 tensor of at least {S * M * stride} bytes")
        n = M * self.columns
        if message_poses is not None and (tuple(message_poses.shape) != (S, M, 12) or message_poses.dtype != torch.float64
                                          or not message_poses.is_contiguous()):
            raise ValueError(f"message_poses must be a contiguous float64 tensor [{S}][{M}][12]")
        torch_work = False   # work this call puts on torch's stream, which the decode (on another HIP stream) must not overtake
        if skip is not None:
            if tuple(skip.shape) != (S, M):
                raise ValueError(f"skip must be [{S}][{M}]")
            if skip.dtype != torch.uint8 or not skip.is_contiguous():
                skip, torch_work = skip.to(torch.uint8).contiguous(), True
        if out is None:
            dev = messages.device
            out = dict(xyz=torch.empty((S, n, self.rows, 3), dtype=torch.float32, device=dev),
                       intensity=torch.empty((S, n, self.rows), dtype=torch.uint8, device=dev),
                       poses=torch.empty((S, n, 12), dtype=torch.float64, device=dev))
            if message_poses is None:
                out["poses"].zero_()
                torch_work = True
        if torch_work:
            torch.cuda.current_stream(messages.device).synchronize()
        self._skip_keepalive = skip   # read asynchronously by the kernel
        _check(self.decode_raw(M, messages, stride, message_poses, skip, out["xyz"], out["intensity"], out.get("poses")))
        return out

    def sync(self):
        _check(self.L.cc_points_sync(self.h))

    def counters(self, stream: int | None = None):
        """Since creation: {"skipped_messages", "no_return_points"} of one stream, or a list of them for all streams (synchronises)."""
        if stream is None:
            return [self.counters(s) for s in range(self.num_streams)]
        v = [C.c_uint64(0) for _ in range(2)]
        _check(self.L.cc_points_counters(self.h, stream, *[C.byref(x) for x in v]))
        return dict(skipped_messages=int(v[0].value), no_return_points=int(v[1].value))


__all__ = ["PointsDecoder", "Layout", "layout_from_pointcloud2", "raw_firing_layout", "write_messages", "check_layout", "kernel_path",
           "column_tile", "RAW_FIRING_FIELDS", "RAW_FIRING_POINT_STEP", "INTENSITY_REFERENCE", "INTENSITY_U8", "INTENSITY_F32_UNIT",
           "INTENSITY_F32_255", "PATH_GATHER", "PATH_ROWS", "PATH_MESSAGES", "FLOAT32", "FLOAT64", "UINT8", "UINT32"]
