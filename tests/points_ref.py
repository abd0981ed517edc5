"""numpy restatement the generic PointCloud2 decoder tests compare against: the decode specified in include/cc_points.h (the field reads
of the reference's GenericPointsInput, generic_points_input.hpp:21-53, generalised to organised clouds, with placeholders for the
messages it drops).

Written from the header comment, not from the kernel: every output value is looked up at its byte address
m * stride + r * row_stride + c * column_stride + offset, one byte at a time, integers in int64."""
from __future__ import annotations

import numpy as np

QNAN_BITS = 0x7FC00000
MODE_REFERENCE, MODE_U8, MODE_F32_UNIT, MODE_F32_255 = 0, 1, 2, 3


def _get(layout, name):
    return int(layout[name] if isinstance(layout, dict) else getattr(layout, name))


def reference_intensity(b) -> np.ndarray:
    """Mode 0: static_cast<uint8_t>(*it * 255) of a uint8_t iterator: the first byte b, an int product, its low byte."""
    return ((np.asarray(b).astype(np.int64) * 255) & 0xFF).astype(np.uint8)


def unit_intensity(bits) -> np.ndarray:
    """Mode 2: f32 v -> p = v * 255 in f32; inside (-2^31, 2^31): the low byte of the two's-complement int32 truncated toward zero;
    otherwise (and NaN) 0."""
    v = np.asarray(bits, dtype=np.uint32).view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (v * np.float32(255.0)).astype(np.float32)
        ok = (p > np.float32(-2147483648.0)) & (p < np.float32(2147483648.0))      # False for NaN
        iv = np.trunc(np.where(ok, p, np.float32(0.0)).astype(np.float64)).astype(np.int64)
    return np.where(ok, iv & 0xFF, 0).astype(np.uint8)


def scale255_intensity(bits) -> np.ndarray:
    """Mode 3: f32 v on a 0..255 scale: NaN -> 0, otherwise clamped to [0, 255] and truncated."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)
        clamped = np.clip(np.where(np.isnan(v), 0.0, v), 0.0, 255.0)
    return np.trunc(clamped).astype(np.uint8)


def _u32_at(msg, addr):
    """Little-endian u32 at byte addresses `addr` (int64 array, indexing the last axis of msg [..., M, stride] per message)."""
    out = np.zeros(addr.shape, dtype=np.uint32)
    for b in range(4):
        out |= np.take_along_axis(msg, addr + b, axis=-1).astype(np.uint32) << np.uint32(8 * b)
    return out


def decode(messages, layout, skip=None, message_poses=None) -> dict:
    """messages uint8 [..., M, stride] -> dict(xyz uint32 [..., M*C, H, 3] (f32 bit patterns), intensity uint8 [..., M*C, H],
    poses float64 [..., M*C, 12] (None without message_poses), skipped_messages and no_return_points int64 [...] (counted over the
    messages axis)). skip bool [..., M]; message_poses float64 [..., M, 12]."""
    msg = np.asarray(messages)
    assert msg.dtype == np.uint8 and msg.ndim >= 2
    H, C = _get(layout, "rows"), _get(layout, "columns")
    rs, cs = _get(layout, "row_stride"), _get(layout, "column_stride")
    mode, off_i = _get(layout, "intensity_mode"), _get(layout, "off_intensity")
    lead, M, stride = msg.shape[:-2], msg.shape[-2], msg.shape[-1]
    assert stride >= _get(layout, "message_bytes")
    e = np.arange(H, dtype=np.int64)
    r = H - 1 - e if _get(layout, "reverse_rows") else e                          # message row of engine row e
    c = np.arange(C, dtype=np.int64)
    point = c[:, None] * cs + r[None, :] * rs                                      # [C][H] byte offset of the point in its message
    point = np.broadcast_to(point.reshape(C * H), (*lead, M, C * H))
    xyz = np.stack([_u32_at(msg, point + _get(layout, k)) for k in ("off_x", "off_y", "off_z")], axis=-1)   # [..., M, C*H, 3]
    if off_i < 0:
        inten = np.zeros((*lead, M, C * H), dtype=np.uint8)
    elif mode == MODE_REFERENCE:
        inten = reference_intensity(np.take_along_axis(msg, point + off_i, axis=-1))
    elif mode == MODE_U8:
        inten = np.take_along_axis(msg, point + off_i, axis=-1)
    elif mode == MODE_F32_UNIT:
        inten = unit_intensity(_u32_at(msg, point + off_i))
    elif mode == MODE_F32_255:
        inten = scale255_intensity(_u32_at(msg, point + off_i))
    else:
        raise ValueError(f"intensity mode {mode}")
    sk = np.zeros((*lead, M), dtype=bool) if skip is None else np.asarray(skip).astype(bool)
    assert sk.shape == (*lead, M)
    xyz = np.where(sk[..., None, None], np.uint32(QNAN_BITS), xyz)
    inten = np.where(sk[..., None], np.uint8(0), inten)
    x = xyz[..., 0]
    no_return = (((x & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)) & ~sk[..., None]).sum(axis=(-1, -2))
    poses = None
    if message_poses is not None:
        mp = np.asarray(message_poses, dtype=np.float64)
        assert mp.shape == (*lead, M, 12)
        poses = np.repeat(mp, C, axis=-2)                                          # firing m * C + c carries the pose of message m
    return dict(xyz=np.ascontiguousarray(xyz.reshape(*lead, M * C, H, 3)), intensity=np.ascontiguousarray(inten.reshape(*lead, M * C, H)),
                poses=poses, skipped_messages=sk.sum(axis=-1).astype(np.int64), no_return_points=no_return.astype(np.int64))
