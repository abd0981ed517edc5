"""numpy restatements the Ouster decoder tests compare against (include/cc_ouster.h): the LEGACY column decode of the reference's
OusterInput (ouster_input.hpp:113-166, placeholders for what it drops) and the SDK's make_xyz_lut in the [m_id][row] order."""
from __future__ import annotations

import numpy as np

from continuous_clustering_amd import ouster


def make_lut(meta: dict):
    """(direction, offset) float32 [W][H][3], computed in double like the SDK, then cast."""
    W, H = meta["columns_per_frame"], meta["rows"]
    T = np.asarray(meta["lidar_to_sensor_transform"], dtype=np.float64).reshape(4, 4)
    v = np.arange(W, dtype=np.float64)[:, None]
    enc = 2.0 * np.pi - v * (np.pi * 2.0 / W)
    az = -np.asarray(meta["beam_azimuth_angles"], dtype=np.float64)[None, :] * np.pi / 180.0
    alt = np.asarray(meta["beam_altitude_angles"], dtype=np.float64)[None, :] * np.pi / 180.0
    d = np.stack([np.cos(enc + az) * np.cos(alt), np.sin(enc + az) * np.cos(alt), np.broadcast_to(np.sin(alt), (W, H))], -1)
    b = meta["lidar_origin_to_beam_origin_mm"]
    f = np.stack([(np.cos(enc) - d[..., 0]) * b, (np.sin(enc) - d[..., 1]) * b, (-d[..., 2]) * b], -1)

    def rot(x):
        return np.stack([(x[..., 0] * T[j, 0] + x[..., 1] * T[j, 1]) + x[..., 2] * T[j, 2] for j in range(3)], -1)

    dd = rot(d) * 0.001
    oo = (rot(f) + T[:3, 3]) * 0.001
    return dd.astype(np.float32), oo.astype(np.float32)


def decode(packets: np.ndarray, rows: int, columns_per_packet: int, direction: np.ndarray, offset: np.ndarray, skip=None,
           packet_poses=None) -> dict:
    """packets uint8 [..., P, bytes] -> firings [..., P*C, ...] as cc_ouster_decode writes them, and the counters (summed over P)."""
    H, Cc, W = rows, columns_per_packet, direction.shape[0]
    *lead, P, nbytes = packets.shape
    assert nbytes == Cc * ouster.column_bytes(H)
    cols = np.ascontiguousarray(packets).reshape(*lead, P, Cc, ouster.column_bytes(H))
    so = ouster.HEADER_BYTES + ouster.PIXEL_BYTES * H
    status = np.ascontiguousarray(cols[..., so:so + 4]).view("<u4")[..., 0]
    mid = np.ascontiguousarray(cols[..., 8:10]).view("<u2")[..., 0].astype(np.int64)
    px = cols[..., ouster.HEADER_BYTES:so].reshape(*lead, P, Cc, H, ouster.PIXEL_BYTES)
    rng = np.ascontiguousarray(px[..., 0:4]).view("<u4")[..., 0] & np.uint32(ouster.RANGE_MASK)
    sig = np.ascontiguousarray(px[..., 6:8]).view("<u2")[..., 0]
    skip = np.zeros((*lead, P), dtype=bool) if skip is None else np.asarray(skip).astype(bool)
    live = ~skip[..., None]
    ok_status = (status & 1) != 0
    valid = live & ok_status & (mid < W)
    m = np.where(valid, mid, 0)
    hit = valid[..., None] & (rng > 0)
    xyz = rng.astype(np.float32)[..., None] * direction[m] + offset[m]          # f32 multiply, then f32 add (SDK cartesianT)
    xyz = np.where(hit[..., None], xyz, np.float32(np.nan)).astype(np.float32)
    inten = (np.minimum(np.float32(1.0), sig.astype(np.float32) / np.float32(1000.0)) * np.float32(255.0)).astype(np.uint8)
    inten = np.where(hit, inten, 0).astype(np.uint8)
    out = dict(xyz=xyz.reshape(*lead, P * Cc, H, 3), intensity=inten.reshape(*lead, P * Cc, H),
               measurement_id=np.where(valid, mid, -1).astype(np.int32).reshape(*lead, P * Cc),
               valid=valid.reshape(*lead, P * Cc),
               invalid_columns=(live & ~ok_status).sum(axis=(-1, -2)), bad_measurement_id=(live & ok_status & (mid >= W)).sum(axis=(-1, -2)),
               skipped_packets=skip.sum(axis=-1))
    if packet_poses is not None:
        pp = np.asarray(packet_poses, dtype=np.float64)
        out["poses"] = np.repeat(pp, Cc, axis=-2)
    return out
