"""numpy restatement of the per-profile Ouster column decode (include/cc_ouster_profiles.h) the profile tests compare against. The offset
table below is written out from the profile table of DESIGN.md §12 on its own: it reads neither the library nor the packet writer of
continuous_clustering_amd.ouster. Returns what ouster_ref.decode returns."""
from __future__ import annotations

import numpy as np

LEGACY, SINGLE, DUAL = "LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG19_RFL8_SIG16_NIR16_DUAL"

# bytes before the first column and behind the last; column header; pixel; (status offset in the column or None = behind the last pixel,
# status dtype); range mask of the u32 at pixel byte 0; offset of the u16 SIGNAL in the pixel; column bytes behind the last pixel
TABLE = {
    LEGACY: dict(packet_header=0, packet_footer=0, column_header=16, pixel=12, status=(None, "<u4"), range_mask=0x000FFFFF, signal=6, trailer=4),
    SINGLE: dict(packet_header=32, packet_footer=32, column_header=12, pixel=12, status=(10, "<u2"), range_mask=0x0007FFFF, signal=6, trailer=0),
    DUAL: dict(packet_header=32, packet_footer=32, column_header=12, pixel=16, status=(10, "<u2"), range_mask=0x0007FFFF, signal=8, trailer=0),
}


def column_bytes(profile: str, rows: int) -> int:
    t = TABLE[profile]
    return t["column_header"] + t["pixel"] * rows + t["trailer"]


def packet_bytes(profile: str, rows: int, columns_per_packet: int) -> int:
    t = TABLE[profile]
    return t["packet_header"] + columns_per_packet * column_bytes(profile, rows) + t["packet_footer"]


def _field(a: np.ndarray, off: int, dt: str) -> np.ndarray:
    return np.ascontiguousarray(a[..., off:off + np.dtype(dt).itemsize]).view(dt)[..., 0]


def decode(profile: str, packets: np.ndarray, rows: int, columns_per_packet: int, direction: np.ndarray, offset: np.ndarray, skip=None,
           packet_poses=None) -> dict:
    """packets uint8 [..., P, bytes] of `profile` -> firings [..., P*C, ...] as cc_ouster_decode writes them, and the counters (summed
    over P). Only RANGE and SIGNAL of the first return are read, as by the reference (ouster_input.hpp:139-140)."""
    t = TABLE[profile]
    H, Cc, W = rows, columns_per_packet, direction.shape[0]
    *lead, P, nbytes = packets.shape
    cb = column_bytes(profile, H)
    assert nbytes == packet_bytes(profile, H, Cc), (nbytes, packet_bytes(profile, H, Cc))
    cols = np.ascontiguousarray(packets[..., t["packet_header"]:t["packet_header"] + Cc * cb]).reshape(*lead, P, Cc, cb)
    first_px = t["column_header"]
    end_px = first_px + t["pixel"] * H
    s_off, s_dt = t["status"]
    status = _field(cols, end_px if s_off is None else s_off, s_dt)
    mid = _field(cols, 8, "<u2").astype(np.int64)
    px = cols[..., first_px:end_px].reshape(*lead, P, Cc, H, t["pixel"])
    rng = _field(px, 0, "<u4") & np.uint32(t["range_mask"])
    sig = _field(px, t["signal"], "<u2")
    skip = np.zeros((*lead, P), dtype=bool) if skip is None else np.asarray(skip).astype(bool)
    live = np.broadcast_to(~skip[..., None], mid.shape)
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
        out["poses"] = np.repeat(np.asarray(packet_poses, dtype=np.float64), Cc, axis=-2)
    return out
