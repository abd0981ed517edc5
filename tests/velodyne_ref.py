"""numpy restatement the Velodyne decoder tests compare against: the VLS-128 decode specified in include/cc_velodyne.h (the ROS driver's
RawData::unpack_vls128 as the reference's VelodyneInput uses it, velodyne_input.hpp:46-91, with placeholders for what it drops).

Written from the specification, not from the kernel: one float32 numpy operation per rounding, integers in int64. The rotation tables
and the calibration arrays are inputs (the caller's, as the Ouster LUT is)."""
from __future__ import annotations

import numpy as np

PACKET_BYTES, BLOCKS, BLOCK_BYTES, RECORDS, SLOTS, LASERS = 1206, 12, 100, 32, 3, 128
BANKS = np.array([0xEEFF, 0xDDFF, 0xCCFF, 0xBBFF], dtype=np.int64)
F32 = np.float32


def fields(packets: np.ndarray) -> dict:
    """uint8 [..., stride >= 1206] -> header, rotation int64 [..., 12]; raw int64, intensity uint8 [..., 12, 32]; return_mode [...]."""
    pk = np.asarray(packets)[..., :PACKET_BYTES].astype(np.int64)
    blocks = pk[..., :BLOCKS * BLOCK_BYTES].reshape(*pk.shape[:-1], BLOCKS, BLOCK_BYTES)
    recs = blocks[..., 4:].reshape(*pk.shape[:-1], BLOCKS, RECORDS, 3)
    return dict(header=blocks[..., 0] + 256 * blocks[..., 1], rotation=blocks[..., 2] + 256 * blocks[..., 3],
                raw=recs[..., 0] + 256 * recs[..., 1], intensity=recs[..., 2].astype(np.uint8), return_mode=pk[..., 1204])


def valid_slots(header: np.ndarray) -> np.ndarray:
    """header int [..., 12] -> bool [..., 3]: slot f is valid iff its headers are the four banks in order and every earlier slot is."""
    own = (header.reshape(*header.shape[:-1], SLOTS, 4) == BANKS).all(-1)
    return np.logical_and.accumulate(own, axis=-1)


def block_azimuth_diff(rotation: np.ndarray) -> np.ndarray:
    """rotation int [..., 12] -> float32 [..., 12]: (float) ((36000 + next - this) % 36000) with C's truncating %, 0 for block 11."""
    rot = np.asarray(rotation).astype(np.int64)
    d = 36000 + rot[..., 1:] - rot[..., :-1]
    rem = np.where(d < 0, -((-d) % 36000), d % 36000)
    return np.concatenate([rem, np.zeros_like(rem[..., :1])], axis=-1).astype(F32)


def corrected_azimuth(rotation: np.ndarray) -> np.ndarray:
    """rotation int [..., 12] -> int64 [..., 12, 32]: the table index of record j of block b (laser j + 32 * (b % 4))."""
    rot = np.asarray(rotation).astype(np.int64)
    diff = block_azimuth_diff(rot)
    laser = np.arange(RECORDS)[None, :] + 32 * (np.arange(BLOCKS) % 4)[:, None]       # [12, 32]
    order = laser // 8
    frac = (F32(2.665) / F32(53.3)) * (order + order // 8).astype(F32)               # f32 quotient times f32
    prod = diff[..., None] * frac                                                     # f32, rounded
    a_f = rot.astype(F32)[..., None] + prod                                           # f32, rounded
    x = a_f.astype(np.float64)
    rounded = np.sign(x) * np.floor(np.abs(x) + 0.5)                                  # half away from zero, exact in double
    return (rounded.astype(np.int64) & 0xFFFF) % 36000


def decode(packets: np.ndarray, cos_tab: np.ndarray, sin_tab: np.ndarray, cal: dict, skip=None, packet_poses=None) -> dict:
    """packets uint8 [..., P, stride] -> firings [..., 3P, ...] as cc_velodyne_decode writes them, `valid` [..., 3P], and the counters
    (summed over P). cal: cos_rot_correction, sin_rot_correction, cos_vert_correction, sin_vert_correction, laser_ring (128 each)."""
    f = fields(packets)
    lead = f["header"].shape[:-1]                                                    # (..., P)
    skip = np.zeros(lead, dtype=bool) if skip is None else np.asarray(skip).astype(bool)
    dual = ~skip & (f["return_mode"] == 57)
    live = ~skip & ~dual
    slots = valid_slots(f["header"]) & live[..., None]                               # [..., P, 3]
    a = corrected_azimuth(f["rotation"])                                             # [..., P, 12, 32]
    ct, st = np.asarray(cos_tab, dtype=F32)[a], np.asarray(sin_tab, dtype=F32)[a]

    def by_record(x):                                                                # [128] by laser -> [12, 32] by (block, record)
        return np.tile(np.asarray(x).reshape(4, RECORDS), (SLOTS, 1))

    crc, src = by_record(cal["cos_rot_correction"]).astype(F32), by_record(cal["sin_rot_correction"]).astype(F32)
    cvc, svc = by_record(cal["cos_vert_correction"]).astype(F32), by_record(cal["sin_vert_correction"]).astype(F32)
    d = f["raw"].astype(F32) * F32(0.004)
    p1, p2 = ct * crc, st * src
    cr = p1 + p2
    p3, p4 = st * crc, ct * src
    sr = p3 - p4
    xy = d * cvc
    x = xy * cr
    y = -(xy * sr)
    z = d * svc
    hit = (f["raw"] > 0) & np.repeat(slots, 4, axis=-1)[..., None]                   # [..., P, 12, 32]
    nan = F32(np.nan)
    pts = np.stack([np.where(hit, x, nan), np.where(hit, y, nan), np.where(hit, z, nan)], -1).astype(F32)
    inten = np.where(hit, f["intensity"], 0).astype(np.uint8)
    # (block, record) -> (slot, laser) is a reshape; laser -> row 127 - ring
    row = LASERS - 1 - np.asarray(cal["laser_ring"]).astype(np.int64)
    assert sorted(row.tolist()) == list(range(LASERS))
    pts = pts.reshape(*lead, SLOTS, LASERS, 3)
    inten = inten.reshape(*lead, SLOTS, LASERS)
    xyz = np.empty_like(pts)
    xyz[..., row, :] = pts
    intensity = np.empty_like(inten)
    intensity[..., row] = inten
    *outer, P = lead
    first_rot = f["rotation"][..., ::4]
    out = dict(xyz=xyz.reshape(*outer, P * SLOTS, LASERS, 3), intensity=intensity.reshape(*outer, P * SLOTS, LASERS),
               block_azimuth=np.where(slots, first_rot, -1).astype(np.int32).reshape(*outer, P * SLOTS),
               valid=slots.reshape(*outer, P * SLOTS),
               bad_block_header=(live[..., None] & ~slots).sum(axis=(-1, -2)), dual_return_packets=dual.sum(axis=-1),
               skipped_packets=skip.sum(axis=-1))
    if packet_poses is not None:
        out["poses"] = np.repeat(np.asarray(packet_poses, dtype=np.float64), SLOTS, axis=-2)
    return out
