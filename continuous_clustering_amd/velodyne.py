"""ctypes host mirror of include/cc_velodyne.h — Velodyne VLS-128 UDP payloads decoded on the GPU into engine firings.

`VelodyneDecoder` runs the decode the reference's VelodyneInput gets from the ROS driver's RawData::unpack_vls128
(ros/velodyne_input.hpp:46-91) as a HIP kernel and writes the firings in the layout `Engine.add_firings_device` reads; `load_calibration` /
`make_calibration` turn the driver's calibration YAML into the five per-laser arrays it takes (through `cc_velodyne_make_calibration`).
`write_packets` and `synthetic_packets` produce packets (no recording is available offline): distances ray-cast against the synthetic
scene of `synth` along the directions the decode gives each laser. No CPU variant of the device decode.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import EngineError, _ptr, load_library, synth

ROWS, FIRINGS_PER_PACKET, BLOCKS_PER_PACKET, LASERS_PER_BLOCK = 128, 3, 12, 32
PACKET_BYTES, BLOCK_BYTES = 1206, 100
BANK_HEADERS = (0xEEFF, 0xDDFF, 0xCCFF, 0xBBFF)          # lasers 0-31, 32-63, 64-95, 96-127
RETURN_MODE_STRONGEST, RETURN_MODE_LAST, RETURN_MODE_DUAL = 55, 56, 57
MODEL_VLS128 = 0xA1
DISTANCE_RESOLUTION = 0.004                              # metres per distance unit
SEQUENCE_SECONDS = 53.3e-6                               # one firing sequence of the 128 lasers (the driver's VLS128_SEQ_TDURATION)
CHANNEL_SECONDS = 2.665e-6                               # one group of 8 lasers (VLS128_CHANNEL_TDURATION)

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int
        L.cc_velodyne_create.argtypes = [C.POINTER(vp), i32, i32, i32, vp]
        L.cc_velodyne_destroy.argtypes = [vp]
        L.cc_velodyne_destroy.restype = None
        L.cc_velodyne_last_error.restype = C.c_char_p
        L.cc_velodyne_hip_stream.argtypes = [vp]
        L.cc_velodyne_hip_stream.restype = vp
        L.cc_velodyne_sync.argtypes = [vp]
        L.cc_velodyne_rows.argtypes = []
        L.cc_velodyne_firings_per_packet.argtypes = []
        L.cc_velodyne_check_engine.argtypes = [vp, vp]
        L.cc_velodyne_set_calibration.argtypes = [vp, i32, vp, vp, vp, vp, vp]
        L.cc_velodyne_decode.argtypes = [vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
        L.cc_velodyne_counters.argtypes = [vp, i32] + [C.POINTER(C.c_uint64)] * 3
        L.cc_velodyne_packet_bytes.argtypes = []
        L.cc_velodyne_packet_bytes.restype = C.c_int64
        L.cc_velodyne_rotation_tables.argtypes = [vp, vp]
        L.cc_velodyne_make_calibration.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp]
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_velodyne_last_error().decode())


# ---- calibration and rotation tables ----------------------------------------------------------------------------------------

CAL_ARRAYS = ("cos_rot_correction", "sin_rot_correction", "cos_vert_correction", "sin_vert_correction", "laser_ring")


def rotation_tables():
    """(cos, sin), float32 [36000] each: the tables the kernel looks the block azimuth up in (cc_velodyne_rotation_tables)."""
    c = np.zeros(36000, dtype=np.float32)
    s = np.zeros(36000, dtype=np.float32)
    _check(_lib().cc_velodyne_rotation_tables(c.ctypes.data, s.ctypes.data))
    return c, s


def make_calibration(rot_rad, vert_rad) -> dict:
    """The driver's per-laser rot_correction / vert_correction (radians, laser index order) as the five arrays the decoder takes:
    cos / sin of both angles (float32) and laser_ring (int32: rank of the vertical angle, the lower laser index first among equals).
    The angles are kept under "rot_correction" / "vert_correction"."""
    rot = np.ascontiguousarray(rot_rad, dtype=np.float64).reshape(-1)
    vert = np.ascontiguousarray(vert_rad, dtype=np.float64).reshape(-1)
    if rot.shape != vert.shape or rot.size < 1:
        raise ValueError("rot_rad and vert_rad must have one entry per laser")
    n = rot.size
    cal = {k: np.zeros(n, dtype=np.float32) for k in CAL_ARRAYS[:4]}
    cal["laser_ring"] = np.zeros(n, dtype=np.int32)
    _check(_lib().cc_velodyne_make_calibration(n, rot.ctypes.data, vert.ctypes.data, *[cal[k].ctypes.data for k in CAL_ARRAYS]))
    cal["rot_correction"], cal["vert_correction"] = rot, vert
    return cal


def load_calibration(path: str) -> dict:
    """make_calibration of the driver's calibration YAML (`lasers: [{laser_id, rot_correction, vert_correction, ...}]`, radians).
    Needs PyYAML; distance / offset corrections of the older models are not used by the VLS-128 decode and are ignored."""
    try:
        import yaml
    except ImportError:
        raise ImportError("load_calibration needs PyYAML to read the driver's calibration file; without it, pass the per-laser "
                          "rot_correction / vert_correction angles to make_calibration") from None
    with open(path) as f:
        doc = yaml.safe_load(f)
    lasers = doc.get("lasers") if isinstance(doc, dict) else None
    if not lasers:
        raise ValueError(f"{path}: no `lasers` list")
    n = int(doc.get("num_lasers", len(lasers)))
    if n != ROWS or len(lasers) != ROWS:
        raise ValueError(f"{path}: {len(lasers)} lasers (num_lasers {n}); the decoder is for the {ROWS}-laser VLS-128")
    rot, vert = np.zeros(n), np.zeros(n)
    seen = np.zeros(n, dtype=bool)
    for entry in lasers:
        i = int(entry["laser_id"])
        if not 0 <= i < n or seen[i]:
            raise ValueError(f"{path}: laser_id {i} is out of range or listed twice")
        seen[i] = True
        rot[i], vert[i] = float(entry["rot_correction"]), float(entry["vert_correction"])
    return make_calibration(rot, vert)


def synthetic_calibration(seed: int = 0) -> dict:
    """A MADE-UP 128-laser calibration (the sensor's real VLS128.yaml is not available here): vertical angles evenly spread over
    -25 .. +15 degrees and handed out to the lasers in a shuffled order, azimuth offsets from {+-6.354, +-4.548, +-2.732, +-0.911}
    degrees by laser index."""
    rng = np.random.default_rng(seed + 128)
    vert = np.deg2rad(np.linspace(-25.0, 15.0, ROWS))[rng.permutation(ROWS)]
    offsets = np.array([-6.354, -4.548, -2.732, -0.911, 0.911, 2.732, 4.548, 6.354])
    rot = np.deg2rad(offsets[np.arange(ROWS) % 8])
    return make_calibration(rot, vert)


# ---- device decode -----------------------------------------------------------------------------------------------------------

class VelodyneDecoder:
    """One cc_velodyne handle: `num_streams` VLS-128 sensors, up to `max_packets` packets per stream and call. Pass
    hip_stream=engine.hip_stream() (and set the engine option "input_on_engine_stream") to chain the decode with an engine; close the
    decoder before that engine."""

    def __init__(self, num_streams: int, max_packets: int = 64, device: int = 0, hip_stream: int | None = None):
        self.L = _lib()
        self.num_streams, self.max_packets, self.device = num_streams, max_packets, device
        self.rows, self.firings_per_packet = int(self.L.cc_velodyne_rows()), int(self.L.cc_velodyne_firings_per_packet())
        self.packet_bytes = int(self.L.cc_velodyne_packet_bytes())
        self.h = C.c_void_p()
        rc = self.L.cc_velodyne_create(C.byref(self.h), device, num_streams, max_packets, hip_stream)
        if rc != 0:
            self.h = None
            _check(rc)

    def close(self):
        if getattr(self, "h", None):
            self.L.cc_velodyne_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hip_stream(self) -> int:
        return self.L.cc_velodyne_hip_stream(self.h)

    def check_engine(self, engine):
        """Raise unless the firings fit `engine` (same streams, 128 rows)."""
        _check(self.L.cc_velodyne_check_engine(self.h, engine.h))

    def set_calibration(self, cal: dict, stream: int = -1):
        """`cal`: the dict of make_calibration / load_calibration / synthetic_calibration (or any mapping with the five arrays)."""
        arr = [np.ascontiguousarray(cal[k], dtype=np.float32) for k in CAL_ARRAYS[:4]]
        arr.append(np.ascontiguousarray(cal["laser_ring"], dtype=np.int32))
        if any(a.shape != (self.rows,) for a in arr):
            raise ValueError(f"calibration arrays must have {self.rows} entries")
        _check(self.L.cc_velodyne_set_calibration(self.h, stream, *[a.ctypes.data for a in arr]))

    def decode_raw(self, n_packets: int, d_packets, packet_stride: int = PACKET_BYTES, d_packet_poses=None, d_skip=None, d_xyz=None,
                   d_intensity=None, d_poses=None, d_block_azimuth=None) -> int:
        """cc_velodyne_decode on device pointers / tensors; returns the status code without raising."""
        return self.L.cc_velodyne_decode(self.h, n_packets, _ptr(d_packets), packet_stride, _ptr(d_packet_poses), _ptr(d_skip), _ptr(d_xyz),
                                         _ptr(d_intensity), _ptr(d_poses), _ptr(d_block_azimuth))

    def decode(self, packets, packet_poses=None, skip=None, out: dict | None = None) -> dict:
        """packets: torch uint8 [S][P][stride] on the device, stride an even number >= 1206; packet_poses: float64 [S][P][12] (None:
        out["poses"] is left as it is); skip: uint8 / bool [S][P]. Returns `out` (allocated when None): xyz [S][3P][128][3],
        intensity [S][3P][128], poses [S][3P][12], block_azimuth [S][3P]. Asynchronous on the decoder's HIP stream: the inputs must be
        ready on the device."""
        import torch
        S, P = self.num_streams, int(packets.shape[1])
        n = P * self.firings_per_packet
        if packets.dim() != 3 or packets.shape[0] != S or packets.shape[2] < self.packet_bytes or packets.shape[2] % 2 \
                or packets.dtype != torch.uint8 or not packets.is_contiguous():
            raise ValueError(f"packets must be a contiguous uint8 tensor [{S}][P][stride], stride even and >= {self.packet_bytes}")
        if packet_poses is not None and (tuple(packet_poses.shape) != (S, P, 12) or packet_poses.dtype != torch.float64
                                         or not packet_poses.is_contiguous()):
            raise ValueError(f"packet_poses must be a contiguous float64 tensor [{S}][{P}][12]")
        torch_work = False   # work this call puts on torch's stream, which the decode (on another HIP stream) must not overtake
        if skip is not None:
            if tuple(skip.shape) != (S, P):
                raise ValueError(f"skip must be [{S}][{P}]")
            if skip.dtype != torch.uint8 or not skip.is_contiguous():
                skip, torch_work = skip.to(torch.uint8).contiguous(), True
        if out is None:
            dev = packets.device
            out = dict(xyz=torch.empty((S, n, self.rows, 3), dtype=torch.float32, device=dev),
                       intensity=torch.empty((S, n, self.rows), dtype=torch.uint8, device=dev),
                       poses=torch.empty((S, n, 12), dtype=torch.float64, device=dev),
                       block_azimuth=torch.empty((S, n), dtype=torch.int32, device=dev))
            if packet_poses is None:
                out["poses"].zero_()
                torch_work = True
        if torch_work:
            torch.cuda.current_stream(packets.device).synchronize()
        self._skip_keepalive = skip   # read asynchronously by the kernel
        _check(self.decode_raw(P, packets, int(packets.shape[2]), packet_poses, skip, out["xyz"], out["intensity"], out.get("poses"),
                               out.get("block_azimuth")))
        return out

    def sync(self):
        _check(self.L.cc_velodyne_sync(self.h))

    def counters(self, stream: int | None = None):
        """Placeholders since creation: {"bad_block_header" (firing slots), "dual_return_packets", "skipped_packets"} of one stream, or
        a list of them for all streams (synchronises)."""
        if stream is None:
            return [self.counters(s) for s in range(self.num_streams)]
        v = [C.c_uint64(0) for _ in range(3)]
        _check(self.L.cc_velodyne_counters(self.h, stream, *[C.byref(x) for x in v]))
        return dict(bad_block_header=int(v[0].value), dual_return_packets=int(v[1].value), skipped_packets=int(v[2].value))


# ---- packets -----------------------------------------------------------------------------------------------------------------

def write_packets(raw_distance, intensity, rotation, headers=None, return_mode=RETURN_MODE_STRONGEST, stride: int = PACKET_BYTES,
                  timestamps=None) -> np.ndarray:
    """VLS-128 payloads from per-record arrays [..., P, 12, 32] (block, record; [..., P, 3, 128] = (firing slot, laser) is the same
    memory and is accepted too): raw_distance u16 in 0.004 m, intensity u8; per-block arrays [..., P, 12]: rotation u16 in 0.01
    degree, headers u16 (default: the four bank headers in order, three times); per-packet return_mode (byte 1204) and timestamps (u32
    at 1200). Returns uint8 [..., P, stride] with the bytes behind 1206 zero."""
    if stride < PACKET_BYTES:
        raise ValueError(f"stride must be >= {PACKET_BYTES}")
    raw = np.asarray(raw_distance)
    lead = raw.shape[:-2]
    if raw.shape[-2:] not in ((BLOCKS_PER_PACKET, LASERS_PER_BLOCK), (FIRINGS_PER_PACKET, ROWS)):
        raise ValueError("raw_distance must be [..., P, 12, 32] or [..., P, 3, 128]")
    rec_shape = (*lead, BLOCKS_PER_PACKET, LASERS_PER_BLOCK)
    raw = raw.reshape(rec_shape)
    inten = np.broadcast_to(np.asarray(intensity).reshape(rec_shape) if np.ndim(intensity) >= 2 else np.asarray(intensity), rec_shape)
    pk = np.zeros((*lead, stride), dtype=np.uint8)
    blocks = pk[..., :BLOCKS_PER_PACKET * BLOCK_BYTES].reshape(*lead, BLOCKS_PER_PACKET, BLOCK_BYTES)      # views into pk
    recs = blocks[..., 4:].reshape(*lead, BLOCKS_PER_PACKET, LASERS_PER_BLOCK, 3)

    def put(dst, shape, arr, off, dt):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(arr), shape).astype(dt))
        dst[..., off:off + np.dtype(dt).itemsize] = a[..., None].view(np.uint8)

    bshape = (*lead, BLOCKS_PER_PACKET)
    put(blocks, bshape, np.tile(np.array(BANK_HEADERS, dtype=np.uint16), FIRINGS_PER_PACKET) if headers is None else headers, 0, "<u2")
    put(blocks, bshape, rotation, 2, "<u2")
    put(recs, rec_shape, raw, 0, "<u2")
    put(recs, rec_shape, inten, 2, "u1")
    put(pk, lead, 0 if timestamps is None else timestamps, 1200, "<u4")
    put(pk, lead, return_mode, 1204, "u1")
    put(pk, lead, MODEL_VLS128, 1205, "u1")
    return pk


def corrected_azimuth(rotation) -> np.ndarray:
    """The azimuth (0.01 degree, 0..35999) the decode gives each laser of each firing slot: rotation int [..., 12] ->
    int32 [..., 3, 128] (include/cc_velodyne.h; float32 arithmetic as the driver's)."""
    rot = np.asarray(rotation).astype(np.int64)
    nxt = np.concatenate([rot[..., 1:], rot[..., -1:]], axis=-1)
    d = 36000 + nxt - rot
    diff = (np.sign(d) * (np.abs(d) % 36000)).astype(np.float32)                 # C's %: truncating toward zero
    diff[..., -1] = 0.0
    order = np.arange(16)
    frac = (np.float32(2.665) / np.float32(53.3)) * (order + order // 8).astype(np.float32)
    laser = np.arange(ROWS)
    block = 4 * np.arange(FIRINGS_PER_PACKET)[:, None] + (laser // 32)[None, :]   # [3, 128]
    a_f = rot[..., block].astype(np.float32) + diff[..., block] * frac[laser // 8]
    r = np.where(a_f >= 0, np.floor(a_f + np.float32(0.5)), np.ceil(a_f - np.float32(0.5)))   # exact here: a_f has at most 7 fraction bits
    return ((r.astype(np.int64) & 0xFFFF) % 36000).astype(np.int32)


def rotation_packets(rpm: float = 600.0) -> int:
    """Packets per rotation at `rpm` (a packet is 3 firing sequences of 53.3 us), rounded."""
    return int(round(60.0 / rpm / (FIRINGS_PER_PACKET * SEQUENCE_SECONDS)))


def synthetic_packets(cal: dict, n_packets: int, seed: int = 0, motion: synth.Motion | None = None, rpm: float = 600.0,
                      first_packet: int = 0, scene: synth.SceneModel | None = None, stride: int = PACKET_BYTES) -> dict:
    """`n_packets` consecutive packets of a sensor with calibration `cal`, starting at packet `first_packet` after power-up: distances
    are ray-cast against the synthetic scene of synth (ground, cylinders, wall ring) along the direction the decode gives each laser,
    from a sensor moving with `motion`. Block b of packet p is stamped (12 p + b) * 53.3 us / 4 and its rotation word advances with that
    time at `rpm`. Returns dict(packets uint8 [P][stride], packet_poses float64 [P][12] (odom_from_sensor at the packet's first block),
    raw_distance uint16 [P][12][32], intensity uint8 [P][12][32], rotation uint16 [P][12])."""
    motion = motion or synth.Motion.static()
    scene = scene or synth.SceneModel()
    cx, cy, rad = synth._scene_params(scene, seed)
    rng = np.random.default_rng(seed + 104729)
    rot_corr = np.asarray(cal["rot_correction"], dtype=np.float64)
    vert_corr = np.asarray(cal["vert_correction"], dtype=np.float64)
    cv, sv = np.cos(vert_corr), np.sin(vert_corr)
    laser = np.arange(ROWS)

    def pose_at(t):
        yaw = t * motion.yaw_rate
        if motion.yaw_rate != 0.0:
            px = motion.velocity[0] * np.sin(yaw) / motion.yaw_rate
            py = motion.velocity[0] * (1.0 - np.cos(yaw)) / motion.yaw_rate
        else:
            px, py = t * motion.velocity[0], t * motion.velocity[1]
        return yaw, px, py, t * motion.velocity[2]

    raws, intens, rots, poses = [], [], [], []
    for p0 in range(0, n_packets, 256):
        P = min(256, n_packets - p0)
        b = (first_packet + p0 + np.arange(P))[:, None] * BLOCKS_PER_PACKET + np.arange(BLOCKS_PER_PACKET)[None, :]
        tb = b * (SEQUENCE_SECONDS / 4)                                                    # [P, 12]
        rotation = (np.floor(tb * (rpm / 60.0) * 36000.0).astype(np.int64) % 36000).astype(np.uint16)
        a = corrected_azimuth(rotation).reshape(P * FIRINGS_PER_PACKET, ROWS)              # [F, 128] by laser
        ang = np.deg2rad(a * 0.01) - rot_corr[None, :]
        ds = np.stack([cv * np.cos(ang), -(cv * np.sin(ang)), np.broadcast_to(sv, ang.shape)], -1)   # sensor frame, as the decode
        # every laser of a firing sequence is cast from the pose at its own group's time (order * 2.665 us into the sequence)
        tf = tb[:, ::4].reshape(-1)[:, None] + (laser // 8 + laser // 64)[None, :] * CHANNEL_SECONDS
        yaw, px, py, pz = pose_at(tf)
        cyw, syw = np.cos(yaw), np.sin(yaw)
        dw = np.stack([cyw * ds[..., 0] - syw * ds[..., 1], syw * ds[..., 0] + cyw * ds[..., 1], ds[..., 2]], -1)
        F = dw.shape[0]
        # synth._cast takes one origin per firing: cast each laser as its own one-row firing
        t, _ = synth._cast(np, np.stack([px, py, pz], -1).reshape(F * ROWS, 1, 3), dw.reshape(F * ROWS, 1, 3), cx, cy, rad, scene)
        t = t.reshape(F, ROWS)
        drop = rng.uniform(0, 1, (F, ROWS)) < scene.dropout
        noise = rng.uniform(-scene.range_noise, scene.range_noise, (F, ROWS))
        valid = (t < scene.max_range) & ~drop
        raw = np.where(valid, np.clip(np.rint((np.where(valid, t, 0.0) + noise) / DISTANCE_RESOLUTION), 1, 65535), 0).astype(np.uint16)
        raws.append(raw.reshape(P, BLOCKS_PER_PACKET, LASERS_PER_BLOCK))
        intens.append(rng.integers(0, 256, (P, BLOCKS_PER_PACKET, LASERS_PER_BLOCK), dtype=np.uint8))
        rots.append(rotation)
        yaw0, px0, py0, pz0 = pose_at(tb[:, 0])
        c, s = np.cos(yaw0), np.sin(yaw0)
        z = np.zeros_like(c)
        poses.append(np.stack([c, -s, z, px0, s, c, z, py0, z, z, z + 1.0, pz0], -1))
    raw, inten, rotation = np.concatenate(raws), np.concatenate(intens), np.concatenate(rots)
    stamps = ((first_packet + np.arange(n_packets)) * (FIRINGS_PER_PACKET * SEQUENCE_SECONDS) * 1e6).astype(np.uint64) & 0xFFFFFFFF
    packets = write_packets(raw, inten, rotation, stride=stride, timestamps=stamps)
    return dict(packets=packets, packet_poses=np.concatenate(poses), raw_distance=raw, intensity=inten, rotation=rotation)


__all__ = ["VelodyneDecoder", "make_calibration", "load_calibration", "synthetic_calibration", "rotation_tables", "write_packets",
           "synthetic_packets", "corrected_azimuth", "rotation_packets", "ROWS", "FIRINGS_PER_PACKET", "PACKET_BYTES", "BANK_HEADERS",
           "RETURN_MODE_STRONGEST", "RETURN_MODE_LAST", "RETURN_MODE_DUAL"]
