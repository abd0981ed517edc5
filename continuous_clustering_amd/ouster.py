"""ctypes host mirror of include/cc_ouster.h — Ouster LEGACY lidar packets decoded on the GPU into engine firings.

`OusterDecoder` runs the per-column decode of the reference's OusterInput (ros/ouster_input.hpp:105-181) as a HIP kernel and writes
the firings in the layout `Engine.add_firings_device` reads; `load_metadata` / `make_lut` turn a sensor metadata JSON into the
[W][H][3] look-up tables it takes (the SDK's make_xyz_lut, through `cc_ouster_make_lut`). `write_legacy_packets` and
`synthetic_packets` produce packets (no recording is available offline): ranges ray-cast against the synthetic scene of `synth`
along the LUT's beam directions. No CPU variant of the device decode.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import EngineError, _ptr, load_library, synth

HEADER_BYTES, PIXEL_BYTES, STATUS_BYTES = 16, 12, 4   # LEGACY column: header, per-pixel block, status word (include/cc_ouster.h)
RANGE_MASK = 0x000FFFFF
STATUS_VALID = 0xFFFFFFFF

_bound = False


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int
        L.cc_ouster_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, vp]
        L.cc_ouster_destroy.argtypes = [vp]
        L.cc_ouster_destroy.restype = None
        L.cc_ouster_last_error.restype = C.c_char_p
        L.cc_ouster_hip_stream.argtypes = [vp]
        L.cc_ouster_hip_stream.restype = vp
        L.cc_ouster_set_lut.argtypes = [vp, i32, i32, vp, vp]
        L.cc_ouster_decode.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.cc_ouster_counters.argtypes = [vp, i32] + [C.POINTER(C.c_uint64)] * 3
        L.cc_ouster_sync.argtypes = [vp]
        L.cc_ouster_packet_bytes.argtypes = [i32, i32]
        L.cc_ouster_packet_bytes.restype = C.c_int64
        L.cc_ouster_check_engine.argtypes = [vp, vp]
        L.cc_ouster_make_lut.argtypes = [i32, i32, C.c_double, vp, vp, vp, vp, vp]
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_ouster_last_error().decode())


def column_bytes(rows: int) -> int:
    return HEADER_BYTES + PIXEL_BYTES * rows + STATUS_BYTES


def packet_bytes(rows: int, columns_per_packet: int) -> int:
    return int(_lib().cc_ouster_packet_bytes(rows, columns_per_packet))


# ---- metadata and look-up table ----------------------------------------------------------------------------------------------

def load_metadata(path: str) -> dict:
    """The fields of an Ouster metadata JSON the decode needs (the reference reads it with metadata_from_json, ouster_input.hpp:58)."""
    with open(path) as f:
        j = json.load(f)
    fmt = j["data_format"]
    if fmt.get("udp_profile_lidar", "LEGACY") != "LEGACY":
        raise ValueError(f"{path}: udp_profile_lidar {fmt['udp_profile_lidar']} is not supported (LEGACY only)")
    return dict(rows=int(fmt["pixels_per_column"]), columns_per_frame=int(fmt["columns_per_frame"]),
                columns_per_packet=int(fmt["columns_per_packet"]),
                lidar_origin_to_beam_origin_mm=float(j["lidar_origin_to_beam_origin_mm"]),
                lidar_to_sensor_transform=np.asarray(j["lidar_to_sensor_transform"], dtype=np.float64).reshape(16),
                beam_azimuth_angles=np.asarray(j["beam_azimuth_angles"], dtype=np.float64),
                beam_altitude_angles=np.asarray(j["beam_altitude_angles"], dtype=np.float64))


def synthetic_metadata(rows: int = 64, columns_per_frame: int = 2048, columns_per_packet: int = 16) -> dict:
    """Metadata of a made-up LEGACY sensor (altitudes evenly spread over +-22.5 degrees, a small azimuth stagger per beam)."""
    return dict(rows=rows, columns_per_frame=columns_per_frame, columns_per_packet=columns_per_packet,
                lidar_origin_to_beam_origin_mm=15.8,
                lidar_to_sensor_transform=np.array([-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 38.195, 0, 0, 0, 1], dtype=np.float64),
                beam_azimuth_angles=np.array([(3.0 if r % 4 < 2 else -3.0) + 0.1 * (r % 2) for r in range(rows)], dtype=np.float64),
                beam_altitude_angles=np.linspace(22.5, -22.5, rows))


def make_lut(meta: dict, offset: str = "reference"):
    """(direction, offset), float32 [W][H][3] each, indexed [measurement_id][row]. offset="reference" passes the direction table as the
    offset, as the reference does (ouster_input.hpp:135-136: its points are r*d + d); offset="sdk" is the SDK's beam-origin offset."""
    if offset not in ("reference", "sdk"):
        raise ValueError("offset must be 'reference' or 'sdk'")
    W, H = meta["columns_per_frame"], meta["rows"]
    tf = np.ascontiguousarray(meta["lidar_to_sensor_transform"], dtype=np.float64).reshape(16)
    az = np.ascontiguousarray(meta["beam_azimuth_angles"], dtype=np.float64)
    alt = np.ascontiguousarray(meta["beam_altitude_angles"], dtype=np.float64)
    if az.shape != (H,) or alt.shape != (H,):
        raise ValueError("beam angle tables must have one entry per row")
    d = np.zeros((W, H, 3), dtype=np.float32)
    o = np.zeros((W, H, 3), dtype=np.float32)
    _check(_lib().cc_ouster_make_lut(W, H, float(meta["lidar_origin_to_beam_origin_mm"]), tf.ctypes.data, az.ctypes.data, alt.ctypes.data,
                                     d.ctypes.data, o.ctypes.data))
    return (d, d.copy()) if offset == "reference" else (d, o)


# ---- device decode -----------------------------------------------------------------------------------------------------------

class OusterDecoder:
    """One cc_ouster handle: `num_streams` sensors of `rows` beams, up to `max_packets` packets per stream and call. Pass
    hip_stream=engine.hip_stream() (and set the engine option "input_on_engine_stream") to chain the decode with an engine; close the
    decoder before that engine."""

    def __init__(self, num_streams: int, rows: int, columns_per_packet: int = 16, max_packets: int = 64, device: int = 0,
                 hip_stream: int | None = None):
        self.L = _lib()
        self.num_streams, self.rows, self.columns_per_packet, self.max_packets = num_streams, rows, columns_per_packet, max_packets
        self.device = device
        self.packet_bytes = packet_bytes(rows, columns_per_packet)
        self.h = C.c_void_p()
        rc = self.L.cc_ouster_create(C.byref(self.h), device, num_streams, rows, columns_per_packet, max_packets, hip_stream)
        if rc != 0:
            self.h = None
            _check(rc)

    def close(self):
        if getattr(self, "h", None):
            self.L.cc_ouster_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hip_stream(self) -> int:
        return self.L.cc_ouster_hip_stream(self.h)

    def check_engine(self, engine):
        """Raise unless the firings fit `engine` (same streams, rows == the engine's rows)."""
        _check(self.L.cc_ouster_check_engine(self.h, engine.h))

    def set_lut(self, direction, offset, stream: int = -1):
        d = np.ascontiguousarray(direction, dtype=np.float32)
        o = np.ascontiguousarray(offset, dtype=np.float32)
        if d.ndim != 3 or d.shape[1:] != (self.rows, 3) or o.shape != d.shape:
            raise ValueError(f"LUTs must be [W][{self.rows}][3]")
        _check(self.L.cc_ouster_set_lut(self.h, stream, d.shape[0], d.ctypes.data, o.ctypes.data))

    def decode_raw(self, n_packets: int, d_packets, d_packet_poses=None, d_skip=None, d_xyz=None, d_intensity=None, d_poses=None,
                   d_measurement_id=None) -> int:
        """cc_ouster_decode on device pointers / tensors; returns the status code without raising."""
        return self.L.cc_ouster_decode(self.h, n_packets, _ptr(d_packets), _ptr(d_packet_poses), _ptr(d_skip), _ptr(d_xyz), _ptr(d_intensity),
                                       _ptr(d_poses), _ptr(d_measurement_id))

    def decode(self, packets, packet_poses=None, skip=None, out: dict | None = None) -> dict:
        """packets: torch uint8 [S][P][packet_bytes] on the device; packet_poses: float64 [S][P][12] (None: out["poses"] is left as it
        is); skip: uint8 / bool [S][P]. Returns `out` (allocated when None): xyz [S][P*C][H][3], intensity [S][P*C][H],
        poses [S][P*C][12], measurement_id [S][P*C]. Asynchronous on the decoder's HIP stream: the inputs must be ready on the device."""
        import torch
        S, P = self.num_streams, int(packets.shape[1])
        n = P * self.columns_per_packet
        if tuple(packets.shape) != (S, P, self.packet_bytes) or packets.dtype != torch.uint8 or not packets.is_contiguous():
            raise ValueError(f"packets must be a contiguous uint8 tensor [{S}][P][{self.packet_bytes}]")
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
                       measurement_id=torch.empty((S, n), dtype=torch.int32, device=dev))
            if packet_poses is None:
                out["poses"].zero_()
                torch_work = True
        if torch_work:
            torch.cuda.current_stream(packets.device).synchronize()
        self._skip_keepalive = skip   # read asynchronously by the kernel
        _check(self.decode_raw(P, packets, packet_poses, skip, out["xyz"], out["intensity"], out.get("poses"), out.get("measurement_id")))
        return out

    def sync(self):
        _check(self.L.cc_ouster_sync(self.h))

    def counters(self, stream: int | None = None):
        """Placeholder columns since creation: {"invalid_columns", "bad_measurement_id", "skipped_packets"} of one stream, or a list of
        them for all streams (synchronises)."""
        if stream is None:
            return [self.counters(s) for s in range(self.num_streams)]
        v = [C.c_uint64(0) for _ in range(3)]
        _check(self.L.cc_ouster_counters(self.h, stream, *[C.byref(x) for x in v]))
        return dict(invalid_columns=int(v[0].value), bad_measurement_id=int(v[1].value), skipped_packets=int(v[2].value))


# ---- packets -----------------------------------------------------------------------------------------------------------------

def write_legacy_packets(ranges, signal, m_ids, status=None, timestamps=None, frame_id=None, encoder=None, reflectivity=None,
                         near_ir=None) -> np.ndarray:
    """LEGACY packets from per-pixel arrays [..., P, C, H] (ranges: the raw u32 word, high bits included) and per-column arrays
    [..., P, C] (status default 0xFFFFFFFF = valid). Returns uint8 [..., P, C * (20 + 12 H)]."""
    ranges = np.asarray(ranges)
    *lead, Cc, H = ranges.shape
    cols = np.zeros((*lead, Cc, column_bytes(H)), dtype=np.uint8)

    def put(arr, off, dt):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(arr), cols.shape[:-1]).astype(dt))
        n = np.dtype(dt).itemsize
        cols[..., off:off + n] = a[..., None].view(np.uint8)

    def put_px(arr, off, dt):
        if arr is None:
            return
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(arr), ranges.shape).astype(dt))
        n = np.dtype(dt).itemsize
        px = cols[..., HEADER_BYTES:HEADER_BYTES + PIXEL_BYTES * H].reshape(*lead, Cc, H, PIXEL_BYTES)
        px[..., off:off + n] = a[..., None].view(np.uint8)

    put(0 if timestamps is None else timestamps, 0, "<u8")
    put(m_ids, 8, "<u2")
    put(0 if frame_id is None else frame_id, 10, "<u2")
    put(0 if encoder is None else encoder, 12, "<u4")
    put_px(ranges, 0, "<u4")
    put_px(reflectivity, 4, "<u2")
    put_px(signal, 6, "<u2")
    put_px(near_ir, 8, "<u2")
    put(STATUS_VALID if status is None else status, HEADER_BYTES + PIXEL_BYTES * H, "<u4")
    return cols.reshape(*lead, Cc * column_bytes(H))


def synthetic_packets(meta: dict, n_packets: int, seed: int = 0, first_packet: int = 0, motion: synth.Motion | None = None,
                      scene: synth.SceneModel | None = None, rotation_hz: float = 10.0) -> dict:
    """`n_packets` consecutive packets of a sensor described by `meta`, starting at packet `first_packet` after power-up: ranges are
    ray-cast against the synthetic scene of synth (ground, cylinders, wall ring) along the LUT's beam directions from a sensor moving
    with `motion`. Returns dict(packets uint8 [P][bytes], packet_poses float64 [P][12] (odom_from_sensor at the packet's first column),
    ranges uint32 [P][C][H], signal uint16 [P][C][H], m_ids [P][C], status [P][C])."""
    motion = motion or synth.Motion.static()
    scene = scene or synth.SceneModel()
    H, W, Cc = meta["rows"], meta["columns_per_frame"], meta["columns_per_packet"]
    direction, _ = make_lut(meta, "sdk")
    unit = direction.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    cx, cy, rad = synth._scene_params(scene, seed)
    rng = np.random.default_rng(seed + 104729)
    j = (first_packet * Cc + np.arange(n_packets * Cc)).reshape(n_packets, Cc)   # column counter since power-up
    m_ids = (j % W).astype(np.uint16)
    tsec = j / (W * rotation_hz)

    def pose_at(t):
        yaw = t * motion.yaw_rate
        if motion.yaw_rate != 0.0:
            px = motion.velocity[0] * np.sin(yaw) / motion.yaw_rate
            py = motion.velocity[0] * (1.0 - np.cos(yaw)) / motion.yaw_rate
        else:
            px, py = t * motion.velocity[0], t * motion.velocity[1]
        return yaw, px, py, t * motion.velocity[2]

    yaw, px, py, pz = pose_at(tsec.reshape(-1))
    ds = unit[m_ids.reshape(-1)]                                                   # [F, H, 3] sensor frame
    cyw, syw = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
    dw = np.stack([cyw * ds[..., 0] - syw * ds[..., 1], syw * ds[..., 0] + cyw * ds[..., 1], ds[..., 2]], -1)
    o = np.stack([px, py, pz], -1)[:, None, :]
    t, _ = synth._cast(np, o, dw, cx, cy, rad, scene)
    F = t.shape[0]
    drop = rng.uniform(0, 1, (F, H)) < scene.dropout
    noise = rng.uniform(-scene.range_noise, scene.range_noise, (F, H))
    valid = (t < scene.max_range) & ~drop
    rng_mm = np.where(valid, np.clip(np.rint((np.where(valid, t, 0.0) + noise) * 1000.0), 1, RANGE_MASK), 0).astype(np.uint32)
    ranges = rng_mm.reshape(n_packets, Cc, H)
    signal = rng.integers(0, 1400, (n_packets, Cc, H), dtype=np.uint16)
    status = np.full((n_packets, Cc), STATUS_VALID, dtype=np.uint32)
    stamps = (tsec * 1e9).astype(np.uint64)
    packets = write_legacy_packets(ranges, signal, m_ids, status, timestamps=stamps, frame_id=(j // W).astype(np.uint16),
                                   encoder=(m_ids.astype(np.uint32) * (90112 // W)))
    yaw0, px0, py0, pz0 = pose_at(tsec[:, 0])
    c, s = np.cos(yaw0), np.sin(yaw0)
    z = np.zeros_like(c)
    poses = np.stack([c, -s, z, px0, s, c, z, py0, z, z, z + 1.0, pz0], -1)
    return dict(packets=packets, packet_poses=poses, ranges=ranges, signal=signal, m_ids=m_ids, status=status)


def rotation_packets(meta: dict) -> int:
    """Packets per rotation (W / C)."""
    return meta["columns_per_frame"] // meta["columns_per_packet"]


__all__ = ["OusterDecoder", "load_metadata", "make_lut", "synthetic_metadata", "write_legacy_packets", "synthetic_packets",
           "packet_bytes", "column_bytes", "rotation_packets", "RANGE_MASK", "STATUS_VALID"]
