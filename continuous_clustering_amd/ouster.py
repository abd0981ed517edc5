"""ctypes host mirror of include/cc_ouster.h and include/cc_ouster_profiles.h — Ouster lidar packets (LEGACY and the RNG19_RFL8_SIG16_NIR16
single- and dual-return UDP profiles) decoded on the GPU into engine firings.

`OusterDecoder` runs the per-column decode of the reference's OusterInput (ros/ouster_input.hpp:105-181) as a HIP kernel and writes
the firings in the layout `Engine.add_firings_device` reads; `load_metadata` / `make_lut` turn a sensor metadata JSON into the
[W][H][3] look-up tables it takes (the SDK's make_xyz_lut, through `cc_ouster_make_lut`). `write_legacy_packets`, `write_packets` and
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

# UDP profiles: the CC_OUSTER_PROFILE_* enum of include/cc_ouster_profiles.h, indexing PROFILE_NAMES (the metadata's udp_profile_lidar)
PROFILE_LEGACY, PROFILE_RNG19_RFL8_SIG16_NIR16, PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL = 0, 1, 2
PROFILE_NAMES = ("LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG19_RFL8_SIG16_NIR16_DUAL")
# what the packet writer needs of each profile (the table of include/cc_ouster_profiles.h): packet header (= footer) bytes, column
# header bytes, pixel bytes, column bytes behind the last pixel, range mask, and the offsets within a pixel of the fields it writes
_WIRE = (dict(packet_header=0, header=16, pixel=12, trailer=4, range_mask=0x000FFFFF, status_valid=0xFFFFFFFF),
         dict(packet_header=32, header=12, pixel=12, trailer=0, range_mask=0x0007FFFF, status_valid=0xFFFF,
              reflectivity=4, signal=6, near_ir=8),
         dict(packet_header=32, header=12, pixel=16, trailer=0, range_mask=0x0007FFFF, status_valid=0xFFFF,
              reflectivity=3, range2=4, reflectivity2=7, signal=8, signal2=10, near_ir=12))

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
        L.cc_ouster_create_profile.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32, i32, vp]
        L.cc_ouster_profile_packet_bytes.argtypes = [i32, i32, i32]
        L.cc_ouster_profile_packet_bytes.restype = C.c_int64
        L.cc_ouster_profile_from_name.argtypes = [C.c_char_p]
        L.cc_ouster_profile_of.argtypes = [vp]
        _bound = True
    return L


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, _lib().cc_ouster_last_error().decode())


def profile_id(profile) -> int:
    """The CC_OUSTER_PROFILE_* enum of a udp_profile_lidar name or of the enum itself. ValueError for a profile without a SIGNAL field
    (RNG15_RFL8_NIR8, FUSA_RNG15_RFL8_NIR8_DUAL) and for an unknown one."""
    if isinstance(profile, str):
        p = int(_lib().cc_ouster_profile_from_name(profile.encode()))
        if p == -2:
            raise ValueError(f"udp_profile_lidar {profile} has no SIGNAL field: the reference cannot run this profile")
        if p < 0:
            raise ValueError(f"udp_profile_lidar {profile} is unknown (supported: {', '.join(PROFILE_NAMES)})")
        return p
    p = int(profile)
    if not 0 <= p < len(PROFILE_NAMES):
        raise ValueError(f"no UDP profile {profile} (supported: 0..{len(PROFILE_NAMES) - 1}, {', '.join(PROFILE_NAMES)})")
    return p


def column_bytes(rows: int, profile="LEGACY") -> int:
    w = _WIRE[profile_id(profile)]
    return w["header"] + w["pixel"] * rows + w["trailer"]


def packet_bytes(rows: int, columns_per_packet: int, profile="LEGACY") -> int:
    return int(_lib().cc_ouster_profile_packet_bytes(profile_id(profile), rows, columns_per_packet))


# ---- metadata and look-up table ----------------------------------------------------------------------------------------------

def load_metadata(path: str) -> dict:
    """The fields of an Ouster metadata JSON the decode needs (the reference reads it with metadata_from_json, ouster_input.hpp:58)."""
    with open(path) as f:
        j = json.load(f)
    # the flat layout, or the newer nested one: lidar_data_format, beam_intrinsics, lidar_intrinsics
    fmt = j["lidar_data_format"] if "lidar_data_format" in j else j["data_format"]
    beam, lidar = j.get("beam_intrinsics", j), j.get("lidar_intrinsics", j)
    name = fmt.get("udp_profile_lidar", "LEGACY")
    try:
        profile_id(name)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    return dict(rows=int(fmt["pixels_per_column"]), columns_per_frame=int(fmt["columns_per_frame"]),
                columns_per_packet=int(fmt["columns_per_packet"]), udp_profile_lidar=name,
                lidar_origin_to_beam_origin_mm=float(beam["lidar_origin_to_beam_origin_mm"]),
                lidar_to_sensor_transform=np.asarray(lidar["lidar_to_sensor_transform"], dtype=np.float64).reshape(16),
                beam_azimuth_angles=np.asarray(beam["beam_azimuth_angles"], dtype=np.float64),
                beam_altitude_angles=np.asarray(beam["beam_altitude_angles"], dtype=np.float64))


def synthetic_metadata(rows: int = 64, columns_per_frame: int = 2048, columns_per_packet: int = 16, udp_profile_lidar: str = "LEGACY") -> dict:
    """Metadata of a made-up sensor (altitudes evenly spread over +-22.5 degrees, a small azimuth stagger per beam)."""
    profile_id(udp_profile_lidar)
    return dict(rows=rows, columns_per_frame=columns_per_frame, columns_per_packet=columns_per_packet, udp_profile_lidar=udp_profile_lidar,
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
    """One cc_ouster handle: `num_streams` sensors of `rows` beams and one UDP `profile` (a udp_profile_lidar name or the enum), up to
    `max_packets` packets per stream and call. Pass hip_stream=engine.hip_stream() (and set the engine option "input_on_engine_stream")
    to chain the decode with an engine; close the decoder before that engine."""

    def __init__(self, num_streams: int, rows: int, columns_per_packet: int = 16, max_packets: int = 64, device: int = 0,
                 hip_stream: int | None = None, profile="LEGACY"):
        self.L = _lib()
        self.num_streams, self.rows, self.columns_per_packet, self.max_packets = num_streams, rows, columns_per_packet, max_packets
        self.device = device
        self.profile = profile_id(profile)
        self.profile_name = PROFILE_NAMES[self.profile]
        self.packet_bytes = packet_bytes(rows, columns_per_packet, self.profile)
        self.h = C.c_void_p()
        if self.profile == PROFILE_LEGACY:
            rc = self.L.cc_ouster_create(C.byref(self.h), device, num_streams, rows, columns_per_packet, max_packets, hip_stream)
        else:
            rc = self.L.cc_ouster_create_profile(C.byref(self.h), device, num_streams, rows, columns_per_packet, max_packets, self.profile,
                                                 hip_stream)
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
            raise ValueError(f"packets must be a contiguous uint8 tensor [{S}][P][{self.packet_bytes}] ({self.profile_name} packets)")
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


def write_packets(profile, ranges, signal, m_ids, status=None, timestamps=None, frame_id=None, encoder=None, reflectivity=None, near_ir=None,
                  range2=None, signal2=None, reflectivity2=None, header=None, footer=None) -> np.ndarray:
    """Packets of `profile` (a name or the enum) from per-pixel arrays [..., P, C, H] (ranges, range2: the raw u32 word, the bits the
    profile's range mask removes included) and per-column arrays [..., P, C] (status default: all bits set = valid). LEGACY is
    write_legacy_packets. The RNG19 profiles have a 32-byte packet header and footer: `header` / `footer` uint8 [..., P, 32] are copied
    in as they are (default zeros, with frame_id as the u16 at header byte 2); `encoder` exists in LEGACY only. The 8-bit reflectivity
    is written after the range word, so in the dual profile (byte 3) it replaces that word's top byte; range2, signal2 and
    reflectivity2 (pixel byte 7, the top byte of the range2 word) exist in the dual profile only.
    Returns uint8 [..., P, packet_bytes]."""
    prof = profile_id(profile)
    if prof == PROFILE_LEGACY:
        if any(x is not None for x in (range2, signal2, reflectivity2, header, footer)):
            raise ValueError("LEGACY packets have no second return and no packet header or footer")
        return write_legacy_packets(ranges, signal, m_ids, status, timestamps, frame_id, encoder, reflectivity, near_ir)
    w = _WIRE[prof]
    if prof != PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL and any(x is not None for x in (range2, signal2, reflectivity2)):
        raise ValueError(f"{PROFILE_NAMES[prof]} packets have no second return")
    if encoder is not None:
        raise ValueError(f"{PROFILE_NAMES[prof]} columns have no encoder count")
    ranges = np.asarray(ranges)
    *lead, Cc, H = ranges.shape
    hb, pb, ph = w["header"], w["pixel"], w["packet_header"]
    cb = hb + pb * H + w["trailer"]
    pk = np.zeros((*lead, ph + Cc * cb + ph), dtype=np.uint8)
    cols = pk[..., ph:ph + Cc * cb].reshape(*lead, Cc, cb)                       # views into pk
    px = cols[..., hb:hb + pb * H].reshape(*lead, Cc, H, pb)

    def put(dst, shape, arr, off, dt):
        if arr is None:
            return
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(arr), shape).astype(dt))
        dst[..., off:off + np.dtype(dt).itemsize] = a[..., None].view(np.uint8)

    put(cols, cols.shape[:-1], 0 if timestamps is None else timestamps, 0, "<u8")
    put(cols, cols.shape[:-1], m_ids, 8, "<u2")
    put(cols, cols.shape[:-1], w["status_valid"] if status is None else status, 10, "<u2")
    put(px, ranges.shape, ranges, 0, "<u4")
    put(px, ranges.shape, range2, w.get("range2", 0), "<u4")
    put(px, ranges.shape, reflectivity, w["reflectivity"], "u1")
    put(px, ranges.shape, reflectivity2, w.get("reflectivity2", 0), "u1")
    put(px, ranges.shape, signal, w["signal"], "<u2")
    put(px, ranges.shape, signal2, w.get("signal2", 0), "<u2")
    put(px, ranges.shape, near_ir, w["near_ir"], "<u2")
    if header is not None:
        pk[..., :ph] = np.asarray(header, dtype=np.uint8)
    elif frame_id is not None:
        put(pk, pk.shape[:-1], np.broadcast_to(np.asarray(frame_id), cols.shape[:-1])[..., 0], 2, "<u2")   # its first column's
    if footer is not None:
        pk[..., ph + Cc * cb:] = np.asarray(footer, dtype=np.uint8)
    return pk


def synthetic_packets(meta: dict, n_packets: int, seed: int = 0, first_packet: int = 0, motion: synth.Motion | None = None,
                      scene: synth.SceneModel | None = None, rotation_hz: float = 10.0) -> dict:
    """`n_packets` consecutive packets of a sensor described by `meta`, starting at packet `first_packet` after power-up: ranges are
    ray-cast against the synthetic scene of synth (ground, cylinders, wall ring) along the LUT's beam directions from a sensor moving
    with `motion`. The packets are of the UDP profile `meta` names (LEGACY when it names none), ranges clipped to that profile's range
    mask. Returns dict(packets uint8 [P][bytes], packet_poses float64 [P][12] (odom_from_sensor at the packet's first column),
    ranges uint32 [P][C][H], signal uint16 [P][C][H], m_ids [P][C], status [P][C])."""
    motion = motion or synth.Motion.static()
    scene = scene or synth.SceneModel()
    H, W, Cc = meta["rows"], meta["columns_per_frame"], meta["columns_per_packet"]
    prof = profile_id(meta.get("udp_profile_lidar", "LEGACY"))
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
    rng_mm = np.where(valid, np.clip(np.rint((np.where(valid, t, 0.0) + noise) * 1000.0), 1, _WIRE[prof]["range_mask"]), 0).astype(np.uint32)
    ranges = rng_mm.reshape(n_packets, Cc, H)
    signal = rng.integers(0, 1400, (n_packets, Cc, H), dtype=np.uint16)
    status = np.full((n_packets, Cc), _WIRE[prof]["status_valid"], dtype=np.uint32)
    stamps = (tsec * 1e9).astype(np.uint64)
    packets = write_packets(prof, ranges, signal, m_ids, status, timestamps=stamps, frame_id=(j // W).astype(np.uint16),
                            encoder=(m_ids.astype(np.uint32) * (90112 // W)) if prof == PROFILE_LEGACY else None)
    yaw0, px0, py0, pz0 = pose_at(tsec[:, 0])
    c, s = np.cos(yaw0), np.sin(yaw0)
    z = np.zeros_like(c)
    poses = np.stack([c, -s, z, px0, s, c, z, py0, z, z, z + 1.0, pz0], -1)
    return dict(packets=packets, packet_poses=poses, ranges=ranges, signal=signal, m_ids=m_ids, status=status)


def rotation_packets(meta: dict) -> int:
    """Packets per rotation (W / C)."""
    return meta["columns_per_frame"] // meta["columns_per_packet"]


__all__ = ["OusterDecoder", "load_metadata", "make_lut", "synthetic_metadata", "write_legacy_packets", "write_packets", "synthetic_packets",
           "packet_bytes", "column_bytes", "rotation_packets", "profile_id", "RANGE_MASK", "STATUS_VALID", "PROFILE_NAMES", "PROFILE_LEGACY",
           "PROFILE_RNG19_RFL8_SIG16_NIR16", "PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL"]
