"""CPU: the host side of the Ouster UDP profiles (include/cc_ouster_profiles.h): exported names, pinned packet sizes, profile names,
refusals that come before the device check, the packet writer against the numpy decode of every profile (raw byte positions included) and
load_metadata on flat and nested metadata JSONs."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import ouster_profiles_ref as pref
from continuous_clustering_amd import capi, ouster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = [pref.LEGACY, pref.SINGLE, pref.DUAL]
SIZES = {pref.SINGLE: {(32, 16): 6400, (64, 16): 12544, (128, 16): 24832},
         pref.DUAL: {(32, 16): 8448, (64, 16): 16640, (128, 16): 33024}}


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    load_library()
    return ouster._lib()


def test_header_symbols_are_exported(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_ouster_profiles.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    assert names == ["cc_ouster_create_profile", "cc_ouster_profile_from_name", "cc_ouster_profile_of", "cc_ouster_profile_packet_bytes"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_ouster_profiles.h but not exported by libcc_hip.so"
    enum = dict(re.findall(r"(CC_OUSTER_PROFILE_[A-Z0-9_]+)\s*=\s*(\d+)", txt))
    assert enum == {"CC_OUSTER_PROFILE_LEGACY": "0", "CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16": "1",
                    "CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL": "2"}
    assert ouster.PROFILE_NAMES == (pref.LEGACY, pref.SINGLE, pref.DUAL)


def test_packet_sizes_are_pinned(lib):
    for name, sizes in SIZES.items():
        p = ouster.PROFILE_NAMES.index(name)
        for (H, Cc), want in sizes.items():
            assert lib.cc_ouster_profile_packet_bytes(p, H, Cc) == want, (name, H, Cc)
            assert ouster.packet_bytes(H, Cc, name) == want and ouster.packet_bytes(H, Cc, profile=p) == want
            assert pref.packet_bytes(name, H, Cc) == want
            assert 64 + Cc * ouster.column_bytes(H, name) == want
    for H, Cc in ((4, 1), (32, 16), (64, 16), (128, 16), (128, 64)):
        assert lib.cc_ouster_profile_packet_bytes(0, H, Cc) == lib.cc_ouster_packet_bytes(H, Cc) == Cc * (16 + 12 * H + 4)
        assert ouster.packet_bytes(H, Cc) == ouster.packet_bytes(H, Cc, "LEGACY") == lib.cc_ouster_packet_bytes(H, Cc)
        assert ouster.column_bytes(H) == ouster.column_bytes(H, "LEGACY") == 20 + 12 * H
    assert ouster.packet_bytes(4, 1, pref.SINGLE) == 124 and ouster.packet_bytes(4, 1, pref.DUAL) == 140
    for bad in ((3, 32, 16), (-1, 32, 16), (1, 0, 16), (2, 32, 0)):
        assert lib.cc_ouster_profile_packet_bytes(*bad) == 0, bad


def test_profile_from_name(lib):
    f = lib.cc_ouster_profile_from_name
    assert [f(n.encode()) for n in PROFILES] == [0, 1, 2]
    assert f(b"RNG15_RFL8_NIR8") == -2 and f(b"FUSA_RNG15_RFL8_NIR8_DUAL") == -2
    for garbage in (b"", b"legacy", b"RNG19_RFL8_SIG16_NIR16_", b"RNG19", b"LEGACY "):
        assert f(garbage) == -1, garbage
    assert f(None) == -1
    assert [ouster.profile_id(n) for n in PROFILES] == [0, 1, 2] and ouster.profile_id(2) == 2
    with pytest.raises(ValueError, match="no SIGNAL field: the reference cannot run this profile"):
        ouster.profile_id("RNG15_RFL8_NIR8")
    with pytest.raises(ValueError, match="unknown"):
        ouster.profile_id("RNG19")
    with pytest.raises(ValueError):
        ouster.profile_id(3)
    assert lib.cc_ouster_profile_of(None) == -1


def test_create_profile_checks_arguments_before_the_device(lib):
    import torch
    h = ctypes.c_void_p()
    assert lib.cc_ouster_create_profile(ctypes.byref(h), 0, 2, 32, 16, 8, 7, None) == capi.CC_ERR_INVALID_ARGUMENT and not h.value
    assert b"profile 7" in lib.cc_ouster_last_error()
    assert lib.cc_ouster_create_profile(ctypes.byref(h), 0, 2, 32, 16, 8, -1, None) == capi.CC_ERR_INVALID_ARGUMENT
    # C = 64, H = 128, dual: 32 + 64 * (12 + 16 * 128) + 32 = 131904 B do not fit the 64 KB of LDS a workgroup stages the packet in
    assert lib.cc_ouster_create_profile(ctypes.byref(h), 0, 2, 128, 64, 8, 2, None) == capi.CC_ERR_INVALID_ARGUMENT and not h.value
    assert b"131904" in lib.cc_ouster_last_error() and b"LDS" in lib.cc_ouster_last_error()
    assert lib.cc_ouster_create_profile(ctypes.byref(h), 0, 2, 30, 16, 8, 1, None) == capi.CC_ERR_INVALID_ARGUMENT   # H not a multiple of 4
    with pytest.raises(ouster.EngineError) as ei:
        ouster.OusterDecoder(2, 128, 64, max_packets=8, profile=pref.DUAL)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "131904" in str(ei.value)
    with pytest.raises(ValueError):
        ouster.OusterDecoder(2, 32, 16, profile="RNG15_RFL8_NIR8")
    for p in (0, 1, 2):
        rc = lib.cc_ouster_create_profile(ctypes.byref(h), 0, 2, 32, 16, 8, p, None)
        if torch.cuda.is_available():
            assert rc == capi.CC_OK and lib.cc_ouster_profile_of(h) == p
            lib.cc_ouster_destroy(h)
        else:
            assert rc == capi.CC_ERR_NO_DEVICE and not h.value
            assert b"no gfx950 device" in lib.cc_ouster_last_error()


def _u(b, off, n):
    return int.from_bytes(b[off:off + n].tobytes(), "little")


@pytest.mark.parametrize("profile", PROFILES)
def test_packet_writer_and_numpy_decode_round_trip(lib, profile):
    H, W, Cc, P = 8, 64, 4, 5
    t = pref.TABLE[profile]
    mask = t["range_mask"]
    rng = np.random.default_rng(21)
    d = rng.uniform(-1e-3, 1e-3, (W, H, 3)).astype(np.float32)
    o = rng.uniform(-0.05, 0.05, (W, H, 3)).astype(np.float32)
    ranges = rng.integers(1, mask + 1, (P, Cc, H), dtype=np.uint32)
    ranges[0, 0, :3] = 0
    ranges[0, 1, 0] = mask
    garbage = rng.integers(0, 1 << 32, (P, Cc, H), dtype=np.uint64).astype(np.uint32) & np.uint32(~mask & 0xFFFFFFFF)
    if profile == pref.DUAL:
        garbage &= np.uint32(0x00FFFFFF)                                         # byte 3 is the reflectivity
    signal = rng.integers(0, 1 << 16, (P, Cc, H), dtype=np.uint16)
    m_ids = rng.integers(0, W, (P, Cc)).astype(np.uint16)
    m_ids[1, 1], m_ids[1, 2] = W, 65535
    full = 0xFFFFFFFF if profile == pref.LEGACY else 0xFFFF
    status = np.full((P, Cc), full, dtype=np.uint32)
    status[2, 0], status[2, 1], status[3, 2] = 0, full - 1, 1
    m_ids[2, 1] = W + 3                                                           # invalid status wins over the bad m_id
    kw = {}
    if profile != pref.LEGACY:
        kw = dict(header=rng.integers(0, 256, (P, 32), dtype=np.uint8), footer=rng.integers(0, 256, (P, 32), dtype=np.uint8))
    if profile == pref.DUAL:
        kw.update(range2=rng.integers(0, 1 << 24, (P, Cc, H), dtype=np.uint32), signal2=rng.integers(0, 1 << 16, (P, Cc, H), dtype=np.uint16),
                  reflectivity=rng.integers(0, 256, (P, Cc, H), dtype=np.uint8), reflectivity2=rng.integers(0, 256, (P, Cc, H), dtype=np.uint8))
    near_ir = rng.integers(0, 1 << 16, (P, Cc, H), dtype=np.uint16)
    stamps = np.arange(P * Cc, dtype=np.uint64).reshape(P, Cc) * 781250 + 5
    pk = ouster.write_packets(profile, ranges | garbage, signal, m_ids, status, timestamps=stamps, near_ir=near_ir, **kw)
    assert pk.dtype == np.uint8 and pk.shape == (P, pref.packet_bytes(profile, H, Cc)) == (P, ouster.packet_bytes(H, Cc, profile))

    # raw byte positions, counted here from the profile table: packet header, column header, pixel
    ph, chd, pxb = (0, 16, 12) if profile == pref.LEGACY else (32, 12, 16 if profile == pref.DUAL else 12)
    cb = chd + pxb * H + (4 if profile == pref.LEGACY else 0)
    p, k, r = 3, 2, 5
    col = pk[p, ph + k * cb:ph + (k + 1) * cb]
    assert _u(col, 0, 8) == int(stamps[p, k]) and _u(col, 8, 2) == int(m_ids[p, k])
    if profile == pref.LEGACY:
        assert _u(col, 16 + 12 * H, 4) == 1 and _u(pk[2], 1 * cb + 16 + 12 * H, 4) == 0xFFFFFFFE
    else:
        assert _u(col, 10, 2) == 1 and _u(pk[2], ph + 1 * cb + 10, 2) == 0xFFFE
        assert np.array_equal(pk[:, :32], kw["header"]) and np.array_equal(pk[:, -32:], kw["footer"])
    px = col[chd + pxb * r:chd + pxb * (r + 1)]
    word = int(ranges[p, k, r] | garbage[p, k, r])
    if profile == pref.DUAL:
        assert _u(px, 0, 3) == word & 0xFFFFFF and px[3] == kw["reflectivity"][p, k, r]
        assert _u(px, 4, 3) == int(kw["range2"][p, k, r]) and px[7] == kw["reflectivity2"][p, k, r]    # RANGE2 u32 @4, refl2 u8 @7
        assert _u(px, 8, 2) == int(signal[p, k, r]) and _u(px, 10, 2) == int(kw["signal2"][p, k, r])   # SIGNAL @8, SIGNAL2 @10
        assert _u(px, 12, 2) == int(near_ir[p, k, r])
    else:
        assert _u(px, 0, 4) == word and _u(px, 6, 2) == int(signal[p, k, r]) and _u(px, 8, 2) == int(near_ir[p, k, r])

    skip = np.zeros(P, dtype=bool)
    skip[4] = True
    out = pref.decode(profile, pk, H, Cc, d, o, skip=skip)
    assert int(out["invalid_columns"]) == 2 and int(out["bad_measurement_id"]) == 2 and int(out["skipped_packets"]) == 1
    mid = out["measurement_id"].reshape(P, Cc)
    assert (mid[4] == -1).all() and mid[1, 1] == -1 and mid[1, 2] == -1 and mid[2, 0] == -1 and mid[2, 1] == -1 and mid[3, 2] == m_ids[3, 2]
    xyz, inten = out["xyz"].reshape(P, Cc, H, 3), out["intensity"].reshape(P, Cc, H)
    assert np.isnan(xyz[mid < 0]).all() and (inten[mid < 0] == 0).all()
    assert np.isnan(xyz[0, 0, :3]).all() and (inten[0, 0, :3] == 0).all() and not np.isnan(xyz[0, 0, 3:]).any()
    rr = np.float32(ranges[p, k, r])
    want = (rr * d[m_ids[p, k], r]).astype(np.float32) + o[m_ids[p, k], r]
    assert xyz[p, k, r].view(np.uint32).tolist() == want.astype(np.float32).view(np.uint32).tolist()
    assert inten[p, k, r] == np.uint8(min(np.float32(1), np.float32(signal[p, k, r]) / np.float32(1000)) * np.float32(255))
    # nothing but RANGE, SIGNAL, m_id and status reaches a firing
    clean = pref.decode(profile, ouster.write_packets(profile, ranges, signal, m_ids, status), H, Cc, d, o, skip=skip)
    for key in ("xyz", "intensity", "measurement_id"):
        assert np.array_equal(clean[key].view(np.uint8), out[key].view(np.uint8)), key
    if profile == pref.LEGACY:                                                    # the new writer and reference agree with the merged ones
        import ouster_ref
        assert np.array_equal(pk, ouster.write_legacy_packets(ranges | garbage, signal, m_ids, status, timestamps=stamps, near_ir=near_ir))
        old = ouster_ref.decode(pk, H, Cc, d, o, skip=skip)
        assert np.array_equal(old["xyz"].view(np.uint32), out["xyz"].view(np.uint32)) and np.array_equal(old["intensity"], out["intensity"])


def test_word_0x00080000_is_range_zero_under_the_19_bit_mask(lib):
    H, W, Cc = 4, 8, 1
    d = np.full((W, H, 3), 1e-3, dtype=np.float32)
    ranges = np.array([[[0x00080000, 1, 0x7FFFF, 0]]], dtype=np.uint32)
    nan = {}
    for profile in PROFILES:
        pk = ouster.write_packets(profile, ranges, np.full((1, Cc, H), 500), np.zeros((1, Cc), dtype=np.uint16))
        nan[profile] = np.isnan(pref.decode(profile, pk, H, Cc, d, d)["xyz"][0, :, 0]).tolist()
    assert nan[pref.LEGACY] == [False, False, False, True]
    assert nan[pref.SINGLE] == nan[pref.DUAL] == [True, False, False, True]


def _metadata_json(nested, profile):
    fmt = dict(columns_per_frame=512, columns_per_packet=16, pixels_per_column=4, column_window=[0, 511], udp_profile_imu="LEGACY")
    if profile is not None:
        fmt["udp_profile_lidar"] = profile
    beam = dict(beam_altitude_angles=[10.0, 3.5, -3.5, -10.0], beam_azimuth_angles=[1.5, -1.5, 1.25, -1.25], lidar_origin_to_beam_origin_mm=27.67)
    tf = dict(lidar_to_sensor_transform=[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 36.18, 0, 0, 0, 1])
    if nested:
        return dict(lidar_data_format=fmt, beam_intrinsics=dict(beam, beam_to_lidar_transform=[1, 0, 0, 27.67, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]),
                    lidar_intrinsics=tf, sensor_info=dict(prod_line="OS-1-4"))
    return dict(data_format=fmt, prod_line="OS-1-4", **beam, **tf)


@pytest.mark.parametrize("nested", [False, True], ids=["flat", "nested"])
def test_load_metadata_layouts_profiles_and_refusals(lib, tmp_path, nested):
    path = str(tmp_path / "meta.json")
    for profile in PROFILES + [None]:
        with open(path, "w") as f:
            json.dump(_metadata_json(nested, profile), f)
        meta = ouster.load_metadata(path)
        assert meta["udp_profile_lidar"] == (profile or "LEGACY")
        assert (meta["rows"], meta["columns_per_frame"], meta["columns_per_packet"]) == (4, 512, 16)
        assert meta["lidar_origin_to_beam_origin_mm"] == 27.67 and meta["lidar_to_sensor_transform"].shape == (16,)
        assert meta["lidar_to_sensor_transform"][11] == 36.18
        assert meta["beam_altitude_angles"].tolist() == [10.0, 3.5, -3.5, -10.0] and meta["beam_azimuth_angles"].tolist() == [1.5, -1.5, 1.25, -1.25]
        d, o = ouster.make_lut(meta, "sdk")
        assert d.shape == (512, 4, 3) and np.isfinite(o).all()
    for profile in ("RNG15_RFL8_NIR8", "FUSA_RNG15_RFL8_NIR8_DUAL"):
        with open(path, "w") as f:
            json.dump(_metadata_json(nested, profile), f)
        with pytest.raises(ValueError, match="no SIGNAL field: the reference cannot run this profile"):
            ouster.load_metadata(path)
    with open(path, "w") as f:
        json.dump(_metadata_json(nested, "RNG19_RFL8_SIG16"), f)
    with pytest.raises(ValueError, match="RNG19_RFL8_SIG16 is unknown"):
        ouster.load_metadata(path)


def test_synthetic_metadata_and_packets_follow_the_profile(lib):
    assert ouster.synthetic_metadata(32, 512)["udp_profile_lidar"] == "LEGACY"
    with pytest.raises(ValueError):
        ouster.synthetic_metadata(32, 512, udp_profile_lidar="RNG15_RFL8_NIR8")
    sps = {}
    for profile in PROFILES:
        meta = ouster.synthetic_metadata(8, 64, 4, udp_profile_lidar=profile)
        sp = sps[profile] = ouster.synthetic_packets(meta, 6, seed=3)
        assert sp["packets"].shape == (6, pref.packet_bytes(profile, 8, 4))
        d, o = ouster.make_lut(meta, "reference")
        out = pref.decode(profile, sp["packets"], 8, 4, d, o)
        assert out["valid"].all() and np.array_equal(out["measurement_id"], sp["m_ids"].reshape(-1))
        hit = ~np.isnan(out["xyz"][..., 0])
        assert np.array_equal(hit, sp["ranges"].reshape(-1, 8) > 0) and hit.any() and sp["ranges"].max() <= pref.TABLE[profile]["range_mask"]
    for key in ("ranges", "signal", "m_ids"):
        assert np.array_equal(sps[pref.LEGACY][key], sps[pref.SINGLE][key]) and np.array_equal(sps[pref.LEGACY][key], sps[pref.DUAL][key])
