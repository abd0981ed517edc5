"""CPU: the Ouster packet decoder's host side (include/cc_ouster.h) and the equivalence its placeholder firings rest on.

* every function the header declares is exported, and the device path refuses to run without a GPU;
* cc_ouster_make_lut against a numpy restatement of the SDK's make_xyz_lut on both OS-32 calibrations of the reference;
* the packet writer against the numpy decode (masked range bits, invalid status, m_id >= W, range 0);
* on the oracle: a stream whose dropped columns are fed as all-NaN firings gives the events, labels, ids and published columns of the
  stream without them.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import ouster_ref
import util
from continuous_clustering_amd import capi, ouster, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
META = {side: os.path.join(GOLDEN, f"ouster_os32_{side}_metadata.json") for side in ("left", "right")}


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    return load_library()


def test_header_symbols_are_exported_and_no_gpu_means_no_decoder(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_ouster.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    assert "cc_ouster_decode" in names and "cc_ouster_make_lut" in names and len(names) == 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_ouster.h but not exported by libcc_hip.so"
    import torch
    ouster._lib()
    h = ctypes.c_void_p()
    rc = lib.cc_ouster_create(ctypes.byref(h), 0, 2, 32, 16, 8, None)
    if torch.cuda.is_available():
        assert rc == capi.CC_OK
        lib.cc_ouster_destroy(h)
    else:
        assert rc == capi.CC_ERR_NO_DEVICE and not h.value
        assert b"no gfx950 device" in lib.cc_ouster_last_error()
    assert lib.cc_ouster_create(ctypes.byref(h), 0, 2, 30, 16, 8, None) == capi.CC_ERR_INVALID_ARGUMENT   # H not a multiple of 4
    assert ouster.packet_bytes(32, 16) == 6464 and ouster.packet_bytes(64, 16) == 12608 and ouster.packet_bytes(0, 16) == 0


@pytest.mark.parametrize("side", ["left", "right"])
def test_make_lut_matches_numpy_restatement(lib, side):
    meta = ouster.load_metadata(META[side])
    assert (meta["rows"], meta["columns_per_frame"], meta["columns_per_packet"]) == (32, 1024, 16)
    d, o = ouster.make_lut(meta, offset="sdk")
    rd, ro = ouster_ref.make_lut(meta)
    assert d.shape == (1024, 32, 3) and o.shape == (1024, 32, 3)
    for got, want in ((d, rd), (o, ro)):
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
    # [m_id][row] order: column 0 looks along the sensor's -x (lidar_to_sensor_transform turns the lidar frame by pi about z), the
    # beam's own azimuth offset to the right of it; row 0 is the top beam (altitude 46.09 deg)
    assert np.isclose(np.linalg.norm(d, axis=-1), 0.001, rtol=1e-6).all()
    assert np.isclose(np.arcsin(d[0, :, 2] / 0.001) * 180 / np.pi, meta["beam_altitude_angles"], atol=1e-4).all()
    az = np.degrees(np.arctan2(d[:, 0, 1], d[:, 0, 0]))
    assert abs((az[0] - (180.0 - meta["beam_azimuth_angles"][0]) + 180.0) % 360.0 - 180.0) < 1e-3
    assert np.isclose((az[0] - az[256]) % 360.0, 90.0, atol=1e-3)     # W / 4 columns later the beam has turned a quarter clockwise
    # the reference passes the direction block as the offset (ouster_input.hpp:135-136); the SDK offset is the beam origin, ~ mm away
    rdir, roff = ouster.make_lut(meta, offset="reference")
    assert np.array_equal(rdir, d) and np.array_equal(roff, d)
    beam = o - np.array([0.0, 0.0, meta["lidar_to_sensor_transform"][11] * 0.001], dtype=np.float32)
    assert 0.0 < np.abs(beam).max() < 2 * meta["lidar_origin_to_beam_origin_mm"] * 0.001
    assert not np.array_equal(o, d)


def test_packet_writer_and_numpy_decode_round_trip(lib):
    meta = ouster.load_metadata(META["left"])
    H, W, Cc = 32, 1024, 16
    d, o = ouster.make_lut(meta, offset="sdk")
    rng = np.random.default_rng(7)
    P = 5
    ranges = rng.integers(0, 1 << 20, (P, Cc, H), dtype=np.uint32)
    ranges[0, 0, :4] = 0                                                          # no return
    garbage = rng.integers(0, 1 << 12, (P, Cc, H), dtype=np.uint32) << np.uint32(20)
    signal = rng.integers(0, 1 << 16, (P, Cc, H), dtype=np.uint16)
    m_ids = rng.integers(0, W, (P, Cc)).astype(np.uint16)
    m_ids[1, 3] = W                                                               # out of the LUT
    m_ids[1, 4] = 65535
    status = np.full((P, Cc), 0xFFFFFFFF, dtype=np.uint32)
    status[2, 5] = 0                                                              # invalid column
    status[2, 6] = 0xFFFFFFFE                                                     # bit 0 clear: invalid too
    status[3, 7] = 0x00000001                                                     # bit 0 set: valid
    m_ids[2, 6] = W + 3                                                           # invalid status wins over the bad m_id
    pk = ouster.write_legacy_packets(ranges | garbage, signal, m_ids, status, timestamps=np.arange(P * Cc).reshape(P, Cc) * 781250)
    assert pk.shape == (P, 6464) and pk.dtype == np.uint8
    # raw field positions of the LEGACY table
    col = pk[1, 3 * 404:4 * 404]                                                 # 404 B per column: 16 + 12 * 32 + 4
    assert int.from_bytes(col[8:10].tobytes(), "little") == W
    assert int.from_bytes(col[16 + 12 * 2:16 + 12 * 2 + 4].tobytes(), "little") == int(ranges[1, 3, 2] | garbage[1, 3, 2])
    assert int.from_bytes(col[16 + 12 * 2 + 6:16 + 12 * 2 + 8].tobytes(), "little") == int(signal[1, 3, 2])
    assert int.from_bytes(pk[2, 5 * 404 + 400:6 * 404].tobytes(), "little") == 0
    skip = np.zeros(P, dtype=bool)
    skip[4] = True
    out = ouster_ref.decode(pk, H, Cc, d, o, skip=skip)
    assert int(out["invalid_columns"]) == 2 and int(out["bad_measurement_id"]) == 2 and int(out["skipped_packets"]) == 1
    mid = out["measurement_id"].reshape(P, Cc)
    assert (mid[4] == -1).all() and mid[1, 3] == -1 and mid[1, 4] == -1 and mid[2, 5] == -1 and mid[2, 6] == -1 and mid[3, 7] == m_ids[3, 7]
    xyz = out["xyz"].reshape(P, Cc, H, 3)
    inten = out["intensity"].reshape(P, Cc, H)
    placeholder = mid < 0
    assert np.isnan(xyz[placeholder]).all() and (inten[placeholder] == 0).all()
    assert np.isnan(xyz[0, 0, :4]).all() and (inten[0, 0, :4] == 0).all()
    # a valid pixel: masked range, f32 r * d + o, intensity from signal
    p, k, r = 3, 7, 9
    rr = np.float32(ranges[p, k, r] & 0xFFFFF)
    assert rr > 0
    want = rr * d[m_ids[p, k], r] + o[m_ids[p, k], r]
    assert xyz[p, k, r].view(np.uint32).tolist() == want.astype(np.float32).view(np.uint32).tolist()
    assert inten[p, k, r] == np.uint8(min(np.float32(1), np.float32(signal[p, k, r]) / np.float32(1000)) * np.float32(255))
    # the garbage bits above bit 20 never reach a point
    clean = ouster_ref.decode(ouster.write_legacy_packets(ranges, signal, m_ids, status), H, Cc, d, o, skip=skip)
    assert np.array_equal(clean["xyz"].view(np.uint32), out["xyz"].view(np.uint32))


def _stream_with_placeholders(meta, n_packets, seed, motion):
    """Synthetic packets of one sensor with invalid columns, a bad m_id, an all-invalid packet and skipped packets."""
    sp = ouster.synthetic_packets(meta, n_packets, seed=seed, motion=motion)
    rng = np.random.default_rng(seed)
    Cc, W = meta["columns_per_packet"], meta["columns_per_frame"]
    status, m_ids = sp["status"].copy(), sp["m_ids"].copy()
    status[rng.uniform(0, 1, status.shape) < 0.03] = 0
    status[17] = 0                                                   # a whole packet of invalid columns
    m_ids[23, 5] = W + 1
    m_ids[71, 0] = 40000
    skip = np.zeros(n_packets, dtype=bool)
    skip[[30, 31, 88, n_packets - 2]] = True
    packets = ouster.write_legacy_packets(sp["ranges"], sp["signal"], m_ids, status)
    return packets, sp["packet_poses"], skip


def test_placeholder_firings_equal_dropped_columns_on_the_oracle(oracle_lib):
    """The design's equivalence: a stream fed with all-NaN firings where the reference drops a column gives the same
    events, labels, ids and published columns as the stream without them; only firings_consumed and source_firing count them."""
    from oracle.pyoracle import Oracle
    meta = ouster.load_metadata(META["left"])
    H, Cc = meta["rows"], meta["columns_per_packet"]
    d, o = ouster.make_lut(meta, offset="reference")
    cfg = capi.Config.default()
    cfg.num_columns = meta["columns_per_frame"]
    n_packets = ouster.rotation_packets(meta) * 5 // 2
    packets, pposes, skip = _stream_with_placeholders(meta, n_packets, 11, synth.Motion.translate(5.0))
    dec = ouster_ref.decode(packets, H, Cc, d, o, skip=skip, packet_poses=pposes)
    valid = dec["valid"]
    assert 100 < (~valid).sum() < 0.1 * valid.size
    full = Oracle(cfg, H)
    assert full.add_firings(dec["xyz"], dec["intensity"], dec["poses"]) == 0
    kept = Oracle(cfg, H)
    assert kept.add_firings(dec["xyz"][valid], dec["intensity"][valid], dec["poses"][valid]) == 0
    ef, ek = full.drain_events(), kept.drain_events()
    assert len(ef) == len(ek) and (ek["type"] == capi.EV_CLUSTER).sum() > 10
    for fld in ("type", "a", "b", "c", "d", "column"):
        assert np.array_equal(ef[fld], ek[fld]), fld
    sf, sk = full.state(), kept.state()
    for k in util.STATE_FIELDS:
        if k != "firings_consumed":
            assert sf[k] == sk[k], k
    assert sf["firings_consumed"] == valid.size and sk["firings_consumed"] == valid.sum()
    lo, hi = kept.published_range()
    assert full.published_range() == (lo, hi) and hi - lo > cfg.num_columns
    af, ak = full.read_published(lo, hi), kept.read_published(lo, hi)
    # source_firing counts the placeholders: map the kept stream's firing numbers to the full stream's
    kept_to_full = np.nonzero(valid)[0]
    src = ak["source_firing"]
    assert np.array_equal(af["source_firing"], np.where(src >= 0, kept_to_full[np.clip(src, 0, None)], src))
    ak["source_firing"] = af["source_firing"]
    util.compare_columns(ak, af, lo)
