"""CPU: the Velodyne VLS-128 decoder's host side (include/cc_velodyne.h) and the numpy restatement the GPU tests compare against.

* every function the header declares is exported, and the device path refuses to run without a GPU;
* the rotation tables and cc_velodyne_make_calibration (rings: a permutation, ties by laser index) against restatements;
* the packet writer against the numpy decode (distances, intensities, rows, raw 0);
* a hand-worked vector for the azimuth rule, and the slot validity for every position of one bad header;
* on the oracle: multi-column firings with all-NaN placeholders give what the stream without them gives.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import util
import velodyne_ref
from continuous_clustering_amd import capi, synth, velodyne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    load_library()
    return velodyne._lib()


def test_header_symbols_are_exported_and_no_gpu_means_no_decoder(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_velodyne.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    assert "cc_velodyne_decode" in names and "cc_velodyne_make_calibration" in names and len(names) == 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_velodyne.h but not exported by libcc_hip.so"
    import torch
    h = ctypes.c_void_p()
    rc = lib.cc_velodyne_create(ctypes.byref(h), 0, 2, 8, None)
    if torch.cuda.is_available():
        assert rc == capi.CC_OK
        lib.cc_velodyne_destroy(h)
    else:
        assert rc == capi.CC_ERR_NO_DEVICE and not h.value
        assert b"no gfx950 device" in lib.cc_velodyne_last_error()
    assert lib.cc_velodyne_create(ctypes.byref(h), 0, 0, 8, None) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_velodyne_packet_bytes() == 1206 and lib.cc_velodyne_rows() == 128 and lib.cc_velodyne_firings_per_packet() == 3


def test_rotation_tables_within_one_ulp_of_double(lib):
    ct, st = velodyne.rotation_tables()
    assert ct.shape == (36000,) and st.dtype == np.float32
    i = np.arange(36000)
    rad = ((np.float32(0.01) * i.astype(np.float32)).astype(np.float64) * math.pi / 180.0).astype(np.float32)   # the table's own angle
    want_c = np.array([math.cos(float(r)) for r in rad])
    want_s = np.array([math.sin(float(r)) for r in rad])
    for got, want in ((ct, want_c), (st, want_s)):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= ulp).all(), np.abs((got - want) / ulp).max()
    assert ct[0] == 1.0 and st[0] == 0.0 and abs(st[9000] - 1.0) < 1e-7 and abs(ct[18000] + 1.0) < 1e-7


def test_make_calibration_rings_are_a_stable_rank(lib):
    rng = np.random.default_rng(5)
    vert = np.deg2rad(rng.uniform(-25, 15, 128))
    vert[[7, 90, 33]] = vert[50]                                   # four equal angles: ranked by laser index
    vert[100] = np.nextafter(vert[101], 1.0)                       # differs in double, equal as the driver's float: a tie too
    assert np.float32(vert[100]) == np.float32(vert[101]) and vert[100] != vert[101]
    rot = np.deg2rad(rng.uniform(-7, 7, 128))
    cal = velodyne.make_calibration(rot, vert)
    ring = cal["laser_ring"]
    assert sorted(ring.tolist()) == list(range(128))
    order = np.argsort(vert.astype(np.float32), kind="stable")     # the laser at each ring
    want = np.empty(128, dtype=np.int32)
    want[order] = np.arange(128)
    assert np.array_equal(ring, want)
    assert ring[7] < ring[33] < ring[50] < ring[90] and ring[90] - ring[7] == 3 and ring[101] == ring[100] + 1
    for k, ang, fn in (("cos_rot_correction", rot, math.cos), ("sin_rot_correction", rot, math.sin),
                       ("cos_vert_correction", vert, math.cos), ("sin_vert_correction", vert, math.sin)):
        want = np.array([fn(float(np.float32(x))) for x in ang])
        assert cal[k].dtype == np.float32
        assert (np.abs(cal[k].astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all(), k
    syn = velodyne.synthetic_calibration(3)
    assert sorted(syn["laser_ring"].tolist()) == list(range(128)) and not np.array_equal(syn["laser_ring"], np.arange(128))
    assert np.allclose(np.sort(np.rad2deg(syn["vert_correction"])), np.linspace(-25, 15, 128))
    assert set(np.round(np.abs(np.rad2deg(syn["rot_correction"])), 3)) == {6.354, 4.548, 2.732, 0.911}


def test_load_calibration_reads_the_driver_yaml(lib, tmp_path):
    try:
        import yaml
    except ImportError:                                            # no PyYAML: a clear error, not a silent default
        with pytest.raises(ImportError, match="PyYAML"):
            velodyne.load_calibration(str(tmp_path / "missing.yaml"))
        return
    syn = velodyne.synthetic_calibration(2)
    doc = dict(num_lasers=128, distance_resolution=0.004,
               lasers=[dict(laser_id=i, rot_correction=float(syn["rot_correction"][i]), vert_correction=float(syn["vert_correction"][i]),
                            dist_correction=0.0, vert_offset_correction=0.0) for i in reversed(range(128))])
    path = tmp_path / "vls128_made_up.yaml"
    path.write_text(yaml.safe_dump(doc))
    cal = velodyne.load_calibration(str(path))
    for k in velodyne.CAL_ARRAYS:
        assert np.array_equal(cal[k], syn[k]), k
    doc["lasers"] = doc["lasers"][:64]
    path.write_text(yaml.safe_dump(doc))
    with pytest.raises(ValueError):
        velodyne.load_calibration(str(path))


def test_non_permutation_ring_is_refused(lib):
    cal = velodyne.synthetic_calibration(0)
    arr = [np.ascontiguousarray(cal[k]) for k in velodyne.CAL_ARRAYS]
    for bad in (lambda r: r.__setitem__(5, r[6]), lambda r: r.__setitem__(0, 128), lambda r: r.__setitem__(127, -1)):
        ring = arr[4].copy()
        bad(ring)
        rc = lib.cc_velodyne_set_calibration(None, 0, *[a.ctypes.data for a in arr[:4]], ring.ctypes.data)
        assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"not a permutation" in lib.cc_velodyne_last_error()
    # a good ring gets as far as the missing handle
    rc = lib.cc_velodyne_set_calibration(None, 0, *[a.ctypes.data for a in arr])
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"null handle" in lib.cc_velodyne_last_error()


def test_azimuth_rule_hand_worked():
    """frac[order] = 0.05 * (order + order / 8): bank 0 has 0, .05, .10, .15; bank 3 has .65, .70, .75, .80 (records 0-7, 8-15, ...)."""
    rot = np.array([100, 120, 140, 35990,      # block 3 -> 4 wraps: diff 20, a_f 36003 .. 36006 -> 3 .. 6
                    10, 30, 40000, 40020,      # block 6: a rotation word >= 36000, diff 20: 40000 + 20 frac -> 4000 + ..
                    65000, 64000, 65535, 100])  # block 8: diff 35000; block 10 -> 11: 36000 + 100 - 65535 < 0; block 11: diff 0
    diff = velodyne_ref.block_azimuth_diff(rot)
    assert diff.dtype == np.float32
    assert diff.tolist() == [20, 20, 35850, 20, 20, 3970, 20, (36000 + 65000 - 40020) % 36000, 35000, 1535, -29435, 0]
    a = velodyne_ref.corrected_azimuth(rot)
    assert a.shape == (12, 32)
    assert a[0, [0, 8, 16, 24]].tolist() == [100, 101, 102, 103]                    # bank 0, orders 0..3
    assert a[3, [0, 8, 16, 24]].tolist() == [3, 4, 5, 6]                            # bank 3 of slot 0: 35990 + 13, 14, 15, 16 wraps
    assert a[3, 7] == 3 and a[3, 31] == 6
    assert a[6, [0, 8, 16, 24]].tolist() == [4009, 4010, 4011, 4012]                # bank 2 (orders 8..11: .45 .50 .55 .60) of 40000
    # block 8 is bank 0 of slot 2; 65000 + 35000 * 0.15 = 70250 > 65535: the low 16 bits, 4714
    assert a[8, [0, 8, 16, 24]].tolist() == [65000 % 36000, (65000 + 1750) & 0xFFFF, (65000 + 3500) & 0xFFFF, (65000 + 5250) & 0xFFFF]
    assert a[8, 24] == 4714
    # block 10 is bank 2: 65535 - 29435 * (.45, .50, .55, .60) = 52289.25, 50817.5 (half: away from zero), 49345.75, 47874
    assert a[10, [0, 8, 16, 24]].tolist() == [52289 - 36000, 50818 - 36000, 49346 - 36000, 47874 - 36000]
    assert (a[11] == 100).all()                                                     # diff[11] = 0
    # the writer's own helper (used to aim the synthetic rays) agrees, on these and on random words
    rng = np.random.default_rng(1)
    many = np.concatenate([rot[None], rng.integers(0, 65536, (500, 12)), rng.integers(0, 36000, (500, 12))])
    assert np.array_equal(velodyne.corrected_azimuth(many).reshape(-1, 12, 32), velodyne_ref.corrected_azimuth(many))


def _small_packets(seed=3, P=6):
    rng = np.random.default_rng(seed)
    raw = rng.integers(1, 65536, (P, 12, 32)).astype(np.uint16)
    inten = rng.integers(0, 256, (P, 12, 32)).astype(np.uint8)
    rot = ((np.arange(P * 12) * 5 + 35900) % 36000).reshape(P, 12).astype(np.uint16)
    return raw, inten, rot


def test_packet_writer_and_numpy_decode_round_trip(lib):
    raw, inten, rot = _small_packets()
    raw[0, 0, :4] = 0                                                               # no return
    raw[1, 5, 9] = 65535
    cal = velodyne.synthetic_calibration(1)
    ct, st = velodyne.rotation_tables()
    pk = velodyne.write_packets(raw, inten, rot)
    assert pk.shape == (6, 1206) and pk.dtype == np.uint8
    # raw field positions
    assert pk[2, 0:2].tolist() == [0xFF, 0xEE] and pk[2, 300:302].tolist() == [0xFF, 0xBB] and pk[2, 1204] == 55 and pk[2, 1205] == 0xA1
    assert int.from_bytes(pk[1, 502:504].tobytes(), "little") == rot[1, 5]
    assert int.from_bytes(pk[1, 500 + 4 + 27:500 + 4 + 29].tobytes(), "little") == 65535 and pk[1, 500 + 4 + 29] == inten[1, 5, 9]
    wide = velodyne.write_packets(raw.reshape(6, 3, 128), inten.reshape(6, 3, 128), rot, stride=1216)     # (slot, laser) is the same memory
    assert wide.shape == (6, 1216) and np.array_equal(wide[:, :1206], pk) and not wide[:, 1206:].any()
    f = velodyne_ref.fields(pk)
    assert np.array_equal(f["raw"], raw) and np.array_equal(f["intensity"], inten) and np.array_equal(f["rotation"], rot)
    skip = np.zeros(6, dtype=bool)
    skip[4] = True
    poses = np.arange(6 * 12, dtype=np.float64).reshape(6, 12)
    out = velodyne_ref.decode(pk, ct, st, cal, skip=skip, packet_poses=poses)
    assert out["xyz"].shape == (18, 128, 3) and out["valid"].sum() == 15 and not out["valid"][12:15].any()
    assert int(out["skipped_packets"]) == 1 and int(out["bad_block_header"]) == 0 and int(out["dual_return_packets"]) == 0
    assert np.array_equal(out["poses"][3:6], np.repeat(poses[1:2], 3, 0))
    assert out["block_azimuth"].tolist() == [int(rot[p, 4 * k]) if p != 4 else -1 for p in range(6) for k in range(3)]
    # rows: laser L of slot k lands in row 127 - ring[L]; the distance survives as |xyz| = raw * 0.004, the intensity as the byte
    row = 127 - cal["laser_ring"]
    dist = np.linalg.norm(out["xyz"].astype(np.float64), axis=-1).reshape(6, 3, 128)
    want = raw.reshape(6, 3, 128).astype(np.float64) * 0.004
    live = ~skip
    assert np.allclose(dist[live][:, :, row][want[live] > 0], want[live][want[live] > 0], rtol=1e-6)
    assert np.array_equal(out["intensity"].reshape(6, 3, 128)[live][:, :, row], np.where(raw > 0, inten, 0).reshape(6, 3, 128)[live])
    assert np.isnan(out["xyz"].reshape(6, 3, 128, 3)[0, 0, row[:4]]).all() and (out["intensity"].reshape(6, 3, 128)[0, 0, row[:4]] == 0).all()
    assert np.isnan(out["xyz"][12:15]).all() and not out["intensity"][12:15].any()
    # the top ring looks up, the bottom ring down, and the azimuth of a point is the table angle minus the laser's offset (clockwise)
    z = out["xyz"].reshape(6, 3, 128, 3)[1, 1, :, 2]
    assert z[0] > 0 > z[127]
    L = 40
    a = velodyne_ref.corrected_azimuth(rot)[1, 4 + L // 32, L % 32]
    x, y, _ = out["xyz"].reshape(6, 3, 128, 3)[1, 1, row[L]]
    want_az = -(math.radians(a * 0.01) - cal["rot_correction"][L])
    assert abs((math.atan2(y, x) - want_az + math.pi) % (2 * math.pi) - math.pi) < 1e-4


def test_slot_validity_for_every_bad_header_position(lib):
    raw, inten, rot = _small_packets(P=1)
    cal = velodyne.synthetic_calibration(1)
    ct, st = velodyne.rotation_tables()
    good = np.tile(np.array(velodyne.BANK_HEADERS, dtype=np.uint16), 3)
    clean = velodyne_ref.decode(velodyne.write_packets(raw, inten, rot), ct, st, cal)
    assert clean["valid"].tolist() == [True, True, True]
    for b in range(12):
        for word in (0xFFEE, 0x0000, good[(b + 1) % 4]):                          # garbage, zero, another bank's header
            hdr = good.copy()
            hdr[b] = word
            out = velodyne_ref.decode(velodyne.write_packets(raw, inten, rot, headers=hdr[None]), ct, st, cal)
            assert out["valid"].tolist() == [k < b // 4 for k in range(3)], (b, word)
            assert int(out["bad_block_header"]) == 3 - b // 4
            for k in range(3):                                                      # the slots in front are untouched, the rest all NaN
                if k < b // 4:
                    assert np.array_equal(out["xyz"][k].view(np.uint32), clean["xyz"][k].view(np.uint32))
                else:
                    assert np.isnan(out["xyz"][k]).all() and not out["intensity"][k].any() and out["block_azimuth"][k] == -1
    for k in range(3):                                                              # mis-ordered banks inside one slot
        hdr = good.copy()
        hdr[4 * k + 1], hdr[4 * k + 2] = hdr[4 * k + 2], hdr[4 * k + 1]
        out = velodyne_ref.decode(velodyne.write_packets(raw, inten, rot, headers=hdr[None]), ct, st, cal)
        assert out["valid"].tolist() == [j < k for j in range(3)]
    dual = velodyne_ref.decode(velodyne.write_packets(raw, inten, rot, return_mode=57), ct, st, cal)
    assert not dual["valid"].any() and int(dual["dual_return_packets"]) == 1 and int(dual["bad_block_header"]) == 0
    last = velodyne_ref.decode(velodyne.write_packets(raw, inten, rot, return_mode=56), ct, st, cal)
    assert last["valid"].all()


def test_placeholder_firings_equal_dropped_firings_on_the_oracle(oracle_lib):
    """with multi-column firings too, a stream fed all-NaN firings where the reference drops a firing gives the events,
    labels, ids and published columns of the stream without them; only firings_consumed and source_firing count them."""
    from oracle.pyoracle import Oracle
    cal = velodyne.synthetic_calibration(0)
    ct, st = velodyne.rotation_tables()
    cfg = capi.Config.vls128()
    n_packets = velodyne.rotation_packets() * 2
    sp = velodyne.synthetic_packets(cal, n_packets, seed=11, motion=synth.Motion.translate(5.0))
    hdr = np.tile(np.array(velodyne.BANK_HEADERS, dtype=np.uint16), (n_packets, 3))
    rng = np.random.default_rng(11)
    hit = rng.uniform(0, 1, n_packets) < 0.03
    hdr[hit, rng.integers(0, 12, hit.sum())] = 0
    mode = np.full(n_packets, 55)
    mode[[40, 41, 700]] = 57
    skip = np.zeros(n_packets, dtype=bool)
    skip[[30, 31, 88, n_packets - 2]] = True
    pk = velodyne.write_packets(sp["raw_distance"], sp["intensity"], sp["rotation"], headers=hdr, return_mode=mode)
    dec = velodyne_ref.decode(pk, ct, st, cal, skip=skip, packet_poses=sp["packet_poses"])
    valid = dec["valid"]
    assert 50 < (~valid).sum() < 0.1 * valid.size
    full = Oracle(cfg, 128)
    assert full.add_firings(dec["xyz"], dec["intensity"], dec["poses"]) == 0
    kept = Oracle(cfg, 128)
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
    assert full.published_range() == (lo, hi) and hi - lo > cfg.num_columns // 2
    af, ak = full.read_published(lo, hi), kept.read_published(lo, hi)
    kept_to_full = np.nonzero(valid)[0]
    src = ak["source_firing"]
    assert np.array_equal(af["source_firing"], np.where(src >= 0, kept_to_full[np.clip(src, 0, None)], src))
    ak["source_firing"] = af["source_firing"]
    util.compare_columns(ak, af, lo)
