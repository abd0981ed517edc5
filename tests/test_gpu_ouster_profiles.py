"""GPU: the RNG19_RFL8_SIG16_NIR16 single- and dual-return UDP profiles of the Ouster packet decoder (include/cc_ouster_profiles.h) —
bit-equal to the numpy decode of tests/ouster_profiles_ref.py, the same scene decoded alike from all three wire formats, and chained
with an engine on its HIP stream. Nothing here has a tolerance: the decode is integer field extraction, one f32 multiply and one f32 add."""
import ctypes
import os

import numpy as np
import pytest

import ouster_profiles_ref as pref
import util
from continuous_clustering_amd import capi, ouster, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = {side: os.path.join(GOLDEN, f"ouster_os32_{side}_metadata.json") for side in ("left", "right")}
NEW_PROFILES = [pref.SINGLE, pref.DUAL]
RANGE_MASK = 0x0007FFFF                          # of both new profiles
OVERFLOW_WORD = 0x00080000                       # range 0 under the 19-bit mask, a hit under LEGACY's 20 bits


def _luts(H, Cc, S=3):
    """One LUT per stream: the two OS-32 calibrations of tests/golden for 32 rows, a synthetic sensor otherwise."""
    if H == 32:
        left, right = ouster.load_metadata(META["left"]), ouster.load_metadata(META["right"])
        return [ouster.make_lut(left, "reference"), ouster.make_lut(right, "reference"), ouster.make_lut(left, "sdk")][:S]
    meta = ouster.synthetic_metadata(H, 64 if H == 4 else 512, Cc)
    d, o = ouster.make_lut(meta, "sdk")
    return [(d, d.copy()), (d, o), (np.ascontiguousarray(d[::-1]), np.ascontiguousarray(o[::-1]))][:S]


def _random_packets(profile, seed, S, P, Cc, H, W):
    """Packets [S][P][bytes] of a new profile with everything the decode must not look at filled with random bits, and the pieces
    (`parts`) they were written from."""
    rng = np.random.default_rng(seed)
    shape = (S, P, Cc, H)
    n = int(np.prod(shape))
    ranges = rng.integers(0, RANGE_MASK + 1, shape, dtype=np.uint32)
    special = np.array([0, 1, RANGE_MASK, OVERFLOW_WORD], dtype=np.uint32)
    reps = max(2, n // 50)
    where = rng.permutation(n)[:4 * reps]
    ranges.reshape(-1)[where] = np.tile(special, reps)
    # random bits wherever the range mask removes them: bits 19-31 of the single profile's word, bits 19-23 of the dual profile's
    # (its byte 3 is the reflectivity, random below); the 0x00080000 words stay exactly that
    garbage = rng.integers(0, 1 << (13 if profile == pref.SINGLE else 5), shape, dtype=np.uint32) << np.uint32(19)
    reflectivity = rng.integers(0, 256, shape, dtype=np.uint8)
    overflow = ranges == OVERFLOW_WORD
    garbage[overflow] = 0
    reflectivity[overflow] = 0
    status = rng.choice(np.array([0, 1, 0xFFFE, 0xFFFF], dtype=np.uint32), (S, P, Cc), p=[0.08, 0.4, 0.07, 0.45])
    status.reshape(-1)[:4] = [0xFFFF, 0, 0xFFFE, 1]
    m_ids = rng.integers(0, W, (S, P, Cc)).astype(np.uint16)
    bad = rng.permutation(S * P * Cc)[:max(3, S * P * Cc // 40)]
    m_ids.reshape(-1)[bad] = np.resize(np.array([W, 65535, W + 7], dtype=np.uint16), bad.size)
    signal = rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    signal.reshape(-1)[where[:4]] = [0, 999, 1000, 65535]
    kw = dict(near_ir=rng.integers(0, 1 << 16, shape, dtype=np.uint16), reflectivity=reflectivity,
              header=rng.integers(0, 256, (S, P, 32), dtype=np.uint8), footer=rng.integers(0, 256, (S, P, 32), dtype=np.uint8),
              timestamps=rng.integers(0, 1 << 62, (S, P, Cc), dtype=np.uint64))
    if profile == pref.DUAL:
        kw.update(range2=rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32), signal2=rng.integers(0, 1 << 16, shape, dtype=np.uint16),
                  reflectivity2=rng.integers(0, 256, shape, dtype=np.uint8))
    packets = ouster.write_packets(profile, ranges | garbage, signal, m_ids, status, **kw)
    poses = rng.uniform(-50, 50, (S, P, 12))
    return packets, poses, dict(ranges=ranges, signal=signal, m_ids=m_ids, status=status, overflow=overflow)


def _decode_on_gpu(profile, packets, pposes, skip, luts, H, Cc, misalign=0):
    import torch
    S, P, nbytes = packets.shape
    dec = ouster.OusterDecoder(S, H, Cc, max_packets=P, profile=profile)
    assert dec.packet_bytes == nbytes and dec.profile_name == profile
    for s, (d, o) in enumerate(luts):
        dec.set_lut(d, o, stream=s)
    dev = torch.device("cuda")
    if misalign:
        buf = torch.zeros(packets.size + 16, dtype=torch.uint8, device=dev)
        d_pk = buf[misalign:misalign + packets.size].view(S, P, nbytes)
        d_pk.copy_(torch.from_numpy(packets))
        assert d_pk.data_ptr() % 16 == misalign and d_pk.is_contiguous()
    else:
        d_pk = torch.from_numpy(packets).to(dev)
        assert d_pk.data_ptr() % 16 == 0
    d_pp = torch.from_numpy(pposes).to(dev)
    d_skip = None if skip is None else torch.from_numpy(skip).to(dev)
    torch.cuda.synchronize()
    out = dec.decode(d_pk, d_pp, d_skip)
    dec.sync()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    counters = dec.counters()
    dec.close()
    return got, counters


def _assert_bit_equal(got, counters, ref, s):
    assert np.array_equal(got["xyz"][s].view(np.uint32), ref["xyz"].view(np.uint32)), s
    assert np.array_equal(got["intensity"][s], ref["intensity"]), s
    assert np.array_equal(got["poses"][s].view(np.uint64), ref["poses"].view(np.uint64)), s
    assert np.array_equal(got["measurement_id"][s], ref["measurement_id"]), s
    assert counters[s] == dict(invalid_columns=int(ref["invalid_columns"]), bad_measurement_id=int(ref["bad_measurement_id"]),
                               skipped_packets=int(ref["skipped_packets"])), (s, counters[s])


# (4, 1): packets of 124 / 140 B, no multiple of 16: the dword staging path. (32, 16): the OS-32 calibrations. (128, 16): the largest LDS
# footprint (33 KB for dual). misalign 4: the packet pointer is not 16-byte aligned, so a 16-byte-multiple packet is staged by dwords too.
@pytest.mark.parametrize("profile,H,Cc,misalign", [(p, H, Cc, 0) for p in NEW_PROFILES for H, Cc in ((4, 1), (32, 16), (128, 16))]
                         + [(pref.DUAL, 32, 16, 4)])
def test_decoder_bit_equal_to_numpy_decode(profile, H, Cc, misalign):
    S, P = 3, 8
    luts = _luts(H, Cc)
    W = luts[0][0].shape[0]
    packets, pposes, parts = _random_packets(profile, 1000 + H + Cc, S, P, Cc, H, W)
    assert packets.shape == (S, P, pref.packet_bytes(profile, H, Cc))
    assert (packets.shape[2] % 16 == 0) == (H != 4)
    skip = np.zeros((S, P), dtype=bool)
    skip[0, 3] = skip[2, [0, 7]] = True
    got, counters = _decode_on_gpu(profile, packets, pposes, skip, luts, H, Cc, misalign)
    seen = dict(placeholder=0, overflow_nan=0, hit=0, invalid=0, bad_mid=0)
    for s, (d, o) in enumerate(luts):
        ref = pref.decode(profile, packets[s], H, Cc, d, o, skip=skip[s], packet_poses=pposes[s])
        _assert_bit_equal(got, counters, ref, s)
        v = ref["valid"]
        nan = np.isnan(ref["xyz"][..., 0])
        over = parts["overflow"][s].reshape(P * Cc, H)
        assert nan[over].all()                                                   # the word 0x00080000 is range 0: NaN
        seen["overflow_nan"] += int((over & v[:, None]).sum())
        seen["placeholder"] += int((~v).sum())
        seen["hit"] += int((~nan).sum())
        seen["invalid"] += int(ref["invalid_columns"])
        seen["bad_mid"] += int(ref["bad_measurement_id"])
    assert all(n > 0 for n in seen.values()), seen
    assert set(np.unique(parts["status"]).tolist()) == {0, 1, 0xFFFE, 0xFFFF}


def test_same_scene_from_three_wire_formats():
    """The same ranges (< 2^19), signal, m_ids and status written as LEGACY, single and dual decode to the same firings and counters:
    the new paths against the one already there."""
    S, P, H, Cc = 2, 8, 32, 16
    luts = _luts(H, Cc, S)
    W = luts[0][0].shape[0]
    _, pposes, parts = _random_packets(pref.SINGLE, 77, S, P, Cc, H, W)
    ranges = np.where(parts["overflow"], 0, parts["ranges"])                      # < 2^19 in every format
    assert ranges.max() == RANGE_MASK and (ranges == 0).any()
    skip = np.zeros((S, P), dtype=bool)
    skip[1, 2] = True
    results = {}
    for profile in [pref.LEGACY] + NEW_PROFILES:
        packets = ouster.write_packets(profile, ranges, parts["signal"], parts["m_ids"], parts["status"])
        assert packets.shape[2] == pref.packet_bytes(profile, H, Cc)
        results[profile] = _decode_on_gpu(profile, packets, pposes, skip, luts, H, Cc)
    want, want_counters = results[pref.LEGACY]
    assert (want["measurement_id"] < 0).sum() > 16 and (want["intensity"] > 0).any() and want_counters[0]["invalid_columns"] > 0
    for profile in NEW_PROFILES:
        got, counters = results[profile]
        for key in ("xyz", "intensity", "measurement_id", "poses"):
            assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), (profile, key)
        assert counters == want_counters, profile


def _scene_packets(meta, n_packets, seed, motion, first_packet):
    """Ray-cast packets of the profile `meta` names, with garbage in the masked-off range bits, invalid columns and bad m_ids."""
    profile = meta["udp_profile_lidar"]
    sp = ouster.synthetic_packets(meta, n_packets, seed=seed, motion=motion, first_packet=first_packet)
    rng = np.random.default_rng(seed + 1)
    status, m_ids = sp["status"].copy(), sp["m_ids"].copy()
    status[rng.uniform(0, 1, status.shape) < 0.03] = rng.choice([0, 0xFFFE])
    status[11, :] = 0                                                             # a whole packet of invalid columns
    m_ids[rng.uniform(0, 1, m_ids.shape) < 0.01] = meta["columns_per_frame"] + 7
    m_ids[20, 3] = 65535
    garbage = rng.integers(0, 1 << (13 if profile == pref.SINGLE else 5), sp["ranges"].shape, dtype=np.uint32) << np.uint32(19)
    kw = {}
    if profile == pref.DUAL:
        kw = dict(range2=rng.integers(0, 1 << 24, sp["ranges"].shape, dtype=np.uint32), signal2=rng.integers(0, 65536, sp["ranges"].shape))
    pk = ouster.write_packets(profile, sp["ranges"] | garbage, sp["signal"], m_ids, status, reflectivity=rng.integers(0, 256, sp["ranges"].shape),
                              near_ir=rng.integers(0, 65536, sp["ranges"].shape), header=rng.integers(0, 256, (n_packets, 32), dtype=np.uint8),
                              footer=rng.integers(0, 256, (n_packets, 32), dtype=np.uint8), **kw)
    return pk, sp["packet_poses"]


@pytest.mark.parametrize("profile", NEW_PROFILES)
def test_packets_to_engine_equal_oracle_on_valid_firings(oracle_lib, profile):
    """packets of a new profile -> cc_ouster_decode on cc_engine_hip_stream(e) ("input_on_engine_stream") -> cc_engine_add_firings_device,
    two streams, 2 rotations + 8 packets at 8 packets per call: per stream, the oracle fed only the valid numpy-decoded firings."""
    import torch
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    meta = ouster.synthetic_metadata(rows=32, columns_per_frame=512, udp_profile_lidar=profile)
    S, H, Cc, per_call = 2, 32, 16, 8
    n_packets = 2 * ouster.rotation_packets(meta) + 8
    lut = ouster.make_lut(meta, "reference")
    motions = [synth.Motion.translate(5.0), synth.Motion.turn(6.0, 0.3)]
    pk, pp = zip(*[_scene_packets(meta, n_packets, 500 + s, motions[s], first_packet=5 * s) for s in range(S)])
    packets, pposes = np.stack(pk), np.stack(pp)
    assert packets.shape[2] == pref.packet_bytes(profile, H, Cc)
    skip = np.zeros((S, n_packets), dtype=bool)
    skip[1, 40] = True
    cfg = capi.Config.default()
    cfg.num_columns = meta["columns_per_frame"]

    e = Engine(cfg, H, S)
    e.record_events(True)
    e.set_option("input_on_engine_stream", 1)
    dec = ouster.OusterDecoder(S, H, Cc, max_packets=per_call, hip_stream=e.hip_stream(), profile=profile)
    dec.check_engine(e)
    dec.set_lut(*lut)

    oracles, evo, kept_to_full = [], [], []
    for s in range(S):
        ref = pref.decode(profile, packets[s], H, Cc, *lut, skip=skip[s], packet_poses=pposes[s])
        v = ref["valid"]
        o = Oracle(cfg, H)
        assert o.add_firings(ref["xyz"][v], ref["intensity"][v], ref["poses"][v]) == 0
        oracles.append(o)
        evo.append(o.drain_events())
        kept_to_full.append(np.nonzero(v)[0])
        assert (~v).sum() >= 16 and (evo[s]["type"] == capi.EV_CLUSTER).sum() >= 1   # the case cannot pass empty
    dev = torch.device("cuda")
    calls = []
    for p0 in range(0, n_packets, per_call):
        calls.append((torch.from_numpy(np.ascontiguousarray(packets[:, p0:p0 + per_call])).to(dev),
                      torch.from_numpy(np.ascontiguousarray(pposes[:, p0:p0 + per_call])).to(dev),
                      torch.from_numpy(np.ascontiguousarray(skip[:, p0:p0 + per_call]).astype(np.uint8)).to(dev)))
    torch.cuda.synchronize()
    pos = [0] * S
    for d_pk, d_pp, d_skip in calls:
        out = dec.decode(d_pk, d_pp, d_skip)
        e.add_firings_device(per_call * Cc, out["xyz"], out["intensity"], out["poses"])
        assert e.sync() == 0, e.last_error()
        for s in range(S):
            ev = e.drain_events(s)
            ref = evo[s][pos[s]:pos[s] + len(ev)]
            assert len(ev) == len(ref), (s, pos[s], len(ev), len(evo[s]))
            for fld in ("type", "a", "b", "c", "d", "column"):
                assert np.array_equal(ev[fld], ref[fld]), (s, fld)
            pos[s] += len(ev)
            pub = ev[(ev["type"] == capi.EV_PUBLISH_COLUMNS) & (ev["b"] >= ev["a"])]
            if len(pub):
                lo, hi = int(pub["a"].min()), int(pub["b"].max())
                ao, ae = oracles[s].read_published(lo, hi), e.read_columns(lo, hi, stream=s)
                src = ao["source_firing"]
                ao["source_firing"] = np.where(src >= 0, kept_to_full[s][np.clip(src, 0, None)], src)  # placeholders are counted
                util.compare_columns(ao, ae, lo)
    for s in range(S):
        assert pos[s] == len(evo[s])
        so, se = oracles[s].state(), e.state(s)
        for k in util.STATE_FIELDS:
            if k != "firings_consumed":
                assert so[k] == se[k], (s, k)
        assert se["firings_consumed"] == n_packets * Cc and so["firings_consumed"] == len(kept_to_full[s])
    c = dec.counters()
    assert c[1]["skipped_packets"] == 1 and c[0]["skipped_packets"] == 0 and c[0]["invalid_columns"] >= 16 and c[0]["bad_measurement_id"] > 0
    dec.close()                                                                      # before the engine whose HIP stream it uses
    e.close()


def test_refusals_and_profile_of():
    import torch
    L = ouster._lib()
    H, Cc, P = 32, 16, 4
    d, o = _luts(H, Cc, 1)[0]
    dev = torch.device("cuda")
    dec = ouster.OusterDecoder(2, H, Cc, max_packets=P, profile=pref.DUAL)
    dec.set_lut(d, o)
    assert L.cc_ouster_profile_of(dec.h) == 2 and dec.profile == 2
    legacy_sized = torch.zeros((2, P, ouster.packet_bytes(H, Cc)), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="8448"):                                    # LEGACY-sized packets on a dual decoder
        dec.decode(legacy_sized)
    pk = torch.zeros((2, P + 1, dec.packet_bytes), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((2, (P + 1) * Cc, H, 3), dtype=torch.float32, device=dev)
    inten = torch.zeros((2, (P + 1) * Cc, H), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert dec.decode_raw(P + 1, pk, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT    # beyond max_packets
    assert b"max_packets" in L.cc_ouster_last_error()
    assert dec.decode_raw(P, pk, None, None, xyz, inten) == capi.CC_OK               # and a good call still runs: status 0 everywhere
    dec.sync()
    assert dec.counters(0)["invalid_columns"] == P * Cc
    dec.close()
    for p, name in enumerate(ouster.PROFILE_NAMES):
        h = ctypes.c_void_p()
        assert L.cc_ouster_create_profile(ctypes.byref(h), 0, 1, H, Cc, P, p, None) == capi.CC_OK
        assert L.cc_ouster_profile_of(h) == p
        L.cc_ouster_destroy(h)
        dd = ouster.OusterDecoder(1, H, Cc, max_packets=P, profile=name)
        assert L.cc_ouster_profile_of(dd.h) == p
        dd.close()
    h = ctypes.c_void_p()
    assert L.cc_ouster_create(ctypes.byref(h), 0, 1, H, Cc, P, None) == capi.CC_OK
    assert L.cc_ouster_profile_of(h) == 0                                            # a handle of cc_ouster_create is LEGACY
    L.cc_ouster_destroy(h)
    assert L.cc_ouster_create_profile(ctypes.byref(h), 0, 1, 128, 64, P, 2, None) == capi.CC_ERR_INVALID_ARGUMENT and not h.value

