"""GPU: the Ouster packet decoder (include/cc_ouster.h) — bit-equal to the numpy decode, and chained with an engine on its HIP stream it
gives, per stream, what the oracle gives for the valid firings alone."""
import math
import os

import numpy as np
import pytest

import ouster_ref
import util
from continuous_clustering_amd import capi, ouster, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = {side: os.path.join(GOLDEN, f"ouster_os32_{side}_metadata.json") for side in ("left", "right")}


def _tilted_mount():
    """robot_from_sensor of a corner mount like the Touareg's: yaw 40 deg, pitch 8 deg, roll -5 deg, 1.1 m ahead, 0.75 m left, 1.95 m up."""
    def rz(a):
        return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])

    def ry(a):
        return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])

    def rx(a):
        return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])

    R = rz(math.radians(40)) @ ry(math.radians(8)) @ rx(math.radians(-5))
    return np.concatenate([R, np.array([[1.1], [0.75], [1.95]])], 1).reshape(12)


def _packets(meta, n_packets, seed, motion=None, first_packet=0, damage=True):
    """Synthetic packets with garbage in the 12 unused range bits and, with `damage`, invalid columns and a bad m_id."""
    sp = ouster.synthetic_packets(meta, n_packets, seed=seed, motion=motion or synth.Motion.translate(5.0), first_packet=first_packet)
    rng = np.random.default_rng(seed + 1)
    status, m_ids = sp["status"].copy(), sp["m_ids"].copy()
    if damage:
        status[rng.uniform(0, 1, status.shape) < 0.03] = rng.choice([0, 0xFFFFFFFE])
        m_ids[rng.uniform(0, 1, m_ids.shape) < 0.01] = meta["columns_per_frame"] + 7
    garbage = rng.integers(0, 1 << 12, sp["ranges"].shape, dtype=np.uint32) << np.uint32(20)
    pk = ouster.write_legacy_packets(sp["ranges"] | garbage, sp["signal"], m_ids, status, reflectivity=rng.integers(0, 65536, sp["ranges"].shape),
                                     near_ir=rng.integers(0, 65536, sp["ranges"].shape))
    return pk, sp["packet_poses"]


def test_decoder_bit_equal_to_numpy_decode():
    import torch
    left, right = ouster.load_metadata(META["left"]), ouster.load_metadata(META["right"])
    luts = [ouster.make_lut(left, "reference"), ouster.make_lut(right, "reference"), ouster.make_lut(left, "sdk")]
    S, P, H, Cc = 3, 24, 32, 16
    pk, pp = zip(*[_packets(left if s != 1 else right, P, 50 + s) for s in range(S)])
    packets, pposes = np.stack(pk), np.stack(pp)
    skip = np.zeros((S, P), dtype=bool)
    skip[0, 3] = skip[2, [0, 23]] = True
    dec = ouster.OusterDecoder(S, H, Cc, max_packets=P)
    for s, (d, o) in enumerate(luts):
        dec.set_lut(d, o, stream=s)
    dev = torch.device("cuda")
    d_pk, d_pp, d_skip = torch.from_numpy(packets).to(dev), torch.from_numpy(pposes).to(dev), torch.from_numpy(skip).to(dev)
    torch.cuda.synchronize()
    out = dec.decode(d_pk, d_pp, d_skip)
    dec.sync()
    for s, (d, o) in enumerate(luts):
        ref = ouster_ref.decode(packets[s], H, Cc, d, o, skip=skip[s], packet_poses=pposes[s])
        assert (~ref["valid"]).sum() > 10 and (ref["valid"] & np.isnan(ref["xyz"][..., 0]).any(-1)).any()  # placeholders and range 0
        assert np.array_equal(out["xyz"][s].cpu().numpy().view(np.uint32), ref["xyz"].view(np.uint32)), s
        assert np.array_equal(out["intensity"][s].cpu().numpy(), ref["intensity"]), s
        assert np.array_equal(out["poses"][s].cpu().numpy().view(np.uint64), ref["poses"].view(np.uint64)), s
        assert np.array_equal(out["measurement_id"][s].cpu().numpy(), ref["measurement_id"]), s
        c = dec.counters(s)
        assert c == dict(invalid_columns=int(ref["invalid_columns"]), bad_measurement_id=int(ref["bad_measurement_id"]),
                         skipped_packets=int(ref["skipped_packets"])), (s, c)
    # without packet poses the caller's poses stay; counters accumulate over calls
    out["poses"].fill_(7.0)
    torch.cuda.synchronize()
    dec.decode(d_pk, None, None, out=out)
    dec.sync()
    assert bool((out["poses"] == 7.0).all())
    assert dec.counters(1)["invalid_columns"] == 2 * int(ouster_ref.decode(packets[1], H, Cc, *luts[1])["invalid_columns"])


def test_intensity_of_every_signal_value():
    import torch
    H, Cc = 32, 16
    P = 65536 // (H * Cc)
    signal = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(P, Cc, H)
    ranges = np.full((P, Cc, H), 1234, dtype=np.uint32)
    m_ids = (np.arange(P * Cc) % 1024).reshape(P, Cc).astype(np.uint16)
    packets = ouster.write_legacy_packets(ranges, signal, m_ids)
    meta = ouster.load_metadata(META["left"])
    dec = ouster.OusterDecoder(1, H, Cc, max_packets=P)
    dec.set_lut(*ouster.make_lut(meta, "reference"))
    d_pk = torch.from_numpy(packets[None]).cuda()
    torch.cuda.synchronize()
    out = dec.decode(d_pk)
    dec.sync()
    want = (np.minimum(np.float32(1), np.arange(65536, dtype=np.float32) / np.float32(1000)) * np.float32(255)).astype(np.uint8)
    got = out["intensity"][0].cpu().numpy().reshape(-1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} signal values differ, first {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"
    assert want[999] == 254 and want[1000] == 255 and want[65535] == 255


@pytest.mark.parametrize("packets_per_call,tilted", [(1, False), (3, False), (64, False), (3, True)])
def test_packets_to_engine_equal_oracle_on_valid_firings(oracle_lib, packets_per_call, tilted):
    """packets -> cc_ouster_decode on cc_engine_hip_stream(e) ("input_on_engine_stream") -> cc_engine_add_firings_device over more than
    two rotations of three streams equals, per stream, the oracle fed only the valid numpy-decoded firings."""
    import torch
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    left, right = ouster.load_metadata(META["left"]), ouster.load_metadata(META["right"])
    metas = [left, right, left]
    S, H, Cc = 3, 32, 16
    n_packets = 2 * ouster.rotation_packets(left) + 40
    luts = [ouster.make_lut(m, "reference") for m in metas]
    motions = [synth.Motion.translate(5.0), synth.Motion.turn(6.0, 0.3), synth.Motion.static()]
    pk, pp = zip(*[_packets(metas[s], n_packets, 300 + s, motions[s], first_packet=7 * s) for s in range(S)])
    packets, pposes = np.stack(pk), np.stack(pp)
    skip = np.zeros((S, n_packets), dtype=bool)
    skip[0, [5, 70]] = skip[1, 100] = True
    robot_tf = _tilted_mount() if tilted else np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
    cfg = capi.Config.default()
    cfg.num_columns = left["columns_per_frame"]

    e = Engine(cfg, H, S, robot_from_sensor=robot_tf)
    e.record_events(True)
    e.set_option("input_on_engine_stream", 1)
    dec = ouster.OusterDecoder(S, H, Cc, max_packets=packets_per_call, hip_stream=e.hip_stream())
    dec.check_engine(e)
    for s in range(S):
        dec.set_lut(*luts[s], stream=s)

    oracles, evo, kept_to_full = [], [], []
    for s in range(S):
        ref = ouster_ref.decode(packets[s], H, Cc, *luts[s], skip=skip[s], packet_poses=pposes[s])
        v = ref["valid"]
        o = Oracle(cfg, H, robot_tf)
        assert o.add_firings(ref["xyz"][v], ref["intensity"][v], ref["poses"][v]) == 0
        oracles.append(o)
        evo.append(o.drain_events())
        kept_to_full.append(np.nonzero(v)[0])
        assert (~v).sum() > 16
    dev = torch.device("cuda")
    calls = []
    for p0 in range(0, n_packets, packets_per_call):
        m = min(packets_per_call, n_packets - p0)
        calls.append((m, torch.from_numpy(np.ascontiguousarray(packets[:, p0:p0 + m])).to(dev),
                      torch.from_numpy(np.ascontiguousarray(pposes[:, p0:p0 + m])).to(dev),
                      torch.from_numpy(np.ascontiguousarray(skip[:, p0:p0 + m]).astype(np.uint8)).to(dev)))
    torch.cuda.synchronize()
    pos = [0] * S
    for m, d_pk, d_pp, d_skip in calls:
        out = dec.decode(d_pk, d_pp, d_skip)
        e.add_firings_device(m * Cc, out["xyz"], out["intensity"], out["poses"])
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
        assert pos[s] == len(evo[s]) and (evo[s]["type"] == capi.EV_CLUSTER).sum() > 5
        so, se = oracles[s].state(), e.state(s)
        for k in util.STATE_FIELDS:
            if k != "firings_consumed":
                assert so[k] == se[k], (s, k)
        assert se["firings_consumed"] == n_packets * Cc and so["firings_consumed"] == len(kept_to_full[s])
    c = dec.counters(0)
    assert c["skipped_packets"] == 2 and c["invalid_columns"] > 0
    dec.close()                                                                      # before the engine whose HIP stream it uses
    e.close()


def test_bad_arguments_are_refused_not_run():
    import torch
    from continuous_clustering_amd import Engine, EngineError
    H, Cc, P = 32, 16, 4
    meta = ouster.load_metadata(META["left"])
    d, o = ouster.make_lut(meta, "reference")
    cfg = capi.Config.default()
    cfg.num_columns = 1024
    e64 = Engine(cfg, 64, 2)
    dec = ouster.OusterDecoder(2, H, Cc, max_packets=P, hip_stream=e64.hip_stream())
    with pytest.raises(EngineError) as ei:                                           # H != the engine's rows
        dec.check_engine(e64)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "rows" in str(ei.value)
    e3 = Engine(cfg, H, 3)
    with pytest.raises(EngineError) as ei:                                           # stream count differs
        dec.check_engine(e3)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT
    dev = torch.device("cuda")
    pk = torch.zeros((2, P + 1, ouster.packet_bytes(H, Cc)), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((2, (P + 1) * Cc, H, 3), dtype=torch.float32, device=dev)
    inten = torch.zeros((2, (P + 1) * Cc, H), dtype=torch.uint8, device=dev)
    dec.set_lut(d, o, stream=0)
    rc = dec.decode_raw(1, pk, None, None, xyz, inten)                               # stream 1 has no LUT
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"no LUT" in ouster._lib().cc_ouster_last_error()
    dec.set_lut(d, o, stream=1)
    assert dec.decode_raw(P + 1, pk, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT   # more than max_packets
    assert dec.decode_raw(1, pk, None, None, xyz[:, :, :, 1:], inten) == capi.CC_ERR_INVALID_ARGUMENT  # misaligned xyz
    assert dec.decode_raw(1, None, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT     # no packets
    with pytest.raises(ValueError):
        dec.set_lut(d[:, :16], o[:, :16])                                          # LUT of another sensor
    assert ouster._lib().cc_ouster_set_lut(dec.h, 0, 0, d.ctypes.data, o.ctypes.data) == capi.CC_ERR_INVALID_ARGUMENT
    assert ouster._lib().cc_ouster_set_lut(dec.h, 2, 1024, d.ctypes.data, o.ctypes.data) == capi.CC_ERR_INVALID_ARGUMENT
    assert dec.decode_raw(1, pk, None, None, xyz, inten) == capi.CC_OK                        # and a good call still runs
    dec.sync()
    written = xyz.view(-1)[: 2 * Cc * H * 3]                                         # [2][1 * C][H][3]: the stream stride of a 1-packet call
    assert bool(torch.isnan(written).all()) and not bool(torch.isnan(xyz.view(-1)[2 * Cc * H * 3:]).any())  # status 0: all placeholders
    assert dec.counters(0)["invalid_columns"] == Cc
    dec.close()
