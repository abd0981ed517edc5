"""GPU: the Velodyne VLS-128 packet decoder (include/cc_velodyne.h) — bit-equal to the numpy restatement of its specification
(tests/velodyne_ref.py) on damaged packets at every staging path, on every block azimuth, and refusing what it cannot run."""
import numpy as np
import pytest

import velodyne_ref
from continuous_clustering_amd import capi, synth, velodyne

pytestmark = pytest.mark.gpu

GOOD = np.tile(np.array(velodyne.BANK_HEADERS, dtype=np.uint16), 3)


def _damaged_stream(cal, P, seed):
    """Synthetic packets of one sensor with every kind of damage the decoder tells apart; returns the writer's arguments."""
    sp = velodyne.synthetic_packets(cal, P, seed=seed, motion=synth.Motion.translate(5.0), first_packet=615 + seed)
    raw, inten, rot = sp["raw_distance"].copy(), sp["intensity"].copy(), sp["rotation"].copy()
    hdr = np.tile(GOOD, (P, 1))
    hdr[2, 0] = 0xFFEE                                      # bad header at block 0: the whole packet
    hdr[4, 5] = 0                                           # at block 5: slots 1 and 2
    hdr[6, 11] = 0xEEFF                                     # at block 11: slot 2
    hdr[8, 5], hdr[8, 6] = hdr[8, 6], hdr[8, 5]             # mis-ordered banks in slot 1
    mode = np.full(P, 55)
    mode[10] = 57                                           # dual return: refused
    mode[11] = 56                                           # last return: decoded
    raw[12, 3, :8] = 0
    raw[12, 4, 8:16] = 65535
    raw[13] = 0                                             # a packet without a single return
    rot[14] = 35960 + 7 * np.arange(12)                     # a rotation wrap inside the packet: words 35960 .. 36037
    rot[14] %= 36000
    rot[15] = 36000 + 13 * np.arange(12)                    # rotation words >= 36000
    rot[16] = [65000, 64000, 65535, 100, 65535, 65535, 0, 65535, 40000, 30, 35999, 0]   # negative %, sums above 65535
    return raw, inten, rot, hdr, mode, sp["packet_poses"]


def _garbage_padded(pk, stride, seed):
    """The packets at `stride` bytes with garbage behind byte 1206 (the decoder must not look at it)."""
    out = np.random.default_rng(seed).integers(0, 256, (*pk.shape[:-1], stride), dtype=np.uint8)
    out[..., :1206] = pk
    return out


def test_decoder_bit_equal_to_numpy_decode():
    import torch
    S, P = 3, 24
    cals = [velodyne.synthetic_calibration(1), velodyne.synthetic_calibration(1), velodyne.synthetic_calibration(2)]
    ct, st = velodyne.rotation_tables()
    args = [_damaged_stream(cals[s], P, 50 + s) for s in range(S)]
    pk = np.stack([velodyne.write_packets(a[0], a[1], a[2], headers=a[3], return_mode=a[4]) for a in args])
    pposes = np.stack([a[5] for a in args])
    skip = np.zeros((S, P), dtype=bool)
    skip[0, 3] = skip[2, [0, 23]] = True
    skip[1, 10] = True                                      # a skipped dual-return packet counts as skipped only
    dev = torch.device("cuda")
    d_pp, d_skip = torch.from_numpy(pposes).to(dev), torch.from_numpy(skip).to(dev)
    dec = velodyne.VelodyneDecoder(S, max_packets=P)
    for s in range(S):
        dec.set_calibration(cals[s], stream=s)
    refs = [velodyne_ref.decode(pk[s], ct, st, cals[s], skip=skip[s], packet_poses=pposes[s]) for s in range(S)]
    for s, ref in enumerate(refs):                          # the input really contains what the test is about
        assert (~ref["valid"]).sum() >= 9 and (ref["valid"] & np.isnan(ref["xyz"][..., 0]).any(-1)).any()
        assert ref["valid"].sum() > 40 and int(ref["bad_block_header"]) == 3 + 2 + 1 + 2
        assert int(ref["dual_return_packets"]) == (0 if s == 1 else 1)
    calls = 0
    for stride in (1206, 1208, 1216):                       # u16, dword and 16-byte staging
        d_pk = torch.from_numpy(_garbage_padded(pk, stride, stride)).to(dev)
        torch.cuda.synchronize()
        out = dec.decode(d_pk, d_pp, d_skip)
        dec.sync()
        calls += 1
        for s, ref in enumerate(refs):
            assert np.array_equal(out["xyz"][s].cpu().numpy().view(np.uint32), ref["xyz"].view(np.uint32)), (stride, s)
            assert np.array_equal(out["intensity"][s].cpu().numpy(), ref["intensity"]), (stride, s)
            assert np.array_equal(out["poses"][s].cpu().numpy().view(np.uint64), ref["poses"].view(np.uint64)), (stride, s)
            assert np.array_equal(out["block_azimuth"][s].cpu().numpy(), ref["block_azimuth"]), (stride, s)
            c = dec.counters(s)
            assert c == dict(bad_block_header=calls * int(ref["bad_block_header"]), dual_return_packets=calls * int(ref["dual_return_packets"]),
                             skipped_packets=calls * int(ref["skipped_packets"])), (stride, s, c)
    # one packet per call (a workgroup with three idle packet slots); a packet count that is no multiple of the workgroup's four
    for p0, m in ((6, 1), (1, 22)):
        d_pk = torch.from_numpy(np.ascontiguousarray(pk[:, p0:p0 + m])).to(dev)
        d_p1 = torch.from_numpy(np.ascontiguousarray(pposes[:, p0:p0 + m])).to(dev)
        torch.cuda.synchronize()
        out1 = dec.decode(d_pk, d_p1)
        dec.sync()
        for s in range(S):
            ref1 = velodyne_ref.decode(pk[s, p0:p0 + m], ct, st, cals[s], packet_poses=pposes[s, p0:p0 + m])
            assert np.array_equal(out1["xyz"][s].cpu().numpy().view(np.uint32), ref1["xyz"].view(np.uint32)), (m, s)
            assert np.array_equal(out1["intensity"][s].cpu().numpy(), ref1["intensity"]), (m, s)
            assert np.array_equal(out1["poses"][s].cpu().numpy().view(np.uint64), ref1["poses"].view(np.uint64)), (m, s)
            assert np.array_equal(out1["block_azimuth"][s].cpu().numpy(), ref1["block_azimuth"]), (m, s)
    # without packet poses the caller's poses stay
    before = dec.counters(2)
    out["poses"].fill_(7.0)
    d_pk = torch.from_numpy(pk).to(dev)
    torch.cuda.synchronize()
    dec.decode(d_pk, None, None, out=out)
    dec.sync()
    assert bool((out["poses"] == 7.0).all())
    after = dec.counters(2)
    unskipped = velodyne_ref.decode(pk[2], ct, st, cals[2])
    assert after["bad_block_header"] - before["bad_block_header"] == int(unskipped["bad_block_header"])
    assert after["skipped_packets"] == before["skipped_packets"]
    dec.close()


def test_every_block_azimuth():
    """3000 packets whose 36 000 block rotation words are 0 .. 35999, at a fixed distance: in order (streams 0-3: every diff is 1) and
    as k -> 19 k mod 36000 (streams 4-7: every diff is 19, about the sensor's own advance per block). Stream j of each four starts j
    blocks later, so every rotation word meets every bank, and with it every firing order."""
    import torch
    P, S = 3000, 8
    k = np.arange(P * 12)
    rot = np.stack([(step * (k + j)) % 36000 for step in (1, 19) for j in range(4)]).reshape(S, P, 12).astype(np.uint16)
    for r in rot:
        assert np.array_equal(np.sort(r.reshape(-1)), np.arange(36000))
    bank = np.broadcast_to(np.arange(12) % 4, (4, P, 12))
    for g in (0, 4):
        assert np.unique(rot[g:g + 4].astype(np.int64) * 4 + bank).size == 4 * 36000
    cal = velodyne.synthetic_calibration(4)
    ct, st = velodyne.rotation_tables()
    pk = velodyne.write_packets(np.full((S, P, 12, 32), 5000, dtype=np.uint16), 9, rot, stride=1216)
    dec = velodyne.VelodyneDecoder(S, max_packets=P)
    dec.set_calibration(cal)
    d_pk = torch.from_numpy(pk).cuda()
    torch.cuda.synchronize()
    out = dec.decode(d_pk)
    dec.sync()
    got_xyz, got_az = out["xyz"].cpu().numpy(), out["block_azimuth"].cpu().numpy()
    ref = velodyne_ref.decode(pk, ct, st, cal)
    assert ref["valid"].all() and not np.isnan(ref["xyz"]).any()
    bad = np.argwhere(got_xyz.view(np.uint32) != ref["xyz"].view(np.uint32))
    assert bad.size == 0, f"{len(bad)} values differ, first (stream, firing, row, axis) {bad[0]}: {got_xyz[tuple(bad[0])]} vs " \
                          f"{ref['xyz'][tuple(bad[0])]}"
    assert np.array_equal(got_az, ref["block_azimuth"])
    assert bool((out["intensity"] == 9).all())
    assert dec.counters(0) == dict(bad_block_header=0, dual_return_packets=0, skipped_packets=0)
    dec.close()


def test_bad_arguments_are_refused_not_run():
    import torch
    from continuous_clustering_amd import Engine, EngineError
    P = 4
    cal = velodyne.synthetic_calibration(0)
    cfg = capi.Config.vls128()
    e64 = Engine(cfg, 64, 2)
    dec = velodyne.VelodyneDecoder(2, max_packets=P, hip_stream=e64.hip_stream())
    with pytest.raises(EngineError) as ei:                                           # the engine's rows are not 128
        dec.check_engine(e64)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "rows" in str(ei.value)
    e3 = Engine(cfg, 128, 3)
    with pytest.raises(EngineError) as ei:                                           # stream count differs
        dec.check_engine(e3)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "streams" in str(ei.value)
    e2 = Engine(cfg, 128, 2)
    dec.check_engine(e2)
    dev = torch.device("cuda")
    err = velodyne._lib().cc_velodyne_last_error
    pk = torch.zeros((2, P + 1, 1216), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((2, (P + 1) * 3, 128, 3), dtype=torch.float32, device=dev)
    inten = torch.zeros((2, (P + 1) * 3, 128), dtype=torch.uint8, device=dev)
    dec.set_calibration(cal, stream=0)
    rc = dec.decode_raw(1, pk, 1216, None, None, xyz, inten)                         # stream 1 has no calibration
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"no calibration" in err()
    bad = dict(cal, laser_ring=np.where(cal["laser_ring"] == 5, 6, cal["laser_ring"]))
    with pytest.raises(EngineError) as ei:                                           # ring 6 twice
        dec.set_calibration(bad, stream=1)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "permutation" in str(ei.value)
    with pytest.raises(EngineError):
        dec.set_calibration(cal, stream=2)                                           # no such stream
    dec.set_calibration(cal, stream=1)
    assert dec.decode_raw(P + 1, pk, 1216, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT      # more than max_packets
    rc = dec.decode_raw(1, pk, 1216, None, None, xyz[:, :, :, 1:], inten)            # misaligned xyz
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"misaligned" in err()
    rc = dec.decode_raw(1, pk.view(-1)[1:], 1216, None, None, xyz, inten)            # packets at an odd address
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"misaligned" in err()
    rc = dec.decode_raw(1, pk, 1207, None, None, xyz, inten)                         # odd stride
    assert rc == capi.CC_ERR_INVALID_ARGUMENT and b"packet_stride" in err()
    assert dec.decode_raw(1, pk, 1204, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT          # shorter than a payload
    assert dec.decode_raw(1, None, 1216, None, None, xyz, inten) == capi.CC_ERR_INVALID_ARGUMENT        # no packets
    assert dec.decode_raw(1, pk, 1216, None, None, xyz, inten) == capi.CC_OK                            # and a good call still runs
    dec.sync()
    written = xyz.view(-1)[: 2 * 3 * 128 * 3]                                        # [2][3][128][3]: the stream stride of a 1-packet call
    assert bool(torch.isnan(written).all()) and not bool(torch.isnan(xyz.view(-1)[2 * 3 * 128 * 3:]).any())   # header 0: all placeholders
    assert dec.counters(0)["bad_block_header"] == 3
    dec.close()
    for e in (e2, e3, e64):
        e.close()
