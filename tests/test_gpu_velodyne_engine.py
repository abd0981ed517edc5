"""GPU: Velodyne VLS-128 packets -> cc_velodyne_decode on the engine's HIP stream -> cc_engine_add_firings_device gives, per stream, what
the oracle gives for the valid reference-decoded firings alone. The first input of the 128-row multi-column insertion
whose per-laser azimuths come from a calibration and the in-packet interpolation."""
import math

import numpy as np
import pytest

import util
import velodyne_ref
from continuous_clustering_amd import capi, synth, velodyne

pytestmark = pytest.mark.gpu

S = 3
N_PACKETS = 2 * velodyne.rotation_packets() + 40
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
_inputs, _oracles = {}, {}                                  # computed once per variant, shared by the parametrised cases, never changed


def _tilted_mount():
    """robot_from_sensor of a tilted roof mount: yaw 40 deg, pitch 8 deg, roll -5 deg, 1.1 m ahead, 0.75 m left, 1.95 m up."""
    def rz(a):
        return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])

    def ry(a):
        return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])

    def rx(a):
        return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])

    R = rz(math.radians(40)) @ ry(math.radians(8)) @ rx(math.radians(-5))
    return np.concatenate([R, np.array([[1.1], [0.75], [1.95]])], 1).reshape(12)


def _stream_inputs(damaged: bool):
    """packets [S][P][1206], packet poses, skip, calibrations and the reference decode of three streams with different motions."""
    if damaged not in _inputs:
        cals = [velodyne.synthetic_calibration(0), velodyne.synthetic_calibration(0), velodyne.synthetic_calibration(7)]
        motions = [synth.Motion.translate(5.0), synth.Motion.turn(6.0, 0.3), synth.Motion.static()]
        ct, st = velodyne.rotation_tables()
        pk, pp = [], []
        skip = np.zeros((S, N_PACKETS), dtype=bool)
        for s in range(S):
            sp = velodyne.synthetic_packets(cals[s], N_PACKETS, seed=300 + s, motion=motions[s], first_packet=7 * s)
            hdr = np.tile(np.array(velodyne.BANK_HEADERS, dtype=np.uint16), (N_PACKETS, 3))
            mode = np.full(N_PACKETS, 55)
            if damaged:
                rng = np.random.default_rng(900 + s)
                hit = rng.uniform(0, 1, N_PACKETS) < 0.03
                hdr[hit, rng.integers(0, 12, hit.sum())] = rng.choice([0, 0xFFEE, 0xDDFF])
                mode[[50 + s, 400]] = 57
            pk.append(velodyne.write_packets(sp["raw_distance"], sp["intensity"], sp["rotation"], headers=hdr, return_mode=mode))
            pp.append(sp["packet_poses"])
        if damaged:
            skip[0, [5, 70]] = skip[1, 100] = True
        pk, pp = np.stack(pk), np.stack(pp)
        refs = [velodyne_ref.decode(pk[s], ct, st, cals[s], skip=skip[s], packet_poses=pp[s]) for s in range(S)]
        _inputs[damaged] = (pk, pp, skip, cals, refs)
    return _inputs[damaged]


def _oracle_runs(damaged: bool, tilted: bool, cfg, robot_tf):
    """Per stream: the oracle fed only the valid firings, its events, and the firing number of each kept firing in the full stream."""
    from oracle.pyoracle import Oracle
    if (damaged, tilted) not in _oracles:
        refs = _stream_inputs(damaged)[4]
        runs = []
        for s in range(S):
            v = refs[s]["valid"]
            o = Oracle(cfg, 128, robot_tf)
            assert o.add_firings(refs[s]["xyz"][v], refs[s]["intensity"][v], refs[s]["poses"][v]) == 0
            runs.append((o, o.drain_events(), np.nonzero(v)[0]))
        _oracles[(damaged, tilted)] = runs
    return _oracles[(damaged, tilted)]


@pytest.mark.parametrize("damaged", [False, True], ids=["undamaged", "placeholders"])
@pytest.mark.parametrize("packets_per_call,tilted", [(1, False), (3, False), (64, False), (3, True)])
def test_packets_to_engine_equal_oracle_on_valid_firings(oracle_lib, packets_per_call, tilted, damaged):
    """packets -> cc_velodyne_decode on cc_engine_hip_stream(e) ("input_on_engine_stream") -> cc_engine_add_firings_device over two
    rotations plus 40 packets of three streams equals, per stream, the oracle fed only the valid numpy-decoded firings."""
    import torch
    from continuous_clustering_amd import Engine
    packets, pposes, skip, cals, refs = _stream_inputs(damaged)
    robot_tf = _tilted_mount() if tilted else IDENTITY
    cfg = capi.Config.vls128()
    assert cfg.num_columns == 1700
    runs = _oracle_runs(damaged, tilted, cfg, robot_tf)
    for s in range(S):
        n_placeholders = int((~refs[s]["valid"]).sum())
        assert n_placeholders > 20 if damaged else n_placeholders == 0

    e = Engine(cfg, 128, S, robot_from_sensor=robot_tf)
    e.record_events(True)
    e.set_option("input_on_engine_stream", 1)
    dec = velodyne.VelodyneDecoder(S, max_packets=packets_per_call, hip_stream=e.hip_stream())
    dec.check_engine(e)
    for s in range(S):
        dec.set_calibration(cals[s], stream=s)

    dev = torch.device("cuda")
    d_packets, d_pposes = torch.from_numpy(packets).to(dev), torch.from_numpy(pposes).to(dev)
    d_skip = torch.from_numpy(skip.astype(np.uint8)).to(dev)
    calls = []
    for p0 in range(0, N_PACKETS, packets_per_call):
        m = min(packets_per_call, N_PACKETS - p0)
        calls.append((m, d_packets[:, p0:p0 + m].contiguous(), d_pposes[:, p0:p0 + m].contiguous(), d_skip[:, p0:p0 + m].contiguous()))
    torch.cuda.synchronize()
    pos = [0] * S
    for m, d_pk, d_pp, d_sk in calls:
        out = dec.decode(d_pk, d_pp, d_sk)
        e.add_firings_device(m * 3, out["xyz"], out["intensity"], out["poses"])
        assert e.sync() == 0, e.last_error()
        for s in range(S):
            oracle, evo, kept_to_full = runs[s]
            ev = e.drain_events(s)
            ref = evo[pos[s]:pos[s] + len(ev)]
            assert len(ev) == len(ref), (s, pos[s], len(ev), len(evo))
            for fld in ("type", "a", "b", "c", "d", "column"):
                assert np.array_equal(ev[fld], ref[fld]), (s, fld)
            pos[s] += len(ev)
            pub = ev[(ev["type"] == capi.EV_PUBLISH_COLUMNS) & (ev["b"] >= ev["a"])]
            if len(pub):
                lo, hi = int(pub["a"].min()), int(pub["b"].max())
                ao, ae = oracle.read_published(lo, hi), e.read_columns(lo, hi, stream=s)
                src = ao["source_firing"]
                ao["source_firing"] = np.where(src >= 0, kept_to_full[np.clip(src, 0, None)], src)  # placeholders are counted
                util.compare_columns(ao, ae, lo)
    for s in range(S):
        oracle, evo, kept_to_full = runs[s]
        assert pos[s] == len(evo) and (evo["type"] == capi.EV_CLUSTER).sum() > 5
        so, se = oracle.state(), e.state(s)
        for k in util.STATE_FIELDS:
            if k != "firings_consumed":
                assert so[k] == se[k], (s, k)
        assert se["firings_consumed"] == N_PACKETS * 3 and so["firings_consumed"] == len(kept_to_full)
    c = dec.counters(0)
    if damaged:
        assert c["skipped_packets"] == 2 and c["dual_return_packets"] == 2 and c["bad_block_header"] > 0
    else:
        assert c == dict(bad_block_header=0, dual_return_packets=0, skipped_packets=0)
    dec.close()                                                                      # before the engine whose HIP stream it uses
    e.close()
