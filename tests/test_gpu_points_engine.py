"""GPU: PointCloud2 message bytes -> cc_points_decode on the engine's HIP stream -> cc_engine_add_firings_device gives what the same
engine gives when fed the original firing arrays, and what the oracle gives: as the reference's own raw-firing messages,
as organised clouds of 50 columns, and with skipped placeholder messages in the stream."""
import numpy as np
import pytest

import cases
import util
from continuous_clustering_amd import capi, points

pytestmark = pytest.mark.gpu

CASE = "g_s64_translate"                                    # the smallest 64-row case of tests/cases.py that finishes clusters: 800 firings
S = 2
EVENT_FIELDS = ("type", "a", "b", "c", "d", "column")
_shared = {}                                                # computed once, shared by the parametrised cases, never changed


def _published_in(engine, ev, stream=0):
    """(first column, columns) the events of one call published, read while they are fresh, or None."""
    pub = ev[(ev["type"] == capi.EV_PUBLISH_COLUMNS) & (ev["b"] >= ev["a"])]
    if not len(pub):
        return None
    lo, hi = int(pub["a"].min()), int(pub["b"].max())
    return lo, hi, engine.read_columns(lo, hi, stream=stream)


def _joined(pieces, lo, hi):
    """The per-call column reads as one set of arrays over lo .. hi (they must tile the range)."""
    pieces = [p for p in pieces if p is not None]
    assert pieces[0][0] == lo and pieces[-1][1] == hi and all(a[1] + 1 == b[0] for a, b in zip(pieces, pieces[1:]))
    return {k: np.concatenate([p[2][k] for p in pieces]) for k in pieces[0][2]}


def _reference_runs(oracle_lib):
    """The case, the oracle's record of it, and the record of an engine fed the original arrays directly."""
    if not _shared:
        from continuous_clustering_amd import Engine, IDENTITY_TF
        stream, cfg, tf = cases.build_case(CASE)
        tf = IDENTITY_TF if tf is None else tf
        oracle, rc = util.run_oracle(stream, cfg, tf)
        assert rc == 0 and stream.sensor.num_rows == 64
        evo = oracle.drain_events()
        lo, hi = oracle.published_range()
        e = Engine(cfg, 64, 1, 0, tf)
        e.record_events(True)
        events, pieces = [], []
        for f0 in range(0, stream.n_firings, 64):
            assert e.add_firings(stream.xyz[f0:f0 + 64], stream.intensity[f0:f0 + 64], stream.poses[f0:f0 + 64]) == 0 and e.sync() == 0
            events.append(e.drain_events())
            pieces.append(_published_in(e, events[-1]))
        direct = dict(events=np.concatenate(events), columns=_joined(pieces, lo, hi), state=e.state())
        e.close()
        assert (evo["type"] == capi.EV_CLUSTER).sum() > 5 and hi - lo > 100
        _shared.update(stream=stream, cfg=cfg, tf=tf, oracle=oracle, evo=evo, lo=lo, hi=hi, direct=direct)
    return _shared


def _variant(name, stream):
    """(layout, messages [M][stride], skip [M], message poses or None, firing poses or None, messages per call, kept -> fed firing)."""
    n = stream.n_firings
    rng = np.random.default_rng(77)
    if name == "organised":
        C = 50
        layout = points.layout_from_pointcloud2(64, C, 16, C * 16 + 8, [("x", 0, points.FLOAT32, 1), ("y", 4, points.FLOAT32, 1),
                                                                        ("z", 8, points.FLOAT32, 1), ("intensity", 12, points.FLOAT32, 1)],
                                                intensity_mode=points.INTENSITY_F32_255)
        pad = (-n) % C                                      # filler firings of a last, partly filled message would be all-NaN points
        xyz = np.concatenate([stream.xyz, np.full((pad, 64, 3), np.nan, dtype=np.float32)])
        inten = np.concatenate([stream.intensity, np.zeros((pad, 64), dtype=np.uint8)])
        poses = np.concatenate([stream.poses, np.repeat(stream.poses[-1:], pad, 0)])
        msg = points.write_messages(xyz, inten, layout, stride=layout.message_bytes + 5, fill=rng)
        # every firing has its own pose: the caller writes d_poses, the decoder is given no message poses and leaves them alone
        return layout, msg, np.zeros(len(msg), dtype=bool), None, poses, 4, np.arange(n)
    layout = points.raw_firing_layout(64, intensity_mode=points.INTENSITY_U8)
    msg = points.write_messages(stream.xyz, stream.intensity, layout, fill=rng)
    skip = np.zeros(n, dtype=bool)
    poses = stream.poses
    kept = np.arange(n)
    if name == "placeholders":
        # messages the reference would drop (zero stamp), marked in d_skip: garbage bytes that must not be read, a run across a call boundary
        at = np.sort(np.concatenate([[0, 1, 300, 799], np.arange(60, 70), rng.choice(np.arange(100, 780), 12, replace=False)]))
        slots = np.ones(n + len(at), dtype=bool)
        slots[at + np.arange(len(at))] = False              # position of the inserted messages in the fed stream
        kept = np.nonzero(slots)[0]
        full = rng.integers(0, 256, (n + len(at), msg.shape[1]), dtype=np.uint8)
        full[kept] = msg
        fposes = np.zeros((n + len(at), 12))
        fposes[kept] = poses
        msg, skip, poses = full, ~slots, fposes
    return layout, msg, skip, poses, None, 64, kept


@pytest.mark.parametrize("name", ["raw_firing", "organised", "placeholders"])
def test_messages_to_engine_equal_direct_feed_and_oracle(oracle_lib, name):
    import torch
    from continuous_clustering_amd import Engine
    ref = _reference_runs(oracle_lib)
    stream, cfg, evo, lo, hi = ref["stream"], ref["cfg"], ref["evo"], ref["lo"], ref["hi"]
    layout, msg, skip, mposes, fposes, per_call, kept = _variant(name, stream)
    C, M = layout.columns, len(msg)
    assert name != "placeholders" or skip.sum() == 26

    e = Engine(cfg, 64, S, robot_from_sensor=ref["tf"])
    e.record_events(True)
    e.set_option("input_on_engine_stream", 1)
    dec = points.PointsDecoder(S, layout, max_messages=per_call, hip_stream=e.hip_stream())
    dec.check_engine(e)
    dev = torch.device("cuda")
    calls = []
    for m0 in range(0, M, per_call):
        m = min(per_call, M - m0)
        d_msg = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(msg[m0:m0 + m], (S, m, msg.shape[1])))).to(dev)
        d_skip = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(skip[m0:m0 + m].astype(np.uint8), (S, m)))).to(dev)
        d_mp = None if mposes is None else torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mposes[m0:m0 + m], (S, m, 12)))).to(dev)
        out = dict(xyz=torch.empty((S, m * C, 64, 3), dtype=torch.float32, device=dev),
                   intensity=torch.empty((S, m * C, 64), dtype=torch.uint8, device=dev),
                   poses=torch.empty((S, m * C, 12), dtype=torch.float64, device=dev))
        if fposes is not None:
            out["poses"].copy_(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(fposes[m0 * C:(m0 + m) * C], (S, m * C, 12)))))
        calls.append((m, d_msg, d_skip, d_mp, out))
    torch.cuda.synchronize()
    events, pieces = [[] for _ in range(S)], [[] for _ in range(S)]
    for m, d_msg, d_skip, d_mp, out in calls:
        dec.decode(d_msg, d_mp, d_skip, out=out)
        e.add_firings_device(m * C, out["xyz"], out["intensity"], out["poses"])
        assert e.sync() == 0, e.last_error()
        for s in range(S):
            events[s].append(e.drain_events(s))
            pieces[s].append(_published_in(e, events[s][-1], s))
    ao = ref["oracle"].read_published(lo, hi)
    ao["source_firing"] = np.where(ao["source_firing"] >= 0, kept[np.clip(ao["source_firing"], 0, None)], ao["source_firing"])
    direct = dict(ref["direct"]["columns"])
    direct["source_firing"] = ao["source_firing"]
    for s in range(S):
        ev = np.concatenate(events[s])
        for other in (evo, ref["direct"]["events"]):        # the oracle's record, and the engine's own when fed the arrays directly
            assert len(ev) == len(other), (s, len(ev), len(other))
            for fld in EVENT_FIELDS:
                assert np.array_equal(ev[fld], other[fld]), (s, fld)
        ae = _joined(pieces[s], lo, hi)
        util.compare_columns(ao, ae, lo)                    # ground labels, cluster ids and every other published field: the oracle's
        util.compare_columns(direct, ae, lo)                # and the direct feed's
        so, se = ref["oracle"].state(), e.state(s)
        for k in util.STATE_FIELDS:
            if k != "firings_consumed":
                assert so[k] == se[k] == ref["direct"]["state"][k], (s, k)
        assert se["firings_consumed"] == M * C and so["firings_consumed"] == stream.n_firings == len(kept)
        assert dec.counters(s)["skipped_messages"] == int(skip.sum())
    dec.close()                                             # before the engine whose HIP stream it uses
    e.close()
