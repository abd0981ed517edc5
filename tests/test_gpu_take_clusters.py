"""GPU: cc_engine_take_clusters — the clusters finished since the last take, of all streams, as descriptors and grouped point records in
device memory. The takes of a run, one after the other, must be the oracle's CC_EV_CLUSTER events, cluster for cluster, and
their records the published cells that carry the id; clusters must come out while their columns are still unpublished; a take that does not
fit must leave everything as it was; what was cleared before anybody took it must be counted, not invented; and taking between pipelined
calls must disturb neither the engine nor the cursors of cc_engine_take_points."""
import ctypes

import numpy as np
import pytest

import util
from continuous_clustering_amd import capi, synth, take

pytestmark = pytest.mark.gpu

CL, ALL = take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS
FU = "first_unpublished_global_column_index"
BOX = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z")


# ---- helpers (as in test_gpu_take.py) -------------------------------------------------------------------------------------------------------
def _sensor(rows, cols):
    if rows == 128:
        sen = synth.SensorModel.s128()
        sen.num_columns = cols
        return sen
    if rows == 32:
        return synth.SensorModel(num_rows=32, num_columns=cols, incl_top_deg=10.0, incl_bottom_deg=-30.0)
    return synth.SensorModel(num_rows=rows, num_columns=cols)


def _config(rows, cols):
    cfg = capi.Config.vls128() if rows == 128 else capi.Config.kitti()
    cfg.num_columns = cols
    return cfg


def _streams(rows, cols, rotations, seed, nan_last=True):
    """static, turning and (nan_last) one without a single return, which never starts"""
    sen = _sensor(rows, cols)
    start = 16 if rows == 128 else 0  # (per-laser azimuth offsets: the first firings would reach in front of column 0)
    out = [synth.make_stream(cols * rotations, seed=seed, sensor=sen, motion=synth.Motion.static(), start_column=start),
           synth.make_stream(cols * rotations, seed=seed + 1, sensor=sen, motion=synth.Motion.turn(), start_column=start)]
    if nan_last:
        st = out[0]
        out.append(synth.Stream(xyz=np.full_like(st.xyz, np.nan), intensity=st.intensity, poses=st.poses, sensor=sen))
    return out


def _device_inputs(torch, streams, NB, F):
    R = streams[0].sensor.num_rows
    xyz = torch.from_numpy(np.stack([st.xyz[:NB * F].reshape(NB, F, R, 3) for st in streams], axis=1)).cuda()
    inten = torch.from_numpy(np.stack([st.intensity[:NB * F].reshape(NB, F, R) for st in streams], axis=1)).cuda()
    poses = torch.from_numpy(np.stack([st.poses[:NB * F].reshape(NB, F, 12) for st in streams], axis=1)).cuda()
    torch.cuda.synchronize()
    return xyz, inten, poses


def _host(records):
    return records.cpu().numpy().reshape(-1).view(take.TAKE_POINT_DTYPE)


def _host_clusters(clusters):
    return clusters.cpu().numpy().reshape(-1).view(take.TAKE_CLUSTER_DTYPE)


def _same(a, b):
    """bit for bit"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _reference_records(cols: dict, lo: int):
    """the returns of a column view (oracle's read_published / the engine's read_columns) of columns lo .. as records + global columns"""
    has = ~np.isnan(cols["distance"])
    c, r = np.nonzero(has)  # (column, row) order
    rec = np.zeros(len(c), dtype=take.TAKE_POINT_DTYPE)
    for f in ("x", "y", "z", "distance", "ground_point_label"):
        rec[f] = cols[f][has]
    rec["id"] = cols["id"][has].astype(np.uint32)
    assert (cols["id"][has] < 2 ** 32).all()
    rec["source_firing"] = (cols["source_firing"][has] & 0xffffffff).astype(np.uint32)
    rec["row"] = r
    return rec, c.astype(np.int64) + lo


def _assert_records_equal(got, got_gcol, ref, ref_gcol, intensity=None, what=""):
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert np.array_equal(got_gcol, ref_gcol) and np.array_equal(got["row"], ref["row"]), what
    for f in ("x", "y", "z", "distance"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), (what, f)    # bitwise
    for f in ("ground_point_label", "source_firing", "id"):
        assert np.array_equal(got[f], ref[f]), (what, f)
    if intensity is not None:
        assert np.array_equal(got["intensity"], intensity[got["source_firing"].astype(np.int64), got["row"]]), what


class PointLog:
    """the cc_engine_take_points takes of one engine (CLUSTERED stage): per stream the records with GLOBAL columns"""

    def __init__(self, S):
        self.rec = [[] for _ in range(S)]
        self.gcol = [[] for _ in range(S)]
        self.to = [0] * S
        self.started = [False] * S

    def add(self, records, table):
        rec = _host(records)
        pos = 0
        for s in range(len(self.rec)):
            t = table[s]
            assert t["error"] == 0 and t["lost_columns"] == 0 and t["first_record"] == pos, (s, t)
            assert t["col_from"] == self.to[s] or (not self.started[s] and t["col_from"] >= 0), (s, t, self.to[s])  # where the previous one ended
            self.started[s] = self.started[s] or t["col_to"] > t["col_from"]
            r = rec[pos:pos + int(t["n_records"])]
            pos += int(t["n_records"])
            self.rec[s].append(r)
            self.gcol[s].append(r["column"].astype(np.int64) + int(t["col_from"]))
            self.to[s] = int(t["col_to"])
        assert pos == len(rec)

    def of(self, s):
        return np.concatenate(self.rec[s]), np.concatenate(self.gcol[s])


# ---- the cluster takes of one engine ----------------------------------------------------------------------------------------------------------
def _check_cluster(d, r, what):
    """one descriptor against its own records: id, order, span, bounding box, firing range"""
    assert len(r) == d["n_points"] > 0, what
    assert (r["id"] == d["id"]).all(), what
    key = r["column"].astype(np.int64) * 256 + r["row"]
    assert (np.diff(key) > 0).all(), what                                          # strictly increasing in (column, row)
    assert r["column"][0] == 0 and r["column"][-1] == d["n_columns"] - 1, what      # counted from the cluster's own first column, to its last
    for f, v in zip(BOX, (r["x"].min(), r["y"].min(), r["z"].min(), r["x"].max(), r["y"].max(), r["z"].max())):
        assert d[f] == v or (np.isnan(d[f]) and np.isnan(v)), (what, f, d[f], v)    # (== : -0 equals +0; a NaN only equals a NaN)
    assert d["firing_min"] == r["source_firing"].min() and d["firing_max"] == r["source_firing"].max(), what


class ClusterLog:
    """per stream the descriptors of all takes and (with points) every cluster's records, and the checks every single take must pass"""

    def __init__(self, S, min_points, with_points=True):
        self.S, self.min_points, self.with_points = S, min_points, with_points
        self.desc = [[] for _ in range(S)]
        self.rec = [[] for _ in range(S)]  # one array per descriptor
        self.next_id = [1] * S
        self.raw = []                      # (descriptor bytes, record bytes, table) per take

    def add(self, clusters, records, table, counters=None, lost_ok=False):
        cl = _host_clusters(clusters)
        rec = _host(records) if self.with_points else None
        self.raw.append((cl.tobytes(), rec.tobytes() if self.with_points else b"", table.copy()))
        cpos, rpos = 0, 0
        for s in range(self.S):
            t = table[s]
            assert t["error"] == 0 and (lost_ok or t["lost_columns"] == 0), (s, t)
            assert t["first_cluster"] == cpos and t["first_record"] == rpos, (s, t, cpos, rpos)   # the slices abut
            assert t["id_from"] == self.next_id[s] and t["id_to"] >= t["id_from"], (s, t, self.next_id[s])
            if counters is not None:
                assert t["id_to"] == counters[s], (s, t, counters[s])
            d = cl[cpos:cpos + int(t["n_clusters"])]
            assert (d["stream"] == s).all() and (np.diff(d["id"].astype(np.int64)) > 0).all(), s
            assert ((d["id"] >= t["id_from"]) & (d["id"] < t["id_to"])).all(), s
            assert (d["n_points"] >= max(self.min_points, 1)).all() and (d["n_columns"] >= 1).all(), s
            first = rpos + np.concatenate([[0], np.cumsum(d["n_points"].astype(np.int64))])
            assert np.array_equal(d["first_record"], first[:-1]) and t["n_records"] == first[-1] - rpos, s  # grouped by descriptor, no gaps
            for i in range(len(d)):
                self.desc[s].append(d[i])
                if self.with_points:
                    r = rec[first[i]:first[i + 1]]
                    _check_cluster(d[i], r, (s, int(d[i]["id"])))
                    self.rec[s].append(r)
            cpos += len(d)
            rpos = int(first[-1])
            self.next_id[s] = int(t["id_to"])
        assert cpos == len(cl) and (not self.with_points or rpos == len(rec))

    def descriptors(self, s):
        return np.array(self.desc[s], dtype=take.TAKE_CLUSTER_DTYPE)


def _oracle_run(stream, cfg, n_firings):
    from oracle.pyoracle import Oracle
    o = Oracle(cfg, stream.sensor.num_rows)
    assert o.add_firings(stream.xyz[:n_firings], stream.intensity[:n_firings], stream.poses[:n_firings]) == 0
    ev = o.drain_events()
    return o, ev[ev["type"] == capi.EV_CLUSTER], int(ev[ev["type"] == capi.EV_GROUND_COLUMN]["a"][0])


def _assert_descriptors_are_events(d, ev, what):
    assert len(d) == len(ev), (what, len(d), len(ev))
    last = d["col_from"] + d["n_columns"].astype(np.int64) - 1
    for got, ref, name in ((d["id"], ev["c"], "id"), (d["col_from"], ev["a"], "col_from"), (last, ev["b"], "last column"), (d["n_points"], ev["d"], "n_points")):
        assert np.array_equal(got.astype(np.int64), ref.astype(np.int64)), (what, name)


def _by_id(ref, ref_gcol):
    """{id: (records, global columns)} of a record array in (column, row) order; the order inside an id is kept"""
    order = np.argsort(ref["id"], kind="stable")
    ids, starts = np.unique(ref["id"][order], return_index=True)
    ends = list(starts[1:]) + [len(order)]
    return {int(i): (ref[order[a:b]], ref_gcol[order[a:b]]) for i, a, b in zip(ids, starts, ends)}


def _against_oracle(log, s, stream, cfg, n_firings, fu, what=""):
    """the parity of test 1: descriptors == the oracle's cluster events in order, records == the published cells carrying the id. Returns
    (clusters handed over, clusters whose points could not be compared because they reach first_unpublished)."""
    o, ev, lo = _oracle_run(stream, cfg, n_firings)
    assert o.state()[FU] == fu, (what, fu)
    if log.min_points <= 6:
        assert np.array_equal(ev["c"], np.arange(1, len(ev) + 1)), what                 # ids are a counter: 1, 2, ... without a gap
    ev = ev[ev["d"] >= log.min_points]
    d = log.descriptors(s)
    _assert_descriptors_are_events(d, ev, what)
    if log.min_points <= 6:
        assert np.array_equal(d["id"], np.arange(1, len(d) + 1)), what
    cells = _by_id(*_reference_records(o.read_published(lo, fu - 1), lo))
    skipped = 0
    for i in range(len(d)):
        if d[i]["col_from"] + d[i]["n_columns"] - 1 >= fu:
            skipped += 1
            continue
        ref, ref_gcol = cells[int(d[i]["id"])]
        got = log.rec[s][i]
        _assert_records_equal(got, got["column"].astype(np.int64) + int(d[i]["col_from"]), ref, ref_gcol, stream.intensity, (what, int(d[i]["id"])))
    return len(d), skipped


def _run_device(streams, cfg, NB, per_call=None, setup=None):
    """one rotation per add_firings_device call on a fresh engine (events off); per_call(engine, b) after every call"""
    import torch
    from continuous_clustering_amd import Engine
    rows, cols = streams[0].sensor.num_rows, streams[0].sensor.num_columns
    xyz, inten, poses = _device_inputs(torch, streams, NB, cols)
    e = Engine(cfg, rows, len(streams))
    e.record_events(False)
    if setup:
        setup(e)
    for b in range(NB):
        e.add_firings_device(cols, xyz[b], inten[b], poses[b])
        if per_call:
            per_call(e, b)
    assert e.sync() == 0, e.last_error()
    return e


def _counters(e, S):
    return [e.state(s)["cluster_counter"] for s in range(S)]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [32, 64, 128])
def test_takes_concatenate_to_the_oracles_cluster_events(rows, oracle_lib):
    """a partial wavefront, a full one, two trips; three streams of which the last never starts; twelve rotations through the ring of ten"""
    cols, NB, S = (256 if rows == 32 else 360), 12, 3
    streams, cfg = _streams(rows, cols, NB, 9600 + rows), _config(rows, cols)
    log = ClusterLog(S, 6)
    e = _run_device(streams, cfg, NB, lambda e, b: log.add(*e.take_clusters(6), counters=_counters(e, S)))
    assert e.state(0)["ring_buffer_start_global_column_index"] > cols        # the ring start has moved: cleared columns lie behind the floors
    assert len(log.desc[2]) == 0 and e.state(2)[FU] < 0 and e.take_clusters_cursor(2)[0] == 1
    total = skipped = 0
    for s in (0, 1):
        fu = e.state(s)[FU]
        assert fu > 10 * cols                                                # every local column has been re-used
        n, k = _against_oracle(log, s, streams[s], cfg, NB * cols, fu, what=f"stream {s}")
        assert n >= 50, (s, n)
        assert e.take_clusters_cursor(s)[:2] == (e.state(s)["cluster_counter"], fu)
        total, skipped = total + n, skipped + k
    print(f"rows {rows}: {total} clusters, {skipped} beyond first_unpublished at the end")
    assert skipped <= 0.05 * total, (skipped, total)
    e.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------
def _clutter_streams():
    rows, cols, NB = 64, 360, 4
    sen, scene = _sensor(rows, cols), synth.SceneModel.near_clutter()
    return [synth.make_stream(cols * NB, seed=9800, sensor=sen, scene=scene, motion=synth.Motion.static()),
            synth.make_stream(cols * NB, seed=9801, sensor=sen, scene=scene, motion=synth.Motion.translate())], _config(rows, cols), NB


def test_clusters_that_share_columns(oracle_lib):
    import torch
    streams, cfg, NB = _clutter_streams()
    S, cols = 2, 360
    deepest = 0
    for st in streams:                                                       # the scene does what it is here for: clusters side by side
        _, ev, _ = _oracle_run(st, cfg, NB * cols)
        ev = ev[ev["d"] >= 21]
        cover = np.zeros(int(ev["b"].max()) + 2, dtype=np.int64)
        np.add.at(cover, ev["a"], 1)
        np.add.at(cover, ev["b"] + 1, -1)
        deepest = max(deepest, int(np.cumsum(cover).max()))
    assert deepest >= 3, deepest
    logs = {"21": ClusterLog(S, 21), "6": ClusterLog(S, 6), "desc": ClusterLog(S, 21, with_points=False)}
    sentinel = torch.full((64, 32), 0xA5, dtype=torch.uint8, device="cuda")
    calls = {"21": lambda e, b: logs["21"].add(*e.take_clusters(21), counters=_counters(e, S)),
             "6": lambda e, b: logs["6"].add(*e.take_clusters(6), counters=_counters(e, S)),
             "desc": lambda e, b: logs["desc"].add(*e.take_clusters(21, descriptors_only=True, records=sentinel), counters=_counters(e, S))}
    cursors = {}
    for k in ("21", "6", "desc"):
        e = _run_device(streams, cfg, NB, calls[k])
        cursors[k] = [e.take_clusters_cursor(s) for s in range(S)]
        if k == "21":
            for s in range(S):
                n, skipped = _against_oracle(logs[k], s, streams[s], cfg, NB * cols, e.state(s)[FU], what=f"stream {s}")
                print(f"stream {s}: {n} clusters of >= 21 points, {skipped} beyond first_unpublished at the end")
                assert n >= 50 and skipped <= 0.05 * n, (s, n, skipped)
        e.close()
    assert cursors["21"] == cursors["6"] == cursors["desc"]                  # clusters below the threshold are consumed too
    assert (sentinel.cpu().numpy() == 0xA5).all()                            # DESCRIPTORS_ONLY writes no record
    kept = seen = 0
    for (c21, r21, t21), (c6, r6, t6), (cd, rd, td) in zip(logs["21"].raw, logs["6"].raw, logs["desc"].raw):
        assert cd == c21 and rd == b"" and _same(td, t21)                    # the same descriptors without the points
        d = np.frombuffer(c6, dtype=take.TAKE_CLUSTER_DTYPE)
        r = np.frombuffer(r6, dtype=take.TAKE_POINT_DTYPE)
        keep = d["n_points"] >= 21
        kept, seen = kept + int(keep.sum()), seen + len(d)
        packed = d[keep].copy()                                              # min_points = 6 filtered and repacked is min_points = 21
        packed["first_record"] = np.concatenate([[0], np.cumsum(packed["n_points"].astype(np.int64))])[:-1]
        points = [r[int(a):int(a) + int(n)] for a, n in zip(d["first_record"][keep], d["n_points"][keep])]
        assert packed.tobytes() == c21
        assert (np.concatenate(points).tobytes() if points else b"") == r21
        for s in range(S):
            assert all(t21[s][f] == t6[s][f] for f in ("id_from", "id_to", "lost_columns", "error")), s
    assert 0 < kept < seen, (kept, seen)                                     # the threshold filtered something, and not everything


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------
def test_clusters_come_ahead_of_publication_and_after_reset(oracle_lib):
    """one stream on the host path, events on: calls of 97 firings and of 7 (the one-launch path of calls below 64 firings)"""
    from continuous_clustering_amd import Engine
    rows, cols = 64, 360
    stream = synth.make_stream(cols * 3, seed=9500, sensor=_sensor(rows, cols), scene=synth.SceneModel.near_clutter(), motion=synth.Motion.translate())
    cfg = _config(rows, cols)
    e = Engine(cfg, rows)
    runs = []
    for run in range(2):
        assert e.take_clusters_cursor(0)[0] == 1
        log = ClusterLog(1, 21)
        ahead, pending, compared = 0, [], 0                                  # pending: indices into log.desc[0], last column >= first_unpublished
        f, i = 0, 0
        while f < stream.n_firings:
            m = min((97, 7)[i % 2], stream.n_firings - f)
            assert e.add_firings(stream.xyz[f:f + m], stream.intensity[f:f + m], stream.poses[f:f + m]) == 0, e.last_error()
            f += m
            i += 1
            ev = e.drain_events()
            ev = ev[(ev["type"] == capi.EV_CLUSTER) & (ev["d"] >= 21)]
            st = e.state()
            before = len(log.desc[0])
            log.add(*e.take_clusters(21), counters=[st["cluster_counter"]])
            d = log.descriptors(0)[before:]
            _assert_descriptors_are_events(d, ev, f"call {i}")                # each take is that call's own finished clusters
            new = [before + k for k in range(len(d)) if d[k]["col_from"] + d[k]["n_columns"] - 1 >= st[FU]]
            ahead += len(new)
            pending += new
            if run == 0:                                                      # ... and are what is published under their id later on
                for k in [k for k in pending if log.desc[0][k]["col_from"] + log.desc[0][k]["n_columns"] - 1 < st[FU]]:
                    c = log.desc[0][k]
                    a, b = int(c["col_from"]), int(c["col_from"] + c["n_columns"] - 1)
                    assert e.take_clusters_cursor(0)[2] <= a                  # (a rotation passes between publication and clearing)
                    ref, ref_gcol = _reference_records(e.read_columns(a, b), a)
                    mine = ref["id"] == c["id"]
                    got = log.rec[0][k]
                    _assert_records_equal(got, got["column"].astype(np.int64) + a, ref[mine], ref_gcol[mine], stream.intensity, int(c["id"]))
                    pending.remove(k)
                    compared += 1
        st = e.state()
        if run == 0:
            print(f"{ahead} of {len(log.desc[0])} clusters were handed over ahead of publication, {compared} compared once published")
            assert ahead >= 10 and compared >= 10, (ahead, compared, len(log.desc[0]))
        assert e.take_clusters_cursor(0)[:2] == (st["cluster_counter"], st[FU])
        runs.append(log.raw)
        e.reset()
        e.set_robot_from_sensor(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64))
    assert e.take_clusters_cursor(0)[0] == 1
    assert len(runs[0]) == len(runs[1])
    for (c0, r0, t0), (c1, r1, t1) in zip(*runs):
        assert c0 == c1 and r0 == r1 and _same(t0, t1)
    e.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_all_or_nothing_over_both_arrays(oracle_lib):
    import torch
    from continuous_clustering_amd import TakeCapacityError
    rows, cols, NB, S = 64, 360, 3, 3
    streams, cfg = _streams(rows, cols, NB, 9300), _config(rows, cols)
    e, fresh = _run_device(streams, cfg, NB), _run_device(streams, cfg, NB)
    before = [e.take_clusters_cursor(s) for s in range(S)]
    assert all(c[0] == 1 for c in before)
    N, M, need = e.take_clusters_size(6)
    assert N > 20 and M > 6 * N and need["n_clusters"].sum() == N and need["n_records"].sum() == M
    assert [e.take_clusters_cursor(s) for s in range(S)] == before          # the size query moves nothing
    cbuf = torch.full((N + 1, 64), 0xA5, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((M + 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    for cl, rec in ((cbuf[:N - 1], rbuf[:M]), (cbuf[:N], rbuf[:M - 1])):     # short by one cluster, short by one record
        with pytest.raises(TakeCapacityError) as ei:
            e.take_clusters(6, clusters=cl, records=rec)
        assert ei.value.code == capi.CC_ERR_CAPACITY and (ei.value.needed_clusters, ei.value.needed) == (N, M)
        assert np.array_equal(ei.value.table, need)
        assert [e.take_clusters_cursor(s) for s in range(S)] == before      # no cursor moved
        assert (cbuf.cpu().numpy() == 0xA5).all() and (rbuf.cpu().numpy() == 0xA5).all()   # nothing written, inside the capacity or behind it
    c, r, t = e.take_clusters(6, clusters=cbuf[:N], records=rbuf[:M])
    assert (cbuf[N:].cpu().numpy() == 0xA5).all() and (rbuf[M:].cpu().numpy() == 0xA5).all()
    c2, r2, t2 = fresh.take_clusters(6)
    assert len(c) == N == len(c2) and len(r) == M == len(r2) and np.array_equal(t, t2) and np.array_equal(t, need)
    assert np.array_equal(c.cpu().numpy(), c2.cpu().numpy()) and np.array_equal(r.cpu().numpy(), r2.cpu().numpy())  # a retry = a first call
    ClusterLog(S, 6).add(c, r, t, counters=_counters(e, S))
    assert [e.take_clusters_cursor(s)[:2] for s in range(S)] == [(e.state(s)["cluster_counter"], max(e.state(s)[FU], 0)) for s in range(S)]
    assert e.take_clusters_size(6)[:2] == (0, 0)
    c, r, t = e.take_clusters(6)
    assert len(c) == 0 and len(r) == 0 and (t["n_clusters"] == 0).all() and (t["id_from"] == t["id_to"]).all()
    e.close()
    fresh.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------
def test_clusters_cleared_before_a_take_are_lost_not_invented():
    import torch
    from continuous_clustering_amd import Engine
    rows, cols, S, NB = 32, 256, 2, 14
    streams = _streams(rows, cols, NB, 9400, nan_last=False)
    xyz, inten, poses = _device_inputs(torch, streams, NB, cols)
    e = Engine(_config(rows, cols), rows, S)
    e.record_events(False)
    fed = 0
    while fed < NB and min(e.take_clusters_cursor(s)[2] for s in range(S)) <= 0:
        e.add_firings_device(cols, xyz[fed], inten[fed], poses[fed])
        fed += 1
    cur = [e.take_clusters_cursor(s) for s in range(S)]
    assert all(n == 1 and lo > fl for n, fl, lo in cur), (fed, cur)          # nobody took anything while the ring went round
    log = ClusterLog(S, 6)
    clusters, records, table = e.take_clusters(6)
    log.add(clusters, records, table, counters=_counters(e, S), lost_ok=True)
    for s in range(S):
        st, readable = e.state(s), cur[s][2]
        assert table[s]["lost_columns"] == readable - cur[s][1] > 0, (s, table[s], cur[s])
        assert table[s]["id_from"] == 1 and e.take_clusters_cursor(s)[:2] == (st["cluster_counter"], st[FU])
        d = log.descriptors(s)
        assert 0 < len(d) < st["cluster_counter"] - 1                        # some clusters lay wholly below what was cleared
        assert (d["col_from"] >= readable).all(), s
        hi = st["first_unfinished_global_column_index"] - 1
        cells = _by_id(*_reference_records(e.read_columns(readable, hi, stream=s), readable))
        assert set(int(i) for i in d["id"]) == set(i for i, v in cells.items() if i != 0 and len(v[0]) >= 6), s   # nothing dropped that is there
        for i in range(len(d)):
            ref, ref_gcol = cells[int(d[i]["id"])]
            got = log.rec[s][i]
            _assert_records_equal(got, got["column"].astype(np.int64) + int(d[i]["col_from"]), ref, ref_gcol, streams[s].intensity, (s, int(d[i]["id"])))
    _, _, again = e.take_clusters(6)
    assert (again["lost_columns"] == 0).all() and (again["n_clusters"] == 0).all()
    e.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 2])
def test_take_clusters_between_pipelined_calls(pipeline, oracle_lib):
    """the configuration of test_pipelined_throughput_path_matches_oracle with a cluster take AND a point take after every call: the engine
    ends where the oracle does and neither take disturbs the other's cursors"""
    import torch
    from oracle.pyoracle import Oracle
    sen = synth.SensorModel(num_rows=64, num_columns=720)
    cfg = capi.Config.kitti()
    cfg.num_columns = 720
    S, F, NB = 8, 720, 5
    motions = [synth.Motion.static(), synth.Motion.translate(), synth.Motion.turn()]
    streams = [synth.make_stream(F * NB, seed=300 + s, sensor=sen, motion=motions[s % 3]) for s in range(S)]
    log, points = ClusterLog(S, 6), PointLog(S)
    d_table = torch.zeros(S * 56, dtype=torch.uint8, device="cuda")

    def per_call(e, b):
        clusters, records, table = e.take_clusters(6, d_table=d_table)
        assert np.array_equal(d_table.cpu().numpy().view(take.TAKE_CLUSTER_STREAM_DTYPE), table)   # the device copy of the table
        log.add(clusters, records, table)
        points.add(*e.take_points(CL, ALL))

    e = _run_device(streams, cfg, NB, per_call, setup=lambda e: e.set_option("pipeline", pipeline))
    total = skipped = 0
    for s in range(S):
        o = Oracle(cfg, 64)
        assert o.add_firings(streams[s].xyz, streams[s].intensity, streams[s].poses) == 0
        so, se = o.state(), e.state(s)
        for k in util.STATE_FIELDS:
            assert so[k] == se[k], (s, k)
        fu = se[FU]
        got, gcol = points.of(s)                                             # the point takes are still the oracle's published columns
        assert points.to[s] == fu == e.take_cursor(CL, s)[0]
        ref, ref_gcol = _reference_records(o.read_published(0, fu - 1), 0)
        _assert_records_equal(got, gcol, ref, ref_gcol, streams[s].intensity, what=f"points {s}")
        n, k = _against_oracle(log, s, streams[s], cfg, F * NB, fu, what=f"stream {s}")
        assert e.take_clusters_cursor(s)[:2] == (se["cluster_counter"], fu)
        total, skipped = total + n, skipped + k
    print(f"pipeline {pipeline}: {total} clusters, {skipped} beyond first_unpublished at the end")
    assert total >= 8 * 20 and skipped <= 0.05 * total, (total, skipped)
    e.close()


# ---- 6b ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [32, 128])
def test_cluster_records_are_the_point_takes_records(rows):
    """The two hand-overs share one rule for a cell's return and id and one writer of the 32-byte record (cc_k_held.h): after three rotations on
    two engines fed alike, one take_points(CLUSTERED, WITH_ID) and one take_clusters(1) must hold the same cells, keyed by (stream, global
    column, row), with the same 32 bytes but for `column`, which counts from another origin. A partial trip of the row loop and two trips.
    Clusters come out ahead of publication (test 4), so a cluster record in a column at or above the point take's col_to has no partner yet;
    below it the match is one to one, in both directions."""
    cols, NB, S = (256 if rows == 32 else 360), 3, 2
    streams, cfg = _streams(rows, cols, NB, 9900 + rows, nan_last=False), _config(rows, cols)
    e_pts, e_cl = _run_device(streams, cfg, NB), _run_device(streams, cfg, NB)
    points, ptab = e_pts.take_points(CL, take.TAKE_WITH_ID)
    clusters, crecords, ctab = e_cl.take_clusters(1)
    pts, cl, crec = _host(points), _host_clusters(clusters), _host(crecords)
    assert (ptab["error"] == 0).all() and (ctab["error"] == 0).all()
    assert np.array_equal(ptab["lost_columns"], ctab["lost_columns"])        # (nobody took for three rotations: both start at the oldest column held)

    def keyed(rec, stream, gcol):
        """{(stream, global column, row): the record's bytes with `column` blanked}"""
        rec = rec.copy()
        rec["column"] = 0
        raw = rec.view(np.uint8).reshape(-1, 32)
        out = {(int(s), int(c), int(r)): raw[i].tobytes() for i, (s, c, r) in enumerate(zip(stream, gcol, rec["row"]))}
        assert len(out) == len(rec)                                          # no key twice
        return out

    p_stream = np.repeat(np.arange(S), ptab["n_records"])
    assert len(p_stream) == len(pts)
    by_point = keyed(pts, p_stream, pts["column"].astype(np.int64) + ptab["col_from"][p_stream])
    owner = np.repeat(np.arange(len(cl)), cl["n_points"].astype(np.int64))   # records are grouped by descriptor, no gaps (ClusterLog.add)
    assert len(owner) == len(crec) and np.array_equal(crec["id"], cl["id"][owner])
    by_cluster = keyed(crec, cl["stream"][owner], crec["column"].astype(np.int64) + cl["col_from"][owner])
    for s in range(S):
        to = int(ptab["col_to"][s])
        published = {k: v for k, v in by_cluster.items() if k[0] == s and k[1] < to}
        ahead = sum(1 for k in by_cluster if k[0] == s and k[1] >= to)
        mine = {k: v for k, v in by_point.items() if k[0] == s}
        print(f"rows {rows}, stream {s}: {len(published)} cluster records in published columns, {ahead} ahead of publication, {len(mine)} point records")
        assert len(published) > 0
        assert published.keys() == mine.keys(), (s, len(published), len(mine))
        assert all(mine[k] == v for k, v in published.items()), s
    e_pts.close()
    e_cl.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused():
    import torch
    from continuous_clustering_amd import Engine, EngineError
    cfg = _config(64, 360)
    e = Engine(cfg, 64, 2)
    cbuf = torch.zeros((16, 64), dtype=torch.uint8, device="cuda")
    rbuf = torch.zeros((16, 32), dtype=torch.uint8, device="cuda")
    L = take._lib()
    table = np.zeros(2, dtype=take.TAKE_CLUSTER_STREAM_DTYPE)
    n, m = ctypes.c_int64(-7), ctypes.c_int64(-7)
    pn, pm, ht, cp, rp = ctypes.byref(n), ctypes.byref(m), table.ctypes.data, cbuf.data_ptr(), rbuf.data_ptr()
    bad = [(2, cp, 8, rp, 8, ht, pn, pm), (-1, cp, 8, rp, 8, ht, pn, pm),                       # flags
           (0, cp, 8, rp, 8, None, pn, pm), (0, cp, 8, rp, 8, ht, None, pm), (0, cp, 8, rp, 8, ht, pn, None),   # NULL h_table / counters
           (0, cp + 8, 8, rp, 8, ht, pn, pm), (0, cp, 8, rp + 8, 8, ht, pn, pm),                 # misaligned arrays
           (0, cp, 8, None, 0, ht, pn, pm),                                                      # no records without DESCRIPTORS_ONLY
           (0, cp, -1, rp, 8, ht, pn, pm), (0, None, 8, rp, 8, ht, pn, pm), (1, cp, 8, None, 8, ht, pn, pm)]
    for flags, c, cc, r, rc_, h, a, b in bad:
        assert L.cc_engine_take_clusters(e.h, 21, flags, c, cc, r, rc_, None, h, a, b) == capi.CC_ERR_INVALID_ARGUMENT, (flags, cc, rc_)
        assert "cc_engine_take_clusters" in e.last_error()
    assert (n.value, m.value) == (-7, -7) and not table.view(np.uint8).any()
    assert L.cc_engine_take_clusters_cursor(e.h, 2, None, None, None) == capi.CC_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        e.take_clusters(21, clusters=torch.zeros((16, 32), dtype=torch.uint8, device="cuda"), records=rbuf)
    assert L.cc_engine_take_clusters(e.h, 21, 1, cp, 8, None, 0, None, ht, pn, pm) == capi.CC_OK   # DESCRIPTORS_ONLY needs no record array
    c, r, t = e.take_clusters()                                               # nothing fed: nothing to take, no error
    assert len(c) == 0 and len(r) == 0 and (n.value, m.value) == (0, 0)
    for tab in (t, table):
        assert all((tab[f] == 0).all() for f in ("lost_columns", "first_record", "n_records", "first_cluster", "n_clusters", "error"))
        assert (tab["id_from"] == 1).all() and (tab["id_to"] == 1).all()
    assert e.take_clusters_cursor(0) == (1, 0, 0) and e.take_clusters_size()[:2] == (0, 0)
    e.close()
    e = Engine(cfg, 64, 1)
    e.set_option("resident", 1)
    with pytest.raises(EngineError) as ei:
        e.take_clusters()
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "resident" in str(ei.value)
    e.close()
