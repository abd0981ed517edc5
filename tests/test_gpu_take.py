"""GPU: cc_engine_take_points — the points of the columns published (segmented) since the last take, of all streams, compacted in device
memory. The takes of a run, one after the other, must be the oracle's published columns, return for return; a take that
does not fit must leave everything as it was; columns cleared before anybody took them must be counted, not invented; and taking
between pipelined calls must not disturb the engine."""
import ctypes

import numpy as np
import pytest

import util
from continuous_clustering_amd import capi, synth, take

pytestmark = pytest.mark.gpu

CL, SG = take.TAKE_CLUSTERED, take.TAKE_SEGMENTED
ALL, NOT_GROUND, WITH_ID = take.TAKE_ALL_RETURNS, take.TAKE_NOT_GROUND, take.TAKE_WITH_ID


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


def _same(a, b):
    """bit for bit"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Log:
    """the takes of one (engine, stage): per stream the records with GLOBAL columns, and the checks every single take must pass"""

    def __init__(self, S):
        self.rec = [[] for _ in range(S)]
        self.gcol = [[] for _ in range(S)]
        self.to = [0] * S
        self.started = [False] * S
        self.first = [None] * S  # col_from of a stream's first range that is not empty: must be the stream's first column (_oracle_first_column)

    def add(self, records, table, upper=None):
        rec = _host(records)
        pos = 0
        for s in range(len(self.rec)):
            t = table[s]
            assert t["error"] == 0 and t["lost_columns"] == 0, (s, t)
            assert t["first_record"] == pos and t["n_records"] >= 0, (s, t, pos)   # slices follow each other without a gap
            if upper is not None and upper[s] < 0:                                   # a stream that has not started: nothing, at column 0
                assert (t["col_from"], t["col_to"], t["n_records"]) == (0, 0, 0), (s, t)
            else:
                # the first range of a stream begins at the stream's first column, every other where the previous one ended
                assert t["col_from"] == self.to[s] or (not self.started[s] and t["col_from"] >= 0), (s, t, self.to[s])
                if upper is not None:
                    assert t["col_to"] == upper[s], (s, t, upper[s])
                if not self.started[s] and t["col_to"] > t["col_from"]:
                    self.started[s], self.first[s] = True, int(t["col_from"])
            assert t["col_to"] >= t["col_from"]
            r = rec[pos:pos + int(t["n_records"])]
            pos += int(t["n_records"])
            key = r["column"].astype(np.int64) * 256 + r["row"]
            assert (np.diff(key) > 0).all(), s                                       # strictly increasing in (column, row)
            if len(r):
                assert r["column"].max() < t["col_to"] - t["col_from"], s
            self.rec[s].append(r)
            self.gcol[s].append(r["column"].astype(np.int64) + int(t["col_from"]))
            self.to[s] = int(t["col_to"])
        assert pos == len(rec)

    def of(self, s, below=None):
        r, g = np.concatenate(self.rec[s]), np.concatenate(self.gcol[s])
        if below is not None:
            r, g = r[g < below], g[g < below]
        return r, g


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


def _assert_records_equal(got, got_gcol, ref, ref_gcol, intensity=None, ids=True, what=""):
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert np.array_equal(got_gcol, ref_gcol) and np.array_equal(got["row"], ref["row"]), what
    for f in ("x", "y", "z", "distance"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), (what, f)    # bitwise
    for f in ("ground_point_label", "source_firing") + (("id",) if ids else ()):
        assert np.array_equal(got[f], ref[f]), (what, f)
    if not ids:
        assert (got["id"] == 0).all(), what
    if intensity is not None:
        assert np.array_equal(got["intensity"], intensity[got["source_firing"].astype(np.int64), got["row"]]), what


def _oracle_first_column(o):
    """the first column the reference segmented (its first finished_column_callback_(c, c, true)): where a stream's hand-over must begin"""
    ev = o.drain_events()
    return int(ev[ev["type"] == capi.EV_GROUND_COLUMN]["a"][0])


def _against_oracle(log, s, stream, cfg, n_firings, first_unpublished, ids=True, what=""):
    from oracle.pyoracle import Oracle
    R = stream.sensor.num_rows
    o = Oracle(cfg, R)
    assert o.add_firings(stream.xyz[:n_firings], stream.intensity[:n_firings], stream.poses[:n_firings]) == 0
    assert o.state()["first_unpublished_global_column_index"] == first_unpublished
    got, gcol = log.of(s, below=first_unpublished)
    lo = _oracle_first_column(o)
    assert log.first[s] == lo and 0 <= lo < stream.sensor.num_columns, (what, log.first[s], lo)   # nothing in front was dropped
    ref, ref_gcol = _reference_records(o.read_published(lo, first_unpublished - 1), lo)
    _assert_records_equal(got, gcol, ref, ref_gcol, stream.intensity, ids, what)
    return len(got)


def _run_device(rows, cols, NB, seed, per_call=None, S_nan=True):
    """one rotation per add_firings_device call on a fresh engine (events off); per_call(engine, b) after every call"""
    import torch
    from continuous_clustering_amd import Engine
    streams = _streams(rows, cols, NB, seed, S_nan)
    cfg = _config(rows, cols)
    xyz, inten, poses = _device_inputs(torch, streams, NB, cols)
    e = Engine(cfg, rows, len(streams))
    e.record_events(False)
    for b in range(NB):
        e.add_firings_device(cols, xyz[b], inten[b], poses[b])
        if per_call:
            per_call(e, b)
    assert e.sync() == 0, e.last_error()
    return e, streams, cfg


@pytest.mark.parametrize("rows", [32, 64, 128])
def test_takes_concatenate_to_the_published_columns(rows, oracle_lib):
    """a partial wavefront, a full one, two rows per lane; three streams of which the last never starts; twelve rotations through the ring of ten"""
    cols, NB, S = (256 if rows == 32 else 360), 12, 3
    logs = {CL: Log(S), SG: Log(S)}

    def per_call(e, b):
        for stage, key in ((CL, "first_unpublished_global_column_index"), (SG, "first_unfinished_global_column_index")):
            upper = [e.state(s)[key] for s in range(S)]
            logs[stage].add(*e.take_points(stage, ALL), upper=upper)

    e, streams, cfg = _run_device(rows, cols, NB, 9100 + rows, per_call)
    assert e.state(0)["ring_buffer_start_global_column_index"] > cols    # the ring start has moved: cleared columns lie behind the cursors
    assert sum(len(r) for r in logs[CL].rec[2]) == 0 and e.state(2)["first_unpublished_global_column_index"] < 0
    for s in (0, 1):
        fu = e.state(s)["first_unpublished_global_column_index"]
        assert fu > 10 * cols                                             # every local column has been re-used
        n = _against_oracle(logs[CL], s, streams[s], cfg, NB * cols, fu, what=f"clustered {s}")
        assert n > 0.1 * rows * fu
        assert len(logs[CL].of(s)[0]) == n                                # nothing at or above first_unpublished
        _against_oracle(logs[SG], s, streams[s], cfg, NB * cols, fu, ids=False, what=f"segmented {s}")
        assert logs[SG].to[s] == e.state(s)["first_unfinished_global_column_index"] >= fu
    e.close()


def test_select_filters(oracle_lib):
    """NOT_GROUND and WITH_ID are ALL_RETURNS filtered; three engines fed identically, since a take consumes"""
    rows, cols, NB, S = 64, 360, 3, 3
    got = {}
    for select in (ALL, NOT_GROUND, WITH_ID):
        log, seg = Log(S), Log(S)

        def per_call(e, b):
            log.add(*e.take_points(CL, select))
            if select == NOT_GROUND:                                      # the SEGMENTED stage filters too, with a cursor of its own
                seg.add(*e.take_points(SG, select))

        e, _, _ = _run_device(rows, cols, NB, 9200, per_call)
        if select == NOT_GROUND:
            got["seg"] = [seg.of(s, below=e.state(s)["first_unpublished_global_column_index"]) for s in range(S)]
        got[select] = [log.of(s) for s in range(S)]
        e.close()
    for s in range(S):
        r, g = got[ALL][s]
        for select, keep in ((NOT_GROUND, r["ground_point_label"] != capi.GP_GROUND), (WITH_ID, r["id"] != 0)):
            fr, fg = got[select][s]
            assert _same(fr, r[keep]) and np.array_equal(fg, g[keep]), (s, select)
            if s < 2:
                assert 0 < len(fr) < len(r), (s, select, len(fr), len(r))
        sr, sg_ = got["seg"][s]                                           # the SEGMENTED stage filters on the same labels; its ids are 0
        ref, sr = r[r["ground_point_label"] != capi.GP_GROUND].copy(), sr.copy()
        ref["id"] = 0
        ref["column"] = sr["column"] = 0                                  # (relative to each take's col_from: the global columns are compared below)
        assert _same(sr, ref) and np.array_equal(sg_, g[r["ground_point_label"] != capi.GP_GROUND]), s


def test_invalid_arguments_are_refused():
    import torch
    from continuous_clustering_amd import Engine, EngineError
    cfg = _config(64, 360)
    e = Engine(cfg, 64, 2)
    buf = torch.zeros((16, 32), dtype=torch.uint8, device="cuda")
    L = take._lib()
    table = np.zeros(2, dtype=take.TAKE_STREAM_DTYPE)
    n = ctypes.c_int64(0)
    byref = ctypes.byref
    bad = [(2, ALL, buf.data_ptr(), 8, table.ctypes.data, byref(n)), (-1, ALL, buf.data_ptr(), 8, table.ctypes.data, byref(n)),
           (CL, 3, buf.data_ptr(), 8, table.ctypes.data, byref(n)), (SG, WITH_ID, buf.data_ptr(), 8, table.ctypes.data, byref(n)),
           (CL, ALL, buf.data_ptr() + 8, 8, table.ctypes.data, byref(n)), (CL, ALL, buf.data_ptr(), 8, None, byref(n)),
           (CL, ALL, buf.data_ptr(), 8, table.ctypes.data, None), (CL, ALL, None, 8, table.ctypes.data, byref(n))]
    for stage, select, ptr, cap, ht, pn in bad:
        assert L.cc_engine_take_points(e.h, stage, select, ptr, cap, None, ht, pn) == capi.CC_ERR_INVALID_ARGUMENT, (stage, select)
        assert "cc_engine_take_points" in e.last_error()
    with pytest.raises(ValueError):
        e.take_points(CL, ALL, records=torch.zeros((16, 16), dtype=torch.uint8, device="cuda"))
    r, t = e.take_points(CL, ALL)                                         # nothing fed: nothing to take, no error
    assert len(r) == 0 and (t["n_records"] == 0).all() and (t["col_to"] == 0).all()
    e.close()
    e = Engine(cfg, 64, 1)
    e.set_option("resident", 1)
    with pytest.raises(EngineError) as ei:
        e.take_points(CL, ALL)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "resident" in str(ei.value)
    e.close()


def test_capacity_is_all_or_nothing(oracle_lib):
    import torch
    from continuous_clustering_amd import TakeCapacityError
    rows, cols, NB, S = 64, 360, 3, 3
    e, _, _ = _run_device(rows, cols, NB, 9300)
    fresh, _, _ = _run_device(rows, cols, NB, 9300)
    N, need = e.take_size(CL, ALL)
    assert N > 1000 and need["n_records"].sum() == N
    before = [e.take_cursor(CL, s) for s in range(S)]
    assert all(c == 0 for c, _ in before)
    buf = torch.full((N + 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(TakeCapacityError) as ei:
        e.take_points(CL, ALL, records=buf[:N - 1])
    assert ei.value.code == capi.CC_ERR_CAPACITY and ei.value.needed == N
    assert np.array_equal(ei.value.table, need)
    assert [e.take_cursor(CL, s) for s in range(S)] == before           # no cursor moved
    assert (buf.cpu().numpy() == 0xA5).all()                              # nothing was written, in front of the capacity or behind it
    r, t = e.take_points(CL, ALL, records=buf[:N])
    assert (buf[N:].cpu().numpy() == 0xA5).all()                          # the sentinel behind the capacity
    r2, t2 = fresh.take_points(CL, ALL)
    assert len(r) == N == len(r2) and np.array_equal(t, t2) and np.array_equal(t, need)
    assert np.array_equal(r.cpu().numpy(), r2.cpu().numpy())              # a retry returns what a first call would have, bit for bit
    assert [e.take_cursor(CL, s)[0] for s in range(S)] == [int(x) for x in t["col_to"]]
    assert e.take_size(CL, ALL)[0] == 0
    e.close()
    fresh.close()


def test_columns_cleared_before_a_take_are_reported_lost():
    rows, cols, S = 32, 256, 2
    import torch
    from continuous_clustering_amd import Engine
    NB = 14
    streams = _streams(rows, cols, NB, 9400, nan_last=False)
    xyz, inten, poses = _device_inputs(torch, streams, NB, cols)
    e = Engine(_config(rows, cols), rows, S)
    e.record_events(False)
    fed = 0
    while fed < NB and min(e.take_cursor(CL, s)[1] for s in range(S)) <= 0:
        e.add_firings_device(cols, xyz[fed], inten[fed], poses[fed])
        fed += 1
    readable = [e.take_cursor(CL, s) for s in range(S)]
    assert all(c == 0 and lo > 0 for c, lo in readable), (fed, readable)  # nobody took anything while the ring went round
    records, table = e.take_points(CL, ALL)
    rec = _host(records)
    for s in range(S):
        t = table[s]
        assert t["lost_columns"] == readable[s][1] - 0 and t["col_from"] == readable[s][1], (s, t, readable[s])
        assert t["col_to"] == e.state(s)["first_unpublished_global_column_index"]
        assert 0 < t["col_to"] - t["col_from"] <= 10 * cols
        got = rec[int(t["first_record"]):int(t["first_record"] + t["n_records"])]
        ref, ref_gcol = _reference_records(e.read_columns(int(t["col_from"]), int(t["col_to"]) - 1, stream=s), int(t["col_from"]))
        _assert_records_equal(got, got["column"].astype(np.int64) + int(t["col_from"]), ref, ref_gcol, streams[s].intensity, what=f"stream {s}")
        assert len(got) > 0
    _, again = e.take_points(CL, ALL)                                     # taken: nothing new, nothing lost
    assert (again["n_records"] == 0).all() and (again["lost_columns"] == 0).all() and (again["col_from"] == again["col_to"]).all()
    e.take_seek(int(table[1]["col_from"]), stage=CL, stream=1)            # back to where stream 1's range began: the same records again
    assert e.take_cursor(CL, 1)[0] == table[1]["col_from"] and e.take_cursor(CL, 0)[0] == table[0]["col_to"]
    records2, table2 = e.take_points(CL, ALL)
    assert table2[0]["n_records"] == 0 and table2[1]["first_record"] == 0 and table2[1]["lost_columns"] == 0
    assert all(table2[1][k] == table[1][k] for k in ("col_from", "col_to", "n_records"))
    assert _same(_host(records2), rec[int(table[1]["first_record"]):int(table[1]["first_record"] + table[1]["n_records"])])
    e.close()


def test_take_after_small_calls_and_reset(oracle_lib):
    """one stream on the host path, events on: calls of 97 firings and of 7 (the one-launch path of calls below 64 firings)"""
    from continuous_clustering_amd import Engine
    rows, cols = 64, 360
    stream = synth.make_stream(cols * 3, seed=9500, sensor=_sensor(rows, cols), motion=synth.Motion.translate())
    cfg = _config(rows, cols)
    e = Engine(cfg, rows)
    runs = []
    for run in range(2):
        assert e.take_cursor(CL, 0)[0] == 0 and e.take_cursor(SG, 0)[0] == 0
        log, seg = Log(1), Log(1)
        f, i = 0, 0
        while f < stream.n_firings:
            m = min((97, 7)[i % 2], stream.n_firings - f)
            assert e.add_firings(stream.xyz[f:f + m], stream.intensity[f:f + m], stream.poses[f:f + m]) == 0, e.last_error()
            f += m
            i += 1
            st = e.state()
            log.add(*e.take_points(CL, ALL), upper=[st["first_unpublished_global_column_index"]])
            if i % 3 == 0:
                seg.add(*e.take_points(SG, ALL), upper=[st["first_unfinished_global_column_index"]])
        seg.add(*e.take_points(SG, ALL))
        fu = e.state()["first_unpublished_global_column_index"]
        if run == 0:
            _against_oracle(log, 0, stream, cfg, stream.n_firings, fu, what="clustered")
            _against_oracle(seg, 0, stream, cfg, stream.n_firings, fu, ids=False, what="segmented")
        runs.append(log.of(0))
        assert e.take_cursor(CL, 0)[0] == fu
        e.reset()
        e.set_robot_from_sensor(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64))
    assert _same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    e.close()


@pytest.mark.parametrize("pipeline", [0, 2])
def test_take_between_pipelined_calls(pipeline, oracle_lib):
    """the configuration of test_pipelined_throughput_path_matches_oracle with a take after every call: the engine ends where the oracle does"""
    import torch
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    sen = synth.SensorModel(num_rows=64, num_columns=720)
    cfg = capi.Config.kitti()
    cfg.num_columns = 720
    S, F, NB = 8, 720, 5
    motions = [synth.Motion.static(), synth.Motion.translate(), synth.Motion.turn()]
    streams = [synth.make_stream(F * NB, seed=300 + s, sensor=sen, motion=motions[s % 3]) for s in range(S)]
    xyz, inten, poses = _device_inputs(torch, streams, NB, F)
    e = Engine(cfg, 64, S)
    e.record_events(False)
    e.set_option("pipeline", pipeline)
    log = Log(S)
    d_table = torch.zeros(S * 48, dtype=torch.uint8, device="cuda")
    for b in range(NB):
        e.add_firings_device(F, xyz[b], inten[b], poses[b])
        records, table = e.take_points(CL, ALL, d_table=d_table)
        assert np.array_equal(d_table.cpu().numpy().view(take.TAKE_STREAM_DTYPE), table)   # the device copy of the table
        log.add(records, table)
    assert e.sync() == 0, e.last_error()
    for s in range(S):
        o = Oracle(cfg, 64)
        assert o.add_firings(streams[s].xyz, streams[s].intensity, streams[s].poses) == 0
        so, se = o.state(), e.state(s)
        for k in util.STATE_FIELDS:
            assert so[k] == se[k], (s, k)
        hi = se["first_unpublished_global_column_index"] - 1
        lo = max(hi - 600, se["ring_buffer_start_global_column_index"])
        util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo, mirror=False)
        got, gcol = log.of(s)
        assert log.to[s] == hi + 1
        first = _oracle_first_column(o)
        assert log.first[s] == first == 0, (s, log.first[s], first)       # (start_column 0: the hand-over begins at column 0)
        ref, ref_gcol = _reference_records(o.read_published(first, hi), first)
        _assert_records_equal(got, gcol, ref, ref_gcol, streams[s].intensity, what=f"stream {s}")
    e.close()
