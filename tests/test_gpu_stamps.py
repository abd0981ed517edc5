"""GPU: the firing-stamp log and its three resolve calls (include/cc_stamps.h).
A. synthetic records against the host twins and the plain-Python model of tests/stamp_cases.py, bit for bit;
B. behind a real engine: every taken point, column, stream and cluster stamp against numpy over the host copy of the same records,
   stamps[stream][source_firing] and then the reference's rules; the engine must not notice the stamp calls;
C. fed by cc_pose_tracks_sweep's d_stamps on one HIP stream, through a reset of one stream;
D. refusals: nothing launched, a text in last_error."""
import numpy as np
import pytest

import stamp_cases as sc
from continuous_clustering_amd import EngineError, capi, poses, stamps, synth, take

pytestmark = pytest.mark.gpu

M64 = np.uint64(sc.M64)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    """a numpy array (structured or not) as a uint8 CUDA tensor [n, itemsize]"""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8).reshape(-1, a.dtype.itemsize).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _u64(t):
    return t.cpu().numpy().reshape(-1).view(np.uint64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _cl(t):
    return t.cpu().numpy().reshape(-1).view(stamps.CLUSTER_STAMP_DTYPE)


def _missing(log, S):
    return [log.counters(s)[1] for s in range(S)]


def _resolve_points(fs, rec, table):
    out, sn = fs.of_points(_dev(rec), _dev(table))
    fs.sync()
    return _u64(out), _u32(sn)


def _resolve_columns(fs, rec, table):
    cols, streams = fs.of_columns(_dev(rec), _dev(table), table)
    fs.sync()
    return _u64(cols), _u64(streams)


def _resolve_clusters(fs, cl, rec, last):
    out, pts = fs.of_clusters(_dev(cl), _dev(rec), last, with_point_stamps=True)
    fs.sync()
    return _cl(out), _u64(pts)


@pytest.fixture(scope="module")
def synthetic():
    """(device log, host twin, model), filled alike"""
    fs = sc.fill_log(stamps.FiringStamps(sc.S, sc.CAPACITY))
    yield fs, sc.fill_log(stamps.HostFiringStamps(sc.S, sc.CAPACITY)), sc.fill_log(sc.ModelLog(sc.S, sc.CAPACITY))
    fs.close()


# ---- A ----------------------------------------------------------------------------------------------------------------------------------------
def test_heads_after_filling(synthetic):
    fs, twin, model = synthetic
    assert fs.capacity == 1024
    heads = [fs.counters(s)[0] for s in range(sc.S)]
    assert heads == [twin.counters(s)[0] for s in range(sc.S)] == [model.counters(s)[0] for s in range(sc.S)]
    assert heads == [3000, 0, (1 << 32) + 500, 77, 16]


def test_points_and_columns_of_synthetic_records(synthetic):
    """ring wrap, 2^32, streams with empty slices, columns without a record / with only zeros / with zeros among stamps"""
    fs, twin, model = synthetic
    rec, table = sc.point_case()
    before = [_missing(log, sc.S) for log in (fs, twin, model)]
    got, got_sn = _resolve_points(fs, rec, table)
    ref, ref_sn = twin.of_points(rec, table)
    mod, mod_sn = sc.model_of_points(model, rec, table)
    assert sc.same(got, ref) and sc.same(got_sn, ref_sn) and sc.same(got, mod) and sc.same(got_sn, mod_sn)
    assert list(got[:4]) == [0, ref[1], ref[2], 0] and ref[1] != 0 and ref[2] != 0        # firings 1975, 1976, 2999, 3000 of stream 0
    cols, streams = _resolve_columns(fs, rec, table)
    ref_cols, ref_streams = twin.of_columns(rec, table)
    mod_cols, mod_streams = sc.model_of_columns(model, rec, table)
    assert sc.same(cols, ref_cols) and sc.same(streams, ref_streams) and sc.same(cols, mod_cols) and sc.same(streams, mod_streams)
    assert len(cols) == 26 and cols[22] == 0 and cols[23] >= sc.EARLIEST and cols[24] == 0 and cols[25] == 1
    again, again_sn = _resolve_points(fs, rec, table)                                      # the same call twice: identical bytes
    again_cols, again_streams = _resolve_columns(fs, rec, table)
    assert sc.same(again, got) and sc.same(again_sn, got_sn) and sc.same(again_cols, cols) and sc.same(again_streams, streams)
    for _ in range(2):
        twin.of_points(rec, table)                                                         # (every resolve call counts what it resolves)
        sc.model_of_points(model, rec, table)
    lost = [[a - b for a, b in zip(_missing(log, sc.S), was)] for log, was in zip((fs, twin, model), before)]
    assert lost[0] == lost[1] == lost[2] and lost[0][0] > 0 and lost[0][2] > 0 and lost[0][1] == lost[0][3] == lost[0][4] == 0


def test_clusters_of_1_to_70001_points_in_one_call(synthetic):
    """sizes 1, 63, 64, 70 001, 65, 4097 (the largest in the middle) and the uint64 edge cases of the midpoint"""
    fs, twin, model = synthetic
    cl, rec = sc.cluster_case()
    assert tuple(cl["n_points"][:6]) == sc.CLUSTER_SIZES
    before = _missing(fs, sc.S)
    for last in (True, False):
        got, got_pts = _resolve_clusters(fs, cl, rec, last)
        ref, ref_pts = twin.of_clusters(cl, rec, last)
        mod, mod_pts = sc.model_of_clusters(model, cl, rec, last)
        assert sc.same(got, ref) and sc.same(got_pts, ref_pts), last
        assert sc.same(got, mod) and sc.same(got_pts, mod_pts), last
    again, again_pts = _resolve_clusters(fs, cl, rec, False)
    assert sc.same(again, got) and sc.same(again_pts, got_pts)
    sp = got[len(sc.CLUSTER_SIZES):]
    assert (int(sp["min_stamp"][3]), int(sp["max_stamp"][3]), int(sp["stamp"][3])) == (1, sc.M64, 1 << 63)
    assert int(sp["stamp"][0]) == (1 << 63) + 11 and sp["min_stamp"][4] == 0 and sp["n_missing"][4] == 0
    assert got["n_missing"][3] > 0 and got["n_missing"][0] == 0
    lost = [int(got["n_missing"][cl["stream"] == s].sum()) for s in range(sc.S)]
    assert [a - b for a, b in zip(_missing(fs, sc.S), before)] == [3 * n for n in lost] and lost[0] > 0 and lost[2] > 0 and lost[4] == 0


def test_nothing_to_resolve_and_nothing_pushed():
    import torch
    fs, twin = stamps.FiringStamps(2, 64), stamps.HostFiringStamps(2, 64)
    table = np.zeros(2, dtype=take.TAKE_STREAM_DTYPE)
    d_table, none = _dev(table), torch.empty((0, 32), dtype=torch.uint8, device="cuda")
    sentinel = torch.full((4, 32), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert fs.of_points_raw(0, none, d_table, sentinel, None) == 0
    assert fs.of_clusters_raw(0, 0, None, 0, None, sentinel, None) == 0
    assert fs.of_clusters_raw(0, 0, None, 3, sentinel, sentinel, None) == 0                # records, but no cluster to stamp
    assert fs.of_columns_raw(0, None, d_table, table, sentinel, None) == 0                 # no column in the table, no stream output
    fs.sync()
    assert (sentinel.cpu().numpy() == 0xA5).all()
    cols, streams = fs.of_columns(none, d_table, table)
    fs.sync()
    assert len(cols) == 0 and not _u64(streams).any()
    rec = np.zeros(3, dtype=take.TAKE_POINT_DTYPE)                                         # head == 0: every firing is missing
    rec["source_firing"] = [0, 1, sc.M32]
    table[0]["n_records"], table[0]["col_to"], table[1]["first_record"] = 3, 2, 3
    got, sn = _resolve_points(fs, rec, table)
    assert not got.any() and not sn.any() and fs.counters(0) == (0, 3) and fs.counters(1) == (0, 0)
    cols, streams = _resolve_columns(fs, rec, table)
    assert len(cols) == 2 and not cols.any() and not streams.any() and fs.counters(0) == (0, 6)
    cl = np.zeros(1, dtype=take.TAKE_CLUSTER_DTYPE)
    cl["n_points"] = 3
    got, _ = _resolve_clusters(fs, cl, rec, False)
    assert sc.same(got, twin.of_clusters(cl, rec, False)[0]) and tuple(got[0]) == (0, 0, 0, 3, 0)
    fs.close()


@pytest.mark.parametrize("repeat", [3, 16])
def test_push_with_repeat_is_push_host_of_the_expanded_array(repeat):
    S, n = 3, 40
    rng = np.random.default_rng(repeat)
    st = sc.jittered(rng, S * n).reshape(S, n)
    a, b = stamps.FiringStamps(S, 1000), stamps.FiringStamps(S, 1000)
    a.seek(1, 12345)
    b.seek(1, 12345)
    a.push(n, _dev(st), repeat)
    for s in range(S):
        b.push_host(s, np.repeat(st[s], repeat))
    rec = np.zeros(S * n * repeat, dtype=take.TAKE_POINT_DTYPE)
    table = np.zeros(S, dtype=take.TAKE_STREAM_DTYPE)
    for s in range(S):
        table[s]["first_record"], table[s]["n_records"] = s * n * repeat, n * repeat
        rec["source_firing"][s * n * repeat:(s + 1) * n * repeat] = np.arange(n * repeat) + (12345 if s == 1 else 0)
    got_a, _ = _resolve_points(a, rec, table)
    got_b, _ = _resolve_points(b, rec, table)
    assert sc.same(got_a, np.repeat(st, repeat, axis=1).reshape(-1)) and sc.same(got_b, got_a)
    assert [a.counters(s) for s in range(S)] == [b.counters(s) for s in range(S)] == [(n * repeat, 0), (12345 + n * repeat, 0), (n * repeat, 0)]
    a.close()
    b.close()


def test_reset_of_one_stream_leaves_the_others():
    rec, table = sc.point_case()
    fs2, twin2 = sc.fill_log(stamps.FiringStamps(sc.S, sc.CAPACITY)), sc.fill_log(stamps.HostFiringStamps(sc.S, sc.CAPACITY))
    before, _ = _resolve_points(fs2, rec, table)
    twin2.of_points(rec, table)
    fs2.reset_streams(2)
    twin2.reset_streams(2)
    assert fs2.counters(2) == (0, 0) and fs2.counters(0)[0] == 3000 and fs2.counters(0)[1] > 0
    after, _ = _resolve_points(fs2, rec, table)
    mine = slice(int(table[2]["first_record"]), int(table[2]["first_record"] + table[2]["n_records"]))
    expect = before.copy()
    expect[mine] = 0
    assert sc.same(after, expect) and before[mine].any() and sc.same(after, twin2.of_points(rec, table)[0])
    assert _missing(fs2, sc.S) == _missing(twin2, sc.S) and fs2.counters(2) == (0, 200)
    fs2.push_host(2, [5, 6, 7])                                                            # the stream counts from 0 again
    rec["source_firing"][mine] = 1
    assert (_resolve_points(fs2, rec, table)[0][mine] == 6).all()
    fs2.close()


def test_more_streams_than_the_staged_table_holds():
    """1100 streams: the slices' first records are searched in global memory (above 1024 streams nothing is staged in LDS) and the column
    offsets are summed over more than one pass of 256; every third stream has an empty slice"""
    S, per = 1100, 5
    rng = np.random.default_rng(3)
    fs, twin = stamps.FiringStamps(S, 64), stamps.HostFiringStamps(S, 64)
    st = sc.jittered(rng, S * 40).reshape(S, 40)
    fs.push(40, _dev(st))
    twin.push(st)
    counts = np.where(np.arange(S) % 3 == 1, 0, per)
    table = np.zeros(S, dtype=take.TAKE_STREAM_DTYPE)
    table["n_records"], table["first_record"] = counts, np.concatenate([[0], np.cumsum(counts)[:-1]])
    table["col_from"] = np.arange(S) * 7
    table["col_to"] = table["col_from"] + np.arange(S) % 4                                 # 0 to 3 columns
    rec = np.zeros(int(counts.sum()), dtype=take.TAKE_POINT_DTYPE)
    rec["source_firing"] = rng.integers(0, 44, len(rec))                                   # 40 .. 43 are not pushed yet
    rec["column"] = np.sort(rng.integers(0, 3, (len(rec) // per, per)), axis=1).reshape(-1)   # some lie beyond their stream's columns
    got, got_sn = _resolve_points(fs, rec, table)
    ref, ref_sn = twin.of_points(rec, table)
    assert sc.same(got, ref) and sc.same(got_sn, ref_sn) and (got == 0).any() and (got != 0).any()
    cols, streams = _resolve_columns(fs, rec, table)
    ref_cols, ref_streams = twin.of_columns(rec, table)
    assert sc.same(cols, ref_cols) and sc.same(streams, ref_streams) and len(cols) == int((np.arange(S) % 4).sum()) and cols.any()
    assert _missing(fs, S) == _missing(twin, S) and sum(_missing(fs, S)) > 0
    fs.close()


def test_descriptors_without_members_between_clusters():
    """300 descriptors with n_points = 0 between two clusters: more than the 257 a block stages next to its first record"""
    fs, twin = sc.fill_log(stamps.FiringStamps(sc.S, sc.CAPACITY)), sc.fill_log(stamps.HostFiringStamps(sc.S, sc.CAPACITY))
    rng = np.random.default_rng(4)
    sizes = [10] + [0] * 300 + [500, 0, 3]
    cl = np.zeros(len(sizes), dtype=take.TAKE_CLUSTER_DTYPE)
    cl["n_points"], cl["first_record"] = sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]])
    cl["stream"] = 2
    cl["stream"][:5] = 0
    rec = np.zeros(sum(sizes), dtype=take.TAKE_POINT_DTYPE)
    rec["source_firing"][:10] = rng.integers(1976, 3000, 10)
    rec["source_firing"][10:] = (sc.SEEK_AT + rng.integers(0, 1000, len(rec) - 10)) & sc.M32
    for last in (False, True):
        got, got_pts = _resolve_clusters(fs, cl, rec, last)
        ref, ref_pts = twin.of_clusters(cl, rec, last)
        assert sc.same(got, ref) and sc.same(got_pts, ref_pts), last
    assert not got[1:301].tobytes().strip(b"\0") and got["min_stamp"][301] >= sc.EARLIEST and got["n_missing"].sum() == 0
    fs.close()


# ---- B ----------------------------------------------------------------------------------------------------------------------------------------
def _sensor(rows, cols):
    if rows == 128:
        sen = synth.SensorModel.s128()
        sen.num_columns = cols
        return sen
    return synth.SensorModel(num_rows=rows, num_columns=cols)


def _config(rows, cols):
    cfg = capi.Config.vls128() if rows == 128 else capi.Config.kitti()
    cfg.num_columns = cols
    return cfg


def _streams(rows, cols, rotations, seed):
    """static, turning, and one without a single return, which never starts"""
    sen = _sensor(rows, cols)
    start = 16 if rows == 128 else 0
    out = [synth.make_stream(cols * rotations, seed=seed, sensor=sen, motion=synth.Motion.static(), start_column=start),
           synth.make_stream(cols * rotations, seed=seed + 1, sensor=sen, motion=synth.Motion.turn(), start_column=start)]
    out.append(synth.Stream(xyz=np.full_like(out[0].xyz, np.nan), intensity=out[0].intensity, poses=out[0].poses, sensor=sen))
    return out


def _firing_stamps(S, n, cols, seed):
    """[S][n] around 1.7e18 ns with jitter; inside rotation 3 a step back of 50 ms; firing 1000 of every stream is stamped 0"""
    rng = np.random.default_rng(seed)
    st = np.stack([sc.jittered(rng, n) for _ in range(S)])
    st[:, 3 * cols + cols // 2:] -= np.uint64(50_000_000)
    st[:, 1000] = 0
    return st


def _expected_columns(pt, rec, table):
    """ros_utils.cpp:51-71 over the host copy: per column and per stream the minimum non-zero stamp, else 0"""
    width = np.maximum(table["col_to"] - table["col_from"], 0)
    offset = np.concatenate([[0], np.cumsum(width)])
    cols, streams = np.full(int(offset[-1]), M64), np.full(len(table), M64)
    for s in range(len(table)):
        a, n = int(table[s]["first_record"]), int(table[s]["n_records"])
        v, c = pt[a:a + n], rec["column"][a:a + n].astype(np.int64) + offset[s]
        np.minimum.at(cols, c[v != 0], v[v != 0])
        if (v != 0).any():
            streams[s] = v[v != 0].min()
    cols[cols == M64], streams[streams == M64] = 0, 0
    return cols, streams


def _expected_clusters(pt, cl, last):
    """cc.cpp:1007-1010, 1025-1028 over the host copy (clusters abut in the record array)"""
    out = np.zeros(len(cl), dtype=stamps.CLUSTER_STAMP_DTYPE)
    if len(cl):
        first = cl["first_record"].astype(np.int64)
        out["min_stamp"], out["max_stamp"] = np.minimum.reduceat(pt, first), np.maximum.reduceat(pt, first)
        out["stamp"] = out["max_stamp"] if last else out["min_stamp"] + (out["max_stamp"] - out["min_stamp"]) // np.uint64(2)
    return out


def _host(t, dtype):
    return t.cpu().numpy().reshape(-1).view(dtype)


def _run(streams, cfg, NB, st=None, capacity=0, lag=0):
    """one rotation per call; with `st`, push + take_clusters(6) + of_clusters + take_points + of_points + of_columns after every call and
    compare (lag = 1: a take's records are resolved one rotation late, behind the next call's push, as a consumer does that works on the
    previous hand-over while the next rotation runs); returns what describes the engine afterwards, the bytes of every take, the log's
    missing counts and what was checked"""
    import torch
    from continuous_clustering_amd import Engine
    rows, cols, S = streams[0].sensor.num_rows, streams[0].sensor.num_columns, len(streams)
    xyz = torch.from_numpy(np.stack([s.xyz[:NB * cols].reshape(NB, cols, rows, 3) for s in streams], axis=1)).cuda()
    inten = torch.from_numpy(np.stack([s.intensity[:NB * cols].reshape(NB, cols, rows) for s in streams], axis=1)).cuda()
    pose = torch.from_numpy(np.stack([s.poses[:NB * cols].reshape(NB, cols, 12) for s in streams], axis=1)).cuda()
    d_st = None if st is None else [torch.from_numpy(st[:, b * cols:(b + 1) * cols].copy().view(np.int64)).cuda() for b in range(NB)]
    d_ctable = torch.zeros(S * 56, dtype=torch.uint8, device="cuda")
    d_ptables = [torch.zeros(S * 48, dtype=torch.uint8, device="cuda") for _ in range(NB)]   # a resolve may run a call after its take
    torch.cuda.synchronize()
    e = Engine(cfg, rows, S)
    e.record_events(False)
    fs = stamps.FiringStamps(S, capacity) if st is not None else None
    takes, checked = [], {"points": 0, "clusters": 0, "columns": 0, "zero": 0}

    def resolve_and_compare(b, clusters, crec, ctable, records, ptable, d_ptable):
        held = capacity >= 4096
        cl, cr = _host(clusters, take.TAKE_CLUSTER_DTYPE), _host(crec, take.TAKE_POINT_DTYPE)
        pr = _host(records, take.TAKE_POINT_DTYPE)
        assert ptable["n_records"][2] == 0 and ctable["n_clusters"][2] == 0 and (cl["stream"] != 2).all()   # the stream that never starts
        # clusters: stamps[stream][source_firing], then the rule
        of_cluster = np.repeat(cl["stream"], cl["n_points"])
        expect_pts = st[of_cluster, cr["source_firing"]] if held else None
        for last in (False, True):
            out, pts = fs.of_clusters(clusters, crec, last, with_point_stamps=True)
            fs.sync()
            got, got_pts = _host(out, stamps.CLUSTER_STAMP_DTYPE), _u64(pts)
            if held:
                assert sc.same(got_pts, expect_pts), (b, last)
                assert sc.same(got, _expected_clusters(expect_pts, cl, last)), (b, last)
            else:
                assert sc.same(got_pts[got_pts != 0], st[of_cluster, cr["source_firing"]][got_pts != 0])   # what is held is right
                assert len(cl) == 0 or (got["n_missing"] <= np.add.reduceat((got_pts == 0).astype(np.uint32), cl["first_record"])).all()
        checked["clusters"] += len(cl)
        # points and columns
        of_point = np.repeat(np.arange(S), ptable["n_records"])
        out, sn = fs.of_points(records, d_ptable)
        cols_t, streams_t = fs.of_columns(records, d_ptable, ptable)
        fs.sync()
        got, got_sn, got_cols, got_streams = _u64(out), _u32(sn), _u64(cols_t), _u64(streams_t)
        if held:
            expect = st[of_point, pr["source_firing"]]
            assert sc.same(got, expect), b
            assert sc.same(got_sn, np.stack([(expect // np.uint64(10 ** 9)).astype(np.uint32), (expect % np.uint64(10 ** 9)).astype(np.uint32)], axis=1))
            exp_cols, exp_streams = _expected_columns(expect, pr, ptable)
            assert sc.same(got_cols, exp_cols) and sc.same(got_streams, exp_streams), b
            assert got_streams[2] == 0
            checked["zero"] += int((expect == 0).sum())
        else:
            checked["zero"] += int((got == 0).sum())
        checked["points"] += len(pr)
        checked["columns"] += len(got_cols)

    pending = None
    for b in range(NB):
        e.add_firings_device(cols, xyz[b], inten[b], pose[b])
        if fs:
            fs.push(cols, d_st[b])
        if pending:
            resolve_and_compare(*pending)
        clusters, crec, ctable = e.take_clusters(6, d_table=d_ctable)
        records, ptable = e.take_points(d_table=d_ptables[b])
        takes.append((clusters.cpu().numpy().tobytes(), crec.cpu().numpy().tobytes(), ctable.tobytes(), records.cpu().numpy().tobytes(),
                      ptable.tobytes()))
        pending = (b, clusters, crec, ctable, records, ptable, d_ptables[b]) if fs and lag else None
        if fs and not lag:
            resolve_and_compare(b, clusters, crec, ctable, records, ptable, d_ptables[b])
    assert e.sync() == 0, e.last_error()
    state = ([e.state(s) for s in range(S)], [e.take_cursor(take.TAKE_CLUSTERED, s) for s in range(S)], [e.take_clusters_cursor(s) for s in range(S)])
    lost = _missing(fs, S) if fs else None
    if fs:
        assert [fs.counters(s)[0] for s in range(S)] == [NB * cols] * S
        fs.close()
    e.close()
    return state, takes, lost, checked


@pytest.mark.parametrize("rows", [64, 128])
def test_stamps_behind_an_engine(rows):
    """three streams (static, turning, never starting), 360 columns, twelve rotations through the ring of ten"""
    cols, NB, S = 360, 12, 3
    streams, cfg = _streams(rows, cols, NB, 9600 + rows), _config(rows, cols)
    st = _firing_stamps(S, NB * cols, cols, rows)
    plain = _run(streams, cfg, NB)
    state, takes, lost, checked = _run(streams, cfg, NB, st, capacity=8192)
    print(f"rows {rows}: {checked}")
    assert lost == [0, 0, 0] and checked["points"] > 100_000 and checked["clusters"] >= 100 and checked["columns"] > 2 * 10 * cols
    assert checked["zero"] >= 2                                       # the firing stamped 0 came through, in both streams that run
    assert state == plain[0] and takes == plain[1]                    # the engine and both take cursors did not notice the stamp calls


def test_a_log_of_512_firings_reports_missing():
    """a log of capacity 512 is smaller than one rotation of lag needs: with every take resolved one rotation late, behind the next call's
    push, its records reach up to 360 + 370 firings behind the head (370: the oldest record of a take at its own time, measured with the
    CPU oracle at this shape); the older part has left the log, resolves to 0 and is counted, what is still held is right, and neither the
    engine nor the takes notice. Resolved at once, behind its own call's push, the same log loses nothing (the 8192-slot run above)."""
    cols, NB, S = 360, 12, 3
    streams, cfg = _streams(64, cols, NB, 9664), _config(64, cols)
    st = _firing_stamps(S, NB * cols, cols, 64)
    plain = _run(streams, cfg, NB)
    _, takes, lost, seen = _run(streams, cfg, NB, st, capacity=512, lag=1)
    print(f"capacity 512, resolved one rotation late: missing {lost}, zero stamps among {seen['points']} points: {seen['zero']}")
    assert takes == plain[1] and lost[0] > 0 and lost[1] > 0 and lost[2] == 0 and seen["zero"] > 118   # (118: the firing stamped 0 alone)


# ---- C ----------------------------------------------------------------------------------------------------------------------------------------
def test_stamps_from_a_pose_sweep_and_a_reset_in_the_middle():
    """d_stamps of cc_pose_tracks_sweep go straight into push on the same HIP stream; stream 1 is reset after the third rotation"""
    import torch
    from continuous_clustering_amd import Engine, IDENTITY_TF
    rows, cols, NB, S = 64, 360, 6, 2
    streams, cfg = _streams(rows, cols, NB, 9700)[:2], _config(rows, cols)
    xyz = torch.from_numpy(np.stack([s.xyz[:NB * cols].reshape(NB, cols, rows, 3) for s in streams], axis=1)).cuda()
    inten = torch.from_numpy(np.stack([s.intensity[:NB * cols].reshape(NB, cols, rows) for s in streams], axis=1)).cuda()
    pose = torch.from_numpy(np.stack([s.poses[:NB * cols].reshape(NB, cols, 12) for s in streams], axis=1)).cuda()
    t_stamps = (sc.BASE + np.arange(8, dtype=np.uint64) * np.uint64(100_000_000))                       # 10 Hz odometry, identity poses
    t_poses = np.tile(np.asarray(IDENTITY_TF, dtype=np.float64), (8, 1))
    d_poses = torch.empty((S, cols, 12), dtype=torch.float64, device="cuda")
    d_stamps = torch.empty((S, cols), dtype=torch.int64, device="cuda")
    d_table = torch.zeros(S * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tracks = poses.PoseTracks(S, 8)
    fs = stamps.FiringStamps(S, 8192, hip_stream=tracks.hip_stream())
    assert fs.hip_stream() == tracks.hip_stream()
    e = Engine(cfg, rows, S)
    e.record_events(False)
    for s in range(S):
        tracks.set(s, t_stamps, t_poses)
    known, checked = [[], []], [[0, 0], [0, 0]]                                                         # per stream: before / after the reset
    for b in range(NB):
        start = [sc.BASE + b * 100_000_000 + 7 * s for s in range(S)]
        end = [v + 99_954_321 for v in start]
        tracks.sweep(cols, start, end, d_poses, d_stamps=d_stamps)
        fs.push(cols, d_stamps)                                                                          # no host copy, no wait
        for s in range(S):
            known[s].append(poses.host_sweep(t_stamps, t_poses, cols, start[s], end[s])[0])
        e.add_firings_device(cols, xyz[b], inten[b], pose[b])
        records, table = e.take_points(d_table=d_table)
        out, _ = fs.of_points(records, d_table, with_sec_nsec=False)
        fs.sync()
        got, pr = _u64(out), _host(records, take.TAKE_POINT_DTYPE)
        for s in range(S):
            a, n = int(table[s]["first_record"]), int(table[s]["n_records"])
            assert sc.same(got[a:a + n], np.concatenate(known[s])[pr["source_firing"][a:a + n]]), (b, s)
            checked[s][b >= 3] += n
        if b == 2:
            e.reset_streams(1)
            e.set_robot_from_sensor(IDENTITY_TF, stream=1)
            fs.reset_streams(1)
            known[1] = []                                                                                # stream 1 counts its firings from 0 again
    assert fs.counters(0) == (NB * cols, 0) and fs.counters(1) == (3 * cols, 0)
    assert all(n > 10_000 for pair in checked for n in pair), checked
    fs.close()
    tracks.close()
    e.close()


# ---- D ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    import torch
    fs = stamps.FiringStamps(2, 64)
    rec, table = np.zeros(4, dtype=take.TAKE_POINT_DTYPE), np.zeros(2, dtype=take.TAKE_STREAM_DTYPE)
    table[0]["n_records"], table[0]["col_to"], table[1]["first_record"] = 4, 2, 4
    cl = np.zeros(1, dtype=take.TAKE_CLUSTER_DTYPE)
    cl["n_points"] = 4
    d_rec, d_table, d_cl = _dev(np.concatenate([rec, rec])), _dev(table), _dev(cl)
    out = torch.full((8, 32), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros((2, 65), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bad = capi.CC_ERR_INVALID_ARGUMENT

    def refused(rc, *words):
        assert rc == bad and all(w in stamps.last_error() for w in words), (rc, stamps.last_error())

    refused(fs.of_points_raw(4, d_rec.data_ptr() + 8, d_table, out), "cc_firing_stamps_of_points", "misaligned")
    refused(fs.of_columns_raw(4, d_rec.data_ptr() + 8, d_table, table, out, None), "cc_firing_stamps_of_columns", "misaligned")
    refused(fs.of_clusters_raw(0, 1, d_cl, 4, d_rec.data_ptr() + 8, out), "cc_firing_stamps_of_clusters", "misaligned")
    refused(fs.push_raw(65, d_st, 1), "cc_firing_stamps_push", "capacity")
    refused(fs.push_raw(22, d_st, 3), "cc_firing_stamps_push", "capacity")
    refused(fs.push_raw(0, d_st, 1), "cc_firing_stamps_push")
    refused(fs.push_raw(4, None, 1), "cc_firing_stamps_push", "d_stamps")
    refused(fs.of_points_raw(4, d_rec, None, out), "cc_firing_stamps_of_points", "d_table")
    refused(fs.of_columns_raw(4, d_rec, None, table, out, None), "cc_firing_stamps_of_columns", "d_table")
    refused(fs.of_clusters_raw(0, 1, d_cl, 4, None, out), "cc_firing_stamps_of_clusters", "stamps need the records")
    refused(fs.of_points_raw(4, None, d_table, out), "cc_firing_stamps_of_points", "d_records")
    for call, name in ((lambda: fs.push_host(2, [1]), "cc_firing_stamps_push_host"), (lambda: fs.push_host(-1, [1]), "cc_firing_stamps_push_host"),
                       (lambda: fs.seek(2, 0), "cc_firing_stamps_seek"), (lambda: fs.reset_streams([0, 2]), "cc_firing_stamps_reset_streams"),
                       (lambda: fs.counters(2), "cc_firing_stamps_counters"), (lambda: fs.push_host(0, np.zeros(65, dtype=np.uint64)), "capacity")):
        with pytest.raises(EngineError) as err:
            call()
        assert err.value.code == bad and name in str(err.value), name
    fs.sync()
    assert (out.cpu().numpy() == 0xA5).all() and fs.counters(0) == (0, 0) and fs.counters(1) == (0, 0)
    assert fs.push_raw(64, d_st, 1) == 0 and fs.push_raw(21, d_st, 3) == 0 and fs.counters(1) == (127, 0)   # what just fits is taken
    fs.close()
