"""GPU: cc_engine_reset_streams — reset(num_rows) (cc.cpp:11-64) for single streams of a multi-stream engine.

The yardstick of a reset stream is its oracle after Oracle.reset() (the SAME object: it keeps the inclination table, as the reference's
resize does); the yardstick of every other stream is its uninterrupted oracle or a twin engine that never had the reset. Everything is
compared bit for bit. After a reset the robot transform of the stream is gone on both sides and is set again on both."""
import numpy as np
import pytest

import cases
import util
from continuous_clustering_amd import capi, synth, take

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
EVENT_FIELDS = ("type", "a", "b", "c", "d", "column")
MOTIONS = (synth.Motion.static, synth.Motion.translate, synth.Motion.turn)


def _device_batches(streams, n_batches, F):
    import torch
    S, R = len(streams), streams[0].sensor.num_rows
    xyz = torch.from_numpy(np.stack([st.xyz[:n_batches * F].reshape(n_batches, F, R, 3) for st in streams], axis=1)).cuda()
    inten = torch.from_numpy(np.stack([st.intensity[:n_batches * F].reshape(n_batches, F, R) for st in streams], axis=1)).cuda()
    poses = torch.from_numpy(np.stack([st.poses[:n_batches * F].reshape(n_batches, F, 12) for st in streams], axis=1)).cuda()
    torch.cuda.synchronize()
    assert xyz.shape[:2] == (n_batches, S)
    return xyz, inten, poses


def _part(st, b, F, n=1):
    return st.xyz[b * F:(b + n) * F], st.intensity[b * F:(b + n) * F], st.poses[b * F:(b + n) * F]


class Shape:
    """Streams of one shape, made once for the module: host arrays for the oracles, device batches for the engines (read-only)."""

    def __init__(self, rows, cols, S, F, NB, seed, sensor=None, cfg=None):
        self.rows, self.cols, self.S, self.F, self.NB = rows, cols, S, F, NB
        self.sensor = sensor or synth.SensorModel(num_rows=rows, num_columns=cols)
        self.cfg = cfg or capi.Config.kitti()
        self.cfg.num_columns = cols
        self.streams = [synth.make_stream(F * NB, seed=seed + s, sensor=self.sensor, motion=MOTIONS[s % 3]()) for s in range(S)]
        self.dev = _device_batches(self.streams, NB, F)

    def engine(self, events, tf=IDENTITY):
        from continuous_clustering_amd import Engine
        e = Engine(self.cfg, self.rows, self.S, 0, tf)
        e.record_events(events)
        return e

    def oracles(self, tf=IDENTITY):
        from oracle.pyoracle import Oracle
        return [Oracle(self.cfg, self.rows, tf) for _ in range(self.S)]

    def call(self, e, b):
        e.add_firings_device(self.F, self.dev[0][b], self.dev[1][b], self.dev[2][b])

    def feed_oracle(self, o, s, b):
        return o.add_firings(*_part(self.streams[s], b, self.F))


@pytest.fixture(scope="module")
def six(oracle_lib):
    return Shape(64, 720, 6, 360, 8, seed=1100)


def _check_call(e, s, o):
    """What stream `s` reported and published in the last call against its oracle, which was fed the same firings."""
    ev, ref = e.drain_events(s), o.drain_events()
    assert len(ev) == len(ref), (s, len(ev), len(ref))
    assert (ev["stream"] == s).all()
    for fld in EVENT_FIELDS:
        assert np.array_equal(ev[fld], ref[fld]), (s, fld)
    pub = ev[(ev["type"] == capi.EV_PUBLISH_COLUMNS) & (ev["b"] >= ev["a"])]
    if len(pub):
        lo, hi = int(pub["a"].min()), int(pub["b"].max())
        util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo)
    return len(pub)


def _check_state(e, s, o):
    so, se = o.state(), e.state(s)
    for k in util.STATE_FIELDS:
        assert so[k] == se[k], (s, k, so[k], se[k])


def _check_retained_columns(e, s, o, back=600):
    se = e.state(s)
    hi = se["first_unpublished_global_column_index"] - 1
    lo = max(hi - back, se["ring_buffer_start_global_column_index"], 0)
    assert hi > lo
    util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo, mirror=False)


def _reset_both(e, oracles, listed, tf=IDENTITY):
    e.reset_streams(listed)
    for s in listed:
        oracles[s].reset()
        if tf is not None:
            e.set_robot_from_sensor(tf, stream=s)
            oracles[s].set_robot_from_sensor(tf)


def _parity_around_reset(shape, reset_after, listed):
    """Events on: after every call every stream's events and published columns equal its oracle's; the listed streams are reset, with their
    oracles, behind call `reset_after`, their events of that call still queued (the reset drops them)."""
    e, oracles = shape.engine(True), shape.oracles()
    published = [0] * shape.S
    for b in range(shape.NB):
        shape.call(e, b)
        assert e.sync() == 0, e.last_error()
        for s in range(shape.S):
            assert shape.feed_oracle(oracles[s], s, b) == 0
        resetting = b + 1 == reset_after
        for s in range(shape.S):
            if not (resetting and s in listed):
                published[s] += _check_call(e, s, oracles[s])
        if resetting:
            for s in listed:  # mid-rotation: trees unfinished, columns unpublished
                st = e.state(s)
                assert st["n_unfinished_trees"] > 0 and st["first_unpublished_global_column_index"] < st["first_unfinished_global_column_index"]
            _reset_both(e, oracles, listed)
            for s in listed:
                assert len(e.drain_events(s)) == 0 and len(e.drain_links(s)) == 0
                _check_state(e, s, oracles[s])
    for s in range(shape.S):
        assert published[s] > 0, s
        _check_state(e, s, oracles[s])
    e.close()


def test_parity_around_a_mid_rotation_reset(six):
    _parity_around_reset(six, reset_after=3, listed=[1, 4])


def _stream_slice(records, table, s):
    a, n = int(table[s]["first_record"]), int(table[s]["n_records"])
    return records[a:a + n].tobytes()


def _take_everything(e):
    """(point records, their table, cluster descriptors, cluster records, their table) of the next takes, on the host."""
    rec, tab = e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS)
    cl, crec, ctab = e.take_clusters(6)
    return (rec.cpu().numpy().view(take.TAKE_POINT_DTYPE).reshape(-1), tab, cl.cpu().numpy().view(take.TAKE_CLUSTER_DTYPE).reshape(-1),
            crec.cpu().numpy().view(take.TAKE_POINT_DTYPE).reshape(-1), ctab)


def _stream_clusters(taken, s, above=None):
    """Descriptors of stream `s` as bytes, without where they sit in the arrays, and every cluster's records."""
    _, _, cl, crec, ctab = taken
    d = cl[int(ctab[s]["first_cluster"]):int(ctab[s]["first_cluster"]) + int(ctab[s]["n_clusters"])].copy()
    if above is not None:
        d = d[d["col_from"] > above]
    records = [crec[int(c["first_record"]):int(c["first_record"]) + int(c["n_points"])].tobytes() for c in d]
    d["first_record"] = 0
    d["stream"] = 0
    return len(d), d.tobytes(), records


def _assert_same_take(got, sg, ref, sr, clusters_above=None):
    """Stream `sg` of one engine's takes against stream `sr` of another's: the same bytes, but for where the slices start in the arrays.
    `clusters_above`: only the clusters that begin above this column (see test_reset_between_pipelined_calls)."""
    rec_g, tab_g, _, _, ctab_g = got
    rec_r, tab_r, _, _, ctab_r = ref
    for k in ("col_from", "col_to", "n_records", "error"):
        assert tab_g[sg][k] == tab_r[sr][k], (sg, k, tab_g[sg][k], tab_r[sr][k])
    assert _stream_slice(rec_g, tab_g, sg) == _stream_slice(rec_r, tab_r, sr), sg
    for k in ("id_from", "id_to", "error") if clusters_above is not None else ("id_from", "id_to", "lost_columns", "n_records", "n_clusters", "error"):
        assert ctab_g[sg][k] == ctab_r[sr][k], (sg, k, ctab_g[sg][k], ctab_r[sr][k])
    ng, dg, rg = _stream_clusters(got, sg, clusters_above)
    nr, dr, rr = _stream_clusters(ref, sr, clusters_above)
    assert ng == nr and dg == dr and rg == rr, (sg, ng, nr)
    return ng


@pytest.mark.parametrize("options", [(), (("assoc_batch", 0),), (("parallel_insert", 0),), (("lazy_gate_from", 1),), (("lazy_gate", 0), ("lazy_gate_from", 0))],
                         ids=["default", "assoc_batch_0", "parallel_insert_0", "lazy_gate_on", "lazy_gate_off"])
def test_reset_between_pipelined_calls(six, options):
    """Events off, no synchronisation between the calls but the one the reset implies: the untouched streams end as those of a twin engine
    that never had the reset (state, bytes of take_points and take_clusters), the reset ones as their oracles."""
    listed = [1, 4]
    a, t = six.engine(False), six.engine(False)
    for e in (a, t):
        for name, value in options:
            e.set_option(name, value)
    for b in range(six.NB):
        six.call(a, b)
        six.call(t, b)
        if b == 2:
            a.reset_streams(listed)
            for s in listed:
                a.set_robot_from_sensor(IDENTITY, stream=s)
    assert a.sync() == 0, a.last_error()
    assert t.sync() == 0, t.last_error()
    lazy = dict(options).get("lazy_gate_from")
    if lazy is not None:
        assert (a.gate_counters()["lazy_batches"] > 0) == (lazy == 1), a.gate_counters()
    oracles = six.oracles()
    for s in listed:
        for b in range(six.NB):
            assert six.feed_oracle(oracles[s], s, b) == 0
            if b == 2:
                oracles[s].reset()
                oracles[s].set_robot_from_sensor(IDENTITY)
        _check_state(a, s, oracles[s])
        _check_retained_columns(a, s, oracles[s])
    # How far the deferred clearing of the ring has come depends on how the chains of unsynchronised calls overlapped, and with it the lowest
    # column a take can still hand over (cc_engine_take_cursor: readable_from). The two engines are asked for what both still hold: the
    # point cursors are set to the higher of the two bounds, and of the clusters those that begin above it are compared (one that begins at
    # or below it may have lost points in one engine and not in the other).
    above = {}
    for s in range(six.S):
        if s not in listed:
            lo = max(a.take_cursor(take.TAKE_CLUSTERED, s)[1], t.take_cursor(take.TAKE_CLUSTERED, s)[1])
            a.take_seek(lo, take.TAKE_CLUSTERED, s)
            t.take_seek(lo, take.TAKE_CLUSTERED, s)
            above[s] = max(a.take_clusters_cursor(s)[2], t.take_clusters_cursor(s)[2])
    got, ref = _take_everything(a), _take_everything(t)
    for s in range(six.S):
        if s not in listed:
            assert a.state(s) == t.state(s), s
            assert got[1][s]["n_records"] > 64 * 720  # (more than a rotation of columns)
            assert _assert_same_take(got, s, ref, s, clusters_above=above[s]) > 20
    a.close()
    t.close()


def test_parity_around_a_reset_at_128_rows(oracle_lib):
    """Two rows per lane."""
    shape = Shape(128, 360, 3, 180, 8, seed=1300, sensor=cases._s128(360), cfg=cases._vls(360))
    _parity_around_reset(shape, reset_after=3, listed=[1])


class _DeviceBytes:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _output_planes(e, s, cells):
    """(ground labels [cells] u8, cluster ids [cells] u32) of the stream's whole ring, straight from the engine's planes."""
    import torch
    g, i = e.output_planes(s)
    ground = torch.as_tensor(_DeviceBytes(g, cells), device="cuda").cpu().numpy().copy()
    ids = torch.as_tensor(_DeviceBytes(i, cells * 4), device="cuda").cpu().numpy().copy().view(np.uint32)
    return ground, ids


def test_slices_that_do_not_start_on_16_bytes(oracle_lib):
    """3 rows x 37 columns: a stream's ring has 1110 cells, so the slices of stream 1 start 1110 (1-byte planes), 2220 (2-byte) and 4440
    (4-byte) bytes into their planes and end as unevenly. Not a byte of streams 0 and 2 changes; stream 1 reads back as cleared everywhere."""
    rows, cols = 3, 37
    shape = Shape(rows, cols, 3, 37, 6, seed=1400)
    cells = cols * 10 * rows
    assert cells == 1110 and cells % 16 != 0 and (2 * cells) % 16 != 0
    e, oracles = shape.engine(True), shape.oracles()
    fresh = shape.engine(True)
    for b in range(shape.NB):
        shape.call(e, b)
        assert e.sync() == 0, e.last_error()
        for s in range(shape.S):
            assert shape.feed_oracle(oracles[s], s, b) == 0
            _check_call(e, s, oracles[s])
        if b == 3:
            before = [_output_planes(e, s, cells) for s in range(3)]
            assert (before[1][0] != capi.GP_UNKNOWN).any(), "stream 1 had segmented nothing: the reset would not show"
            _reset_both(e, oracles, [1])
            after = [_output_planes(e, s, cells) for s in range(3)]
            for s in (0, 2):
                assert np.array_equal(before[s][0], after[s][0]) and np.array_equal(before[s][1], after[s][1]), s
            assert (after[1][0] == capi.GP_UNKNOWN).all() and (after[1][1] == 0).all()
            got, ref = e.read_columns(0, cols * 10 - 1, stream=1), fresh.read_columns(0, cols * 10 - 1, stream=1)
            for k in ref:
                assert got[k].tobytes() == ref[k].tobytes(), k
            assert (got["global_column_index"] == -1).all() and np.isnan(got["distance"]).all() and (got["is_ignored"] == 0).all()
            assert (got["debug_ground_point_label"] == 143).all()  # CC_DBG_WHITE
            assert (got["tree_root_global_column"] == -1).all()
            for s in (0, 2):  # (and what the neighbours had published is still there)
                _check_retained_columns(e, s, oracles[s], back=cols)
    for s in range(shape.S):
        _check_state(e, s, oracles[s])
    e.close()
    fresh.close()


def test_listing_every_stream_is_the_whole_reset(six):
    """reset_streams(range(S)) on one engine, reset() on its twin, then the same calls to both: events, states and take bytes stay identical."""
    a, w = six.engine(True), six.engine(True)
    for b in range(6):
        for e in (a, w):
            six.call(e, b)
            assert e.sync() == 0, e.last_error()
        for s in range(six.S):
            ea, ew = a.drain_events(s), w.drain_events(s)
            assert ea.tobytes() == ew.tobytes(), (b, s)
        if b == 2:
            _take_everything(a), _take_everything(w)  # (so that the cursors have something to lose)
            a.reset_streams(range(six.S))
            w.reset()
            for e in (a, w):
                e.set_robot_from_sensor(IDENTITY)
            for s in range(six.S):
                assert a.state(s) == w.state(s), s
                for stage in (take.TAKE_CLUSTERED, take.TAKE_SEGMENTED):
                    assert a.take_cursor(stage, s) == w.take_cursor(stage, s) and a.take_cursor(stage, s)[0] == 0
                assert a.take_clusters_cursor(s) == w.take_clusters_cursor(s)
    got, ref = _take_everything(a), _take_everything(w)
    for s in range(six.S):
        assert a.state(s) == w.state(s), s
        _assert_same_take(got, s, ref, s)
        assert got[1][s]["n_records"] > 0
    a.close()
    w.close()


def test_a_dead_stream_comes_back(oracle_lib):
    """The deliberate overrun of tests/test_gpu_ringwrap.py (no finished-cluster check for more than ten rotations: the eleventh runs into
    its own tail, CC_ERR_RING_OVERRUN, a status code) on stream 1 of three, through the host entry; streams 0 and 2 get two rotations each
    and stay healthy. reset_streams([1]) clears the error; the stream then follows its reset oracle and the others never notice."""
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    stream, cfg, tf = cases.build_case("w_s64_240x13")
    assert tf is None
    cfg = cfg.copy()
    cfg.cluster_point_trees_every_nth_column = 100000
    cols = 240
    e = Engine(cfg, 64, 3)
    e.record_events(True)
    oracles = [Oracle(cfg, 64) for _ in range(3)]
    fed = [0, 0, 0]

    def feed(s, rotations, expect=0):
        for _ in range(rotations):
            part = _part(stream, fed[s], 1, cols)
            assert len(part[0]) == cols
            rc_o, rc_e = oracles[s].add_firings(*part), e.add_firings(*part, stream=s)
            fed[s] += cols
            assert rc_o == rc_e, (s, fed[s], rc_o, rc_e, e.last_error())
            if rc_e != 0:
                return rc_e
            _check_call(e, s, oracles[s])
            _check_state(e, s, oracles[s])
        return 0

    assert feed(0, 2) == 0 and feed(2, 2) == 0
    assert feed(1, 13) == capi.CC_ERR_RING_OVERRUN
    assert e.state(1)["error"] == capi.CC_ERR_RING_OVERRUN
    assert feed(0, 1) == 0  # (the others run on beside the dead stream)
    others = {s: e.state(s) for s in (0, 2)}
    fed[1] = 0
    _reset_both(e, oracles, [1])
    st = e.state(1)
    assert st["error"] == 0 and st["reset_required"] == 0 and st["error_a"] == 0 and st["error_b"] == 0
    _check_state(e, 1, oracles[1])
    for s in (0, 2):
        assert e.state(s) == others[s], s
    assert feed(1, 3) == 0 and feed(0, 1) == 0 and feed(2, 2) == 0
    # and all three through the device entry, side by side
    import torch
    parts = [_part(stream, fed[s], 1, cols) for s in range(3)]
    bufs = [torch.from_numpy(np.stack([p[k] for p in parts])).cuda() for k in range(3)]
    torch.cuda.synchronize()
    e.add_firings_device(cols, *bufs)
    assert e.sync() == 0, e.last_error()
    for s in range(3):
        assert oracles[s].add_firings(*parts[s]) == 0
        _check_call(e, s, oracles[s])
        _check_state(e, s, oracles[s])
    e.close()


@pytest.mark.parametrize("take_before", [True, False], ids=["take_before_reset", "first_take_after_reset"])
def test_take_cursors_of_a_reset_stream(six, take_before):
    """The reset stream's hand-over starts again (cursor 0, next cluster id 1) whether the cursor blocks existed at the reset or not: its next
    slices equal those of the same stream of an engine whose streams are all fresh (a twin that had the whole reset at the same place, which
    keeps the inclination table as well); the other streams' slices equal those of a twin that had no reset."""
    s1 = 2
    a, t, w = six.engine(False), six.engine(False), six.engine(False)
    for b in range(3):
        for e in (a, t, w):
            six.call(e, b)
    if take_before:
        first = [_take_everything(e) for e in (a, t, w)]
        assert first[0][1][s1]["n_records"] > 0 and first[0][4][s1]["n_clusters"] > 0
        assert a.take_cursor(take.TAKE_CLUSTERED, s1)[0] > 0
    a.reset_streams(s1)
    a.set_robot_from_sensor(IDENTITY, stream=s1)
    w.reset()
    w.set_robot_from_sensor(IDENTITY)
    assert t.sync() == 0, t.last_error()
    for stage in (take.TAKE_CLUSTERED, take.TAKE_SEGMENTED):
        assert a.take_cursor(stage, s1) == w.take_cursor(stage, s1) and a.take_cursor(stage, s1)[0] == 0
        for s in range(six.S):
            if s != s1:
                assert a.take_cursor(stage, s) == t.take_cursor(stage, s), (stage, s)
    assert a.take_clusters_cursor(s1)[0] == 1
    for s in range(six.S):
        if s != s1:
            assert a.take_clusters_cursor(s) == t.take_clusters_cursor(s), s
    records = clusters = 0
    for b in range(3, 7):  # a take behind every call, as a consumer takes: nothing is cleared before it has been handed over
        for e in (a, t, w):
            six.call(e, b)
        got, ref_t, ref_w = _take_everything(a), _take_everything(t), _take_everything(w)
        assert got[1][s1]["lost_columns"] == 0 and got[4][s1]["lost_columns"] == 0
        clusters += _assert_same_take(got, s1, ref_w, s1)
        records += int(got[1][s1]["n_records"])
        assert a.state(s1) == w.state(s1)
        for s in range(six.S):
            if s != s1:
                _assert_same_take(got, s, ref_t, s)
                assert a.state(s) == t.state(s), s
    assert records > 64 * 720 and clusters > 20
    for e in (a, t, w):
        e.close()


def test_the_robot_transform_is_gone_after_a_reset(oracle_lib):
    """A tilted robot_from_sensor on all streams, one stream reset: it runs as the oracle does after reset(), i.e. into the reference's
    "Transform robot frame from sensor frame was not set yet" (cc.cpp:298-299) at the first column it segments, and with the transform
    once it has been set again; the others keep theirs."""
    ang = np.deg2rad(4.0)
    tilt = np.array([np.cos(ang), 0, np.sin(ang), 0.3, 0, 1, 0, -0.1, -np.sin(ang), 0, np.cos(ang), 0.2], dtype=np.float64)
    shape = Shape(64, 720, 3, 360, 7, seed=1500)
    e, oracles = shape.engine(True, tilt), shape.oracles(tilt)

    def call(b, dead=()):
        shape.call(e, b)
        rc = e.sync()
        for s in range(shape.S):
            rc_o = shape.feed_oracle(oracles[s], s, b)
            if s in dead:
                assert rc_o == capi.CC_ERR_NO_ROBOT_TRANSFORM and e.state(s)["error"] == capi.CC_ERR_NO_ROBOT_TRANSFORM
            else:
                assert rc_o == 0
                _check_call(e, s, oracles[s])
                _check_state(e, s, oracles[s])
        assert rc == (capi.CC_ERR_NO_ROBOT_TRANSFORM if dead else 0), (rc, e.last_error())

    call(0), call(1)
    _reset_both(e, oracles, [1], tf=None)
    call(2, dead=[1])
    _reset_both(e, oracles, [1], tf=tilt)
    for b in range(3, shape.NB):
        call(b)
    assert e.state(1)["cells_published"] > 0
    e.close()


def test_host_entry_around_a_reset(oracle_lib):
    """One-firing add_firings(stream=s) calls on a multi-stream engine before and after reset_streams([s]): these calls answer
    cc_engine_stream_state from a host-side copy of the state and cc_engine_read_columns from views mirrored with the call's results, and
    neither may survive the reset."""
    s1, F = 1, 720
    shape = Shape(64, 720, 3, F, 3, seed=1600)
    e, oracles = shape.engine(True), shape.oracles()
    st = shape.streams

    def feed(s, f0, n):
        part = (st[s].xyz[f0:f0 + n], st[s].intensity[f0:f0 + n], st[s].poses[f0:f0 + n])
        assert oracles[s].add_firings(*part) == 0
        assert e.add_firings(*part, stream=s) == 0, e.last_error()
        pubs = _check_call(e, s, oracles[s])
        _check_state(e, s, oracles[s])
        return pubs

    for s in (0, 2):
        feed(s, 0, 500)
    others = {s: e.state(s) for s in (0, 2)}
    feed(s1, 0, F + 100)
    pubs = sum(feed(s1, F + 100 + k, 1) for k in range(60))
    assert pubs > 0
    hi = e.state(s1)["first_unpublished_global_column_index"] - 1
    assert (e.read_columns(hi - 3, hi, stream=s1)["global_column_index"] >= 0).any()
    _reset_both(e, oracles, [s1])
    _check_state(e, s1, oracles[s1])
    assert e.state(s1)["firings_consumed"] == 0
    assert (e.read_columns(hi - 3, hi, stream=s1)["global_column_index"] == -1).all()
    for s in (0, 2):
        assert e.state(s) == others[s], s
    f0 = F + 160
    feed(s1, f0, F + 100)
    assert sum(feed(s1, f0 + F + 100 + k, 1) for k in range(60)) > 0
    for s in (0, 2):
        feed(s, 500, 400)
    e.close()


def _raw_reset(e, n, idx):
    arr = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    return e.L.cc_engine_reset_streams(e.h, n, None if arr is None else arr.ctypes.data)


def test_arguments(six):
    a, t = six.engine(False), six.engine(False)
    for e in (a, t):
        six.call(e, 0)
        six.call(e, 1)
        assert e.sync() == 0, e.last_error()
    before = [a.state(s) for s in range(six.S)]
    assert before[0]["firings_consumed"] == 2 * six.F
    for n, idx in ((-1, [0]), (1, None), (1, [six.S]), (2, [0, -1]), (3, [1, 2, 1 << 20])):
        assert _raw_reset(a, n, idx) == capi.CC_ERR_INVALID_ARGUMENT, (n, idx)
        assert "cc_engine_reset_streams" in a.last_error()
        assert [a.state(s) for s in range(six.S)] == before, (n, idx)
    assert _raw_reset(a, 0, None) == capi.CC_OK and _raw_reset(a, 0, [5]) == capi.CC_OK
    a.reset_streams([])
    assert [a.state(s) for s in range(six.S)] == before
    # duplicates behave as one
    a.reset_streams([3, 3, 1, 3])
    t.reset_streams([1, 3])
    for e in (a, t):
        for s in (1, 3):
            e.set_robot_from_sensor(IDENTITY, stream=s)
        six.call(e, 2)
        six.call(e, 3)
        assert e.sync() == 0, e.last_error()
    for s in range(six.S):
        assert a.state(s) == t.state(s), s
        assert (a.state(s)["firings_consumed"] == 2 * six.F) == (s in (1, 3))
    # an int is a list of one
    a.reset_streams(np.int64(2))
    assert a.state(2)["firings_consumed"] == 0 and a.state(0)["firings_consumed"] == 4 * six.F
    # reset_required for a reason that needs no other shape: cleared for the listed streams only
    cfg = six.cfg.copy()
    cfg.is_single_threaded = 0
    a.set_config(cfg)
    assert all(a.state(s)["reset_required"] == 1 for s in range(six.S))
    a.reset_streams([0, 5])
    assert [a.state(s)["reset_required"] for s in range(six.S)] == [0, 1, 1, 1, 1, 0]
    # a change of shape that waits for cc_engine_reset cannot be had for one stream
    cfg.num_columns = 360
    a.set_config(cfg)
    before = [a.state(s) for s in range(six.S)]
    assert _raw_reset(a, 1, [0]) == capi.CC_ERR_INVALID_ARGUMENT
    assert "cc_engine_reset_streams" in a.last_error() and "cc_engine_reset " in a.last_error()
    assert [a.state(s) for s in range(six.S)] == before
    a.reset()
    assert all(a.state(s)["reset_required"] == 0 for s in range(six.S))
    a.close()
    t.close()
