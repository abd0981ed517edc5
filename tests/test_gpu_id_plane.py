"""GPU: the id plane of cc_engine_output_planes is maintained from the first call that asks for it ("publish").

Until then the engine writes no cluster ids into Planes::id: a pipelined batch launches no k_publish, the small-call kernels skip the pass. The
first cc_engine_output_planes call with a non-null d_cluster_id fills the plane for every published column still in the ring and switches the
per-batch publishing on for good. The yardstick is the oracle's published `id` of the columns in [max(clear_done, first_column),
first_unpublished), ring slot by ring slot; outside that range the plane has no validity rule and nothing is compared. How far the deferred
clearing has come depends on how the chains of unsynchronised calls overlapped, so two engines are compared on the range both still hold."""
import numpy as np
import pytest

import util
from continuous_clustering_amd import capi, kitti, synth, take

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
MOTIONS = (synth.Motion.static, synth.Motion.translate, synth.Motion.turn)
RING_ROTATIONS = 10


class _DeviceBytes:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _read_ids(ptr, cells):
    import torch
    return torch.as_tensor(_DeviceBytes(ptr, cells * 4), device="cuda").cpu().numpy().copy().view(np.uint32)


class Shape:
    """Streams of one shape, made once for the module: host arrays for the oracles and the small calls, device batches for the pipelined calls
    (read-only). `extra` firings per stream lie behind the NB batches of F."""

    def __init__(self, rows, cols, S, F, NB, seed, extra=0, sensor=None, max_distance=None):
        import torch
        self.rows, self.cols, self.S, self.F, self.NB = rows, cols, S, F, NB
        self.cells = cols * RING_ROTATIONS * rows
        self.sensor = sensor or synth.SensorModel(num_rows=rows, num_columns=cols)
        self.cfg = capi.Config.kitti()
        self.cfg.num_columns = cols
        if max_distance is not None:
            self.cfg.max_distance = max_distance
        self.streams = [synth.make_stream(F * NB + extra, seed=seed + s, sensor=self.sensor, motion=MOTIONS[s % 3]()) for s in range(S)]
        cut = lambda a, tail: np.stack([a(st)[:NB * F].reshape((NB, F) + tail) for st in self.streams], axis=1)  # noqa: E731
        self.dev = tuple(torch.from_numpy(x).cuda() for x in (cut(lambda st: st.xyz, (rows, 3)), cut(lambda st: st.intensity, (rows,)),
                                                              cut(lambda st: st.poses, (12,))))
        torch.cuda.synchronize()
        self._ref = {}

    def engine(self):
        from continuous_clustering_amd import Engine
        e = Engine(self.cfg, self.rows, self.S, 0, IDENTITY)
        e.record_events(False)
        return e

    def call(self, e, b):
        e.add_firings_device(self.F, self.dev[0][b], self.dev[1][b], self.dev[2][b])

    def part(self, s, f0, n):
        st = self.streams[s]
        return st.xyz[f0:f0 + n], st.intensity[f0:f0 + n], st.poses[f0:f0 + n]

    def oracles_after(self, batches):
        """One oracle per stream, fed the first `batches` batches; computed once per count and shared, so left as they are (tests that feed further take fresh_oracles)."""
        if batches not in self._ref:
            self._ref[batches] = self.fresh_oracles(batches)
        return self._ref[batches]

    def fresh_oracles(self, batches):
        from oracle.pyoracle import Oracle
        out = []
        for s in range(self.S):
            o = Oracle(self.cfg, self.rows, IDENTITY)
            assert o.add_firings(*self.part(s, 0, batches * self.F)) == 0, o.last_error()
            out.append(o)
        return out


@pytest.fixture(scope="module")
def tiny(oracle_lib):
    """3 rows x 37 columns, three streams (tests/test_gpu_reset_streams.py): a ring of 1110 cells, slices that do not start on 16 bytes; 13 rotations.
    With the 64-row sensor's inclinations and the KITTI max_distance such a stream publishes no cluster id at all (columns 10 degrees apart, two
    of three rows on the ground): the rows look ahead (4 .. -2 degrees) and points up to 8 m apart associate, which gives 40 - 50 clusters per stream."""
    shape = Shape(3, 37, 3, 37, 13, seed=2100, sensor=synth.SensorModel(num_rows=3, num_columns=37, incl_top_deg=4.0, incl_bottom_deg=-2.0), max_distance=8.0)
    assert shape.cells == 1110
    return shape


@pytest.fixture(scope="module")
def sensor(oracle_lib):
    """64 rows x 360 columns, two streams, one rotation per call: k_insert_par fused, k_assocb, pipelined; 13 rotations and firings for small calls."""
    return Shape(64, 360, 2, 360, 13, seed=2200, extra=600)


def _held_range(e, s):
    """[max(clear_done, first_column), first_unpublished) of stream `s` (cc_engine_take_cursor reports the lower end)."""
    lo = e.take_cursor(take.TAKE_CLUSTERED, s)[1]
    hi = e.state(s)["first_unpublished_global_column_index"]
    return lo, hi


def _slots(shape, plane, lo, hi):
    """The plane's ids of columns [lo, hi) as [columns, rows], read ring slot by ring slot."""
    rc = shape.cols * RING_ROTATIONS
    assert 0 <= lo and hi - lo <= rc
    lc = np.arange(lo, hi) % rc
    return plane.reshape(rc, shape.rows)[lc]


def _assert_current(shape, planes, ranges, oracles, min_columns):
    """Every plane of `planes` ([engine][stream] -> ids of the whole ring) equals the oracle's published ids on the range all engines hold."""
    for s in range(shape.S):
        lo, hi = max(r[s][0] for r in ranges), min(r[s][1] for r in ranges)
        assert hi - lo >= min_columns, (s, lo, hi)
        assert all(r[s][1] == hi for r in ranges), (s, [r[s] for r in ranges])
        want = oracles[s].read_published(lo, hi - 1, fields=("id",))["id"]
        assert (want != 0).any(), s
        for k, p in enumerate(planes):
            got = _slots(shape, p[s], lo, hi)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"engine {k} stream {s}: {len(bad)} ids differ, first (col {lo + bad[0][0]}, row {bad[0][1]}): " \
                                  f"plane {got[tuple(bad[0])]} oracle {want[tuple(bad[0])]}"


def _backlog_equals_per_batch(shape, min_columns):
    a, b = shape.engine(), shape.engine()
    ptr_a = [a.output_planes(s)[1] for s in range(shape.S)]  # before the first firing: ids per batch from the start
    for k in range(shape.NB):
        shape.call(a, k)
        shape.call(b, k)
    assert a.sync() == 0, a.last_error()
    assert b.sync() == 0, b.last_error()
    ptr_b = [b.output_planes(s)[1] for s in range(shape.S)]  # the first request: the backlog of the whole ring
    planes = [[_read_ids(p, shape.cells) for p in ptrs] for ptrs in (ptr_a, ptr_b)]
    ranges = [[_held_range(e, s) for s in range(shape.S)] for e in (a, b)]
    for s in range(shape.S):
        assert ranges[0][s][0] > 0, "nothing has been cleared: slot reuse would not show"
    _assert_current(shape, planes, ranges, shape.oracles_after(shape.NB), min_columns)
    for s in range(shape.S):  # (and the two planes, byte for byte, on what both hold)
        lo, hi = max(ranges[0][s][0], ranges[1][s][0]), ranges[0][s][1]
        assert _slots(shape, planes[0][s], lo, hi).tobytes() == _slots(shape, planes[1][s], lo, hi).tobytes(), s
    a.close()
    b.close()


def test_backlog_equals_per_batch_publishing_3_rows(tiny):
    _backlog_equals_per_batch(tiny, min_columns=tiny.cols // 2)


def test_backlog_equals_per_batch_publishing_64_rows(sensor):
    _backlog_equals_per_batch(sensor, min_columns=sensor.cols // 2)


def test_sticky_over_pipelined_batches_and_small_calls(sensor):
    """One request in mid-stream, without a synchronisation in front of it; then further pipelined batches and calls of 1, 3, 8 (captured graph),
    20, 63 (k_small_all launched directly) and 100 firings (the host path's general launch) on each stream, never asking again: the plane
    read through the first pointers is current."""
    e = sensor.engine()
    for k in range(6):
        sensor.call(e, k)
    ptrs = [e.output_planes(s)[1] for s in range(sensor.S)]
    for k in range(6, sensor.NB):
        sensor.call(e, k)
    oracles = sensor.fresh_oracles(sensor.NB)
    f0 = sensor.NB * sensor.F
    for n in (1, 3, 8, 20, 63, 100, 5, 1):
        for s in range(sensor.S):
            part = sensor.part(s, f0, n)
            assert oracles[s].add_firings(*part) == 0
            assert e.add_firings(*part, stream=s) == 0, e.last_error()
        f0 += n
    assert e.sync() == 0, e.last_error()
    for s in range(sensor.S):
        assert e.state(s)["first_unpublished_global_column_index"] == oracles[s].state()["first_unpublished_global_column_index"]
        assert e.state(s)["first_unpublished_global_column_index"] > sensor.oracles_after(sensor.NB)[s].state()["first_unpublished_global_column_index"], \
            "the small calls published nothing"
    planes = [[_read_ids(p, sensor.cells) for p in ptrs]]
    ranges = [[_held_range(e, s) for s in range(sensor.S)]]
    _assert_current(sensor, planes, ranges, oracles, min_columns=sensor.cols // 2)
    assert [e.output_planes(s)[1] for s in range(sensor.S)] == ptrs
    e.close()


def test_small_call_kernels_made_before_the_request_are_replaced(sensor):
    """Small calls of 1, 8 (captured graphs) and 20 firings (k_small_all) before anybody asks: their graphs bake in "no ids". The request drops
    them; the same call sizes afterwards publish ids, and the columns the earlier calls published come with the backlog."""
    from oracle.pyoracle import Oracle
    e, s = sensor.engine(), 0
    o = Oracle(sensor.cfg, sensor.rows, IDENTITY)
    f0 = 0

    def feed(n):
        nonlocal f0
        part = sensor.part(s, f0, n)
        assert o.add_firings(*part) == 0
        assert e.add_firings(*part, stream=s) == 0, e.last_error()
        f0 += n

    for _ in range(3):
        feed(sensor.F)
    for k in range(30):
        feed((1, 8, 20)[k % 3])
    asked_at = o.state()["first_unpublished_global_column_index"]
    ptr = e.output_planes(s)[1]
    for k in range(18):
        feed((1, 8, 20)[k % 3])
    lo, hi = _held_range(e, s)
    assert hi == o.state()["first_unpublished_global_column_index"]
    assert lo < asked_at - 50 and asked_at + 100 < hi, (lo, asked_at, hi)  # (columns of the backlog and columns published since, both held)
    want = o.read_published(lo, hi - 1, fields=("id",))["id"]
    assert (want[:asked_at - lo] != 0).any() and (want[asked_at - lo:] != 0).any()
    got = _slots(sensor, _read_ids(ptr, sensor.cells), lo, hi)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} ids differ, first (col {lo + bad[0][0]}, row {bad[0][1]}), asked at column {asked_at}"
    e.close()


def _assert_views(shape, e, oracles):
    """read_columns and take_points(CLUSTERED) of what the engine still holds against the oracles: ids included, raw."""
    rec, tab = e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS)
    rec = rec.cpu().numpy().view(take.TAKE_POINT_DTYPE).reshape(-1)
    for s in range(shape.S):
        lo, hi = _held_range(e, s)
        assert hi - lo >= shape.cols // 2, (s, lo, hi)
        ref = oracles[s].read_published(lo, hi - 1)
        util.compare_columns(ref, e.read_columns(lo, hi - 1, stream=s), lo, mirror=False)
        a, n, c0 = int(tab[s]["first_record"]), int(tab[s]["n_records"]), int(tab[s]["col_from"])
        assert n > 0 and c0 >= lo and int(tab[s]["col_to"]) == hi, (s, tab[s])
        r = rec[a:a + n]
        want = ref["id"][c0 - lo + r["column"].astype(np.int64), r["row"].astype(np.int64)]
        assert np.array_equal(r["id"].astype(np.uint64), want), s
        assert (r["id"] != 0).any(), s


def test_views_do_not_depend_on_the_plane(sensor):
    """The id plane is never asked for: read_columns and take_points ids equal the oracle's after pipelined calls and after small calls."""
    e = sensor.engine()
    for k in range(sensor.NB):
        sensor.call(e, k)
    assert e.sync() == 0, e.last_error()
    _assert_views(sensor, e, sensor.oracles_after(sensor.NB))
    oracles = sensor.fresh_oracles(sensor.NB)
    f0 = sensor.NB * sensor.F
    for n in (1, 8, 20, 63, 100, 2):
        for s in range(sensor.S):
            part = sensor.part(s, f0, n)
            assert oracles[s].add_firings(*part) == 0
            assert e.add_firings(*part, stream=s) == 0, e.last_error()
        f0 += n
    _assert_views(sensor, e, oracles)
    e.close()


def test_reset_with_the_plane_off_then_asked_for(tiny):
    """reset_streams([1]) while nobody has asked for the plane, the first request behind it: stream 1's slice is all zero (it has published
    nothing since), streams 0 and 2 get their backlog; once stream 1 publishes again its slice follows its reset oracle."""
    from oracle.pyoracle import Oracle
    e = tiny.engine()
    for k in range(6):
        tiny.call(e, k)
    e.reset_streams([1])
    e.set_robot_from_sensor(IDENTITY, stream=1)
    ptrs = [e.output_planes(s)[1] for s in range(tiny.S)]
    planes = [_read_ids(p, tiny.cells) for p in ptrs]
    assert (planes[1] == 0).all()
    ranges = [_held_range(e, s) for s in range(tiny.S)]
    assert ranges[1][1] <= ranges[1][0]  # (nothing published)
    for s in (0, 2):
        lo, hi = ranges[s]
        want = tiny.oracles_after(6)[s].read_published(lo, hi - 1, fields=("id",))["id"]
        assert hi - lo >= tiny.cols // 2 and (want != 0).any()
        assert np.array_equal(_slots(tiny, planes[s], lo, hi), want), s
    o1 = Oracle(tiny.cfg, tiny.rows, IDENTITY)
    assert o1.add_firings(*tiny.part(1, 0, 6 * tiny.F)) == 0
    o1.reset()
    o1.set_robot_from_sensor(IDENTITY)
    for k in range(6, tiny.NB):
        tiny.call(e, k)
        assert o1.add_firings(*tiny.part(1, k * tiny.F, tiny.F)) == 0
    assert e.sync() == 0, e.last_error()
    lo, hi = _held_range(e, 1)
    assert hi - lo >= tiny.cols // 2
    want = o1.read_published(lo, hi - 1, fields=("id",))["id"]
    assert (want != 0).any()
    assert np.array_equal(_slots(tiny, _read_ids(ptrs[1], tiny.cells), lo, hi), want)
    e.close()


@pytest.mark.parametrize("scatter", ["device", "batched"])
def test_replay_without_the_plane(tmp_path, oracle_lib, scatter):
    """Two short synthetic KITTI sequences through replay.replay, which never asks for the id plane: the frame scatter takes the ids from the
    trees' roots, and the per-frame records are bit-equal to the oracle walk."""
    from continuous_clustering_amd import replay
    import test_gpu_kitti_replay as kr
    lengths = {2: 3, 5: 2}
    want = []
    for k, (seq, nf) in enumerate(lengths.items()):
        seq_dir, _ = kitti.write_synthetic_sequence(str(tmp_path), seq, nf, seed=500 + 10 * k, motion=(6.0 + k, 0.1 * k, 0.0, 0.1 * (k + 1)))
        sc, _, _ = kr.expected_records(seq_dir, seq, nf)
        sc.finish()
        want.append(np.array(sc.records))
    records, totals = replay.replay(str(tmp_path), list(lengths), scatter=scatter)
    assert totals["streams"] == 2 and totals["frames"] == sum(lengths.values())
    got, allwant = kr.evaluation_sorted(records), np.concatenate(want)
    assert got.shape == allwant.shape and (allwant[:, 2:6].sum(axis=1) > 0).all()
    assert np.array_equal(got.view(np.uint64), allwant.view(np.uint64))
