"""GPU: the replay evaluator (cc_replay_eval_*, include/cc_kitti.h): scatter and evaluation of the replayed frames of
all streams in one device call. "Equal" is bit-equal everywhere: the uint64 views of the doubles are compared.

Yardsticks: oracle.pyoracle.eval_frame and evaluation.eval_frame_device for the label compare alone; for engine streams the host walk
evaluation.FrameScatter with pyoracle.eval_frame over the oracle's published columns, and evaluation.DeviceFrameScatter on a twin engine; for
the KITTI path replay.replay's default scatter and the oracle walk of tests/test_gpu_kitti_replay.py."""
import ctypes

import numpy as np
import pytest

from test_eval_cpu import random_frame

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
NO_POINT = np.uint64(2 ** 64 - 1)
RESULT = ("tp", "fn", "fp", "tn", "over_segmentation_entropy", "under_segmentation_entropy")


def _hip():
    """hipMemcpy of the HIP runtime the product library is bound to (dlsym on its handle also searches its dependencies)"""
    from continuous_clustering_amd import load_library
    L = load_library()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return L


def upload(dst_ptr, array):
    """host array -> raw device pointer (the handle's own storage), after everything enqueued so far"""
    import torch
    torch.cuda.synchronize()
    a = np.ascontiguousarray(array)
    assert _hip().hipMemcpy(dst_ptr, a.ctypes.data, a.nbytes, 1) == 0


def bits(records):
    """[(sequence or stream, frame, 6 doubles)] -> uint64 view, for bit-equality"""
    return np.array([[float(v) for v in r] for r in records], dtype=np.float64).reshape(-1, 8).view(np.uint64)


def rec_rows(rec, ids=None):
    """REPLAY_RECORD_DTYPE array -> [(id of the stream, frame, 6 doubles)]"""
    return [((ids[int(r["stream"])] if ids is not None else int(r["stream"])), int(r["frame"]), *[float(r["r"][n]) for n in RESULT]) for r in rec]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the batched label compare alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4099)


def _label_frames():
    """batches of 7 frames (semantic, euclid, is_ground, detection): every pattern over every size (the first seven and the last seven sizes)"""
    rng = np.random.default_rng(41)

    def few(n):
        return [x.copy() for x in random_frame(rng, n, 3, 4)]

    def own(n):
        f = [x.copy() for x in random_frame(rng, n, 5, 5)]
        f[1] = np.arange(1, n + 1, dtype=np.uint32)                      # every point its own pair
        f[3] = np.arange(n, 0, -1).astype(np.uint32) + np.uint32(7)
        return f

    def zero(n):
        f = [x.copy() for x in random_frame(rng, n, 6, 9)]
        f[0] = np.zeros(n, np.uint16)                                    # all semantic 0: no ground counts
        return f

    batches = {}
    for name, make in (("few", few), ("own", own), ("zero", zero)):
        batches[name + "_a"] = [make(n) for n in SIZES[:7]]
        batches[name + "_b"] = [make(n) for n in reversed(SIZES[2:])]
    odd = [[x.copy() for x in random_frame(rng, n, 10, 10)] for n in (4099, 256, 63, 1, 0, 257, 65)]
    odd[0][1] = odd[0][1].astype(np.uint32)
    odd[0][3] = odd[0][3].astype(np.uint32)
    odd[0][1][100:400] = 0xFFFFFFFF                                      # the pair gt = det = 0xFFFFFFFF looks like a free slot of the table
    odd[0][3][100:300] = 0xFFFFFFFF
    batches["odd"] = odd
    assert all(len(b) == 7 for b in batches.values())
    return batches


@pytest.fixture(scope="module")
def label_frames(oracle_lib):
    from continuous_clustering_amd import evaluation
    from oracle import pyoracle
    import torch
    frames = _label_frames()
    want = {}
    for name, batch in frames.items():
        rows = []
        for f in batch:
            w = pyoracle.eval_frame(*f)
            n = len(f[0])
            t = [torch.from_numpy(np.ascontiguousarray(x).astype(dt).view(vt)).cuda() for x, dt, vt in
                 zip(f, (np.uint16, np.uint32, np.uint8, np.uint32), (np.int16, np.int32, np.uint8, np.int32))]
            d = evaluation.eval_frame_device(n, *t) if n else np.zeros(6)
            assert np.array_equal(w.view(np.uint64), d.view(np.uint64)), (name, n)
            rows.append(w)
        want[name] = np.array(rows)
    return frames, want


@pytest.mark.parametrize("eval_lanes,rounds", [(2, 4), (8, 1)])
def test_batched_label_compare_alone(label_frames, eval_lanes, rounds):
    """Hand-filled slots through cc_replay_eval_evaluate_slots (the documented test entry: no walk, no apply): 7 frames in `rounds` rounds,
    every batch twice through the same handle — the tables must be empty again after a round."""
    from continuous_clustering_amd import Engine, capi, evaluation
    frames, want = label_frames
    cfg = capi.Config.kitti()
    cfg.num_columns = 64
    e = Engine(cfg, 8, 1)
    h = evaluation.ReplayEval(e, slots=7, max_points=4099, eval_lanes=eval_lanes)
    for name, batch in frames.items():
        for k, f in enumerate(batch):
            h.add_frame(0, k, f[0], f[1])
        for k, f in enumerate(batch):
            g, d = h.slot_arrays(0, k)
            if len(f[0]):
                upload(g, np.asarray(f[2], dtype=np.uint8))
                upload(d, np.asarray(f[3], dtype=np.uint32))
        for again in range(2):
            before = h.counters()["eval_rounds"]
            rec = h.evaluate_slots(0, list(range(7)))
            assert h.counters()["eval_rounds"] - before == rounds
            assert [int(r["frame"]) for r in rec] == list(range(7)) and not rec["stream"].any()
            got = np.array([[float(r["r"][n]) for n in RESULT] for r in rec])
            assert np.array_equal(got.view(np.uint64), want[name].view(np.uint64)), (name, again, got, want[name])
    with pytest.raises(Exception):
        h.add_frame(0, 0, np.zeros(4100, np.uint16), np.zeros(4100, np.uint32))   # n_points > max_points
    with pytest.raises(Exception):
        h.add_frame(0, 7, np.zeros(4, np.uint16), np.zeros(4, np.uint32))         # frame >= previous_frame + slots
    h.close()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# synthetic engine streams (the construction of tests/test_gpu_eval.py::test_stream_to_evaluation_end_to_end)
# ---------------------------------------------------------------------------------------------------------------------------------------------
class StreamData:
    """One stream of `nframes` frames of `cols` firings: firings, original_index [frame][col][row] (col * rows + row, about 3 % set to -1),
    per-frame ground truth. nan_first: the first frame's firings are all NaN (nothing is published for them)."""

    def __init__(self, rows, cols, nframes, seed, motion, nan_first=False, sequence=0):
        from continuous_clustering_amd import synth
        self.rows, self.cols, self.nframes, self.sequence = rows, cols, nframes, sequence
        sensor = synth.SensorModel(num_rows=rows, num_columns=cols)
        st = synth.make_stream(cols * nframes, seed=seed, sensor=sensor, motion=motion)
        self.xyz, self.inten, self.poses = st.xyz.copy(), st.intensity.copy(), st.poses.copy()
        hit = st.hit.copy()
        if nan_first:
            self.xyz[:cols] = np.nan
            hit[:cols] = 0
        hit = hit.reshape(nframes, cols * rows)
        self.sem = [np.where(h == 1, 40, np.where(h == 2, 50, np.where(h >= 3, 80, 0))).astype(np.uint16) for h in hit]
        self.eu = [np.where(h >= 3, h - 2, 0).astype(np.uint32) for h in hit]
        rng = np.random.default_rng(seed + 5)
        org = np.tile((np.arange(cols)[:, None] * rows + np.arange(rows)[None, :]).astype(np.int32), (nframes, 1, 1))
        org[rng.random(org.shape) < 0.03] = -1
        self.org = org
        self.n_points = cols * rows

    def frame(self, f):
        a, b = f * self.cols, (f + 1) * self.cols
        return self.xyz[a:b], self.inten[a:b], self.poses[a:b]


def oracle_steps(cfg, sd, groups, finish_last=True, oracle=None, first_group=0):
    """The host walk (evaluation.FrameScatter + pyoracle.eval_frame) over the oracle's published columns; groups: the frames fed before each
    step. -> the records of each step."""
    from continuous_clustering_amd.evaluation import FrameScatter
    from oracle import pyoracle
    o = oracle if oracle is not None else pyoracle.Oracle(cfg, sd.rows, IDENTITY)
    sc = FrameScatter(sd.sequence, [sd.n_points] * sd.nframes, sd.sem, sd.eu, evaluate=pyoracle.eval_frame)
    rows = np.arange(sd.rows)[None, :]
    published_to, steps = -1, []
    for gi, group in enumerate(groups):
        before = len(sc.records)
        for f in group:
            assert o.add_firings(*sd.frame(f)) == 0, o.last_error()
        base, hi = o.published_range()
        lo = max(base, published_to + 1)
        if hi >= lo:
            a = o.read_published(lo, hi, fields=("source_firing", "ground_point_label", "id"))
            src = a["source_firing"]
            fr, col = np.maximum(src, 0) // sd.cols, np.maximum(src, 0) % sd.cols
            pt = sd.org[np.minimum(fr, sd.nframes - 1), col, rows]
            ok = (src >= 0) & (pt >= 0)
            u = np.where(ok, (np.uint64(sd.sequence) << np.uint64(48)) | (fr.astype(np.uint64) << np.uint64(32)) | np.maximum(pt, 0).astype(np.uint64), NO_POINT)
            sc.add_columns(u, a["ground_point_label"], a["id"])
            published_to = hi
        if finish_last and gi == len(groups) - 1:
            sc.finish()
        steps.append(list(sc.records[before:]))
    return steps


def device_frames(sds, f):
    """frame f of every stream as [S][cols][...] device tensors"""
    import torch
    parts = [sd.frame(f) for sd in sds]
    t = [torch.from_numpy(np.stack([p[k] for p in parts])).cuda() for k in range(3)]
    torch.cuda.synchronize()
    return t


class World:
    def __init__(self, rows, cols, nframes, specs):
        from continuous_clustering_amd import capi
        self.rows, self.cols, self.nframes = rows, cols, nframes
        self.cfg = capi.Config.kitti()
        self.cfg.num_columns = cols
        self.sds = [StreamData(rows, cols, nframes, sequence=10 + i, **spec) for i, spec in enumerate(specs)]
        self.S = len(self.sds)
        self.ids = [sd.sequence for sd in self.sds]
        self.one_per_step = [[f] for f in range(nframes)]
        self.want = [oracle_steps(self.cfg, sd, self.one_per_step) for sd in self.sds]   # [stream][step] -> records
        self._dev = {}

    def dev(self, f, sds=None):
        key = (f, None if sds is None else tuple(id(x) for x in sds))
        if key not in self._dev:
            self._dev[key] = device_frames(self.sds if sds is None else sds, f)
        return self._dev[key]

    def engine(self, S=None):
        from continuous_clustering_amd import Engine
        return Engine(self.cfg, self.rows, S or self.S, 0, IDENTITY)

    def want_step(self, k, streams=None):
        return [r for s in (streams if streams is not None else range(self.S)) for r in self.want[s][k]]


def batched_for(w, e, sds=None, slots=4, eval_lanes=2):
    from continuous_clustering_amd import evaluation
    sds = w.sds if sds is None else sds
    return evaluation.ReplayEval(e, slots=slots, max_points=sds[0].n_points, eval_lanes=eval_lanes)


def feed(w, e, h, f, sds=None, streams=None):
    """frame f of every stream into engine and evaluator (ground truth, original_index), one add_firings_device"""
    sds = w.sds if sds is None else sds
    for s, sd in enumerate(sds):
        if streams is None or s in streams:
            if h is not None:
                h.add_frame(s, f, sd.sem[f], sd.eu[f])
                upload(h.original_index_ptr(s, f), sd.org[f])
    x, i, p = w.dev(f, None if sds is w.sds else sds)
    e.add_firings_device(w.cols, x, i, p)


def step_ok(h, finish=None, capacity=None):
    rc, rec, n, table = h.step(finish=finish, capacity=capacity)
    assert rc == 0 and n == len(rec) and int(table["frames_evaluated"].sum()) == n
    assert list(zip(rec["stream"], rec["frame"])) == sorted(zip(rec["stream"], rec["frame"]))   # ordered by stream, then frame
    return rec, table


def twin_device_scatter(w):
    """evaluation.DeviceFrameScatter on an engine of its own, one frame per step, finish on the last: [step] -> records of all streams"""
    import torch
    from continuous_clustering_amd import evaluation
    e = w.engine()
    sc = evaluation.DeviceFrameScatter(e, w.ids, w.sds[0].n_points, rows=w.rows, cols=w.cols)
    steps = []
    for f in range(w.nframes):
        before = [len(r) for r in sc.records]
        for s, sd in enumerate(w.sds):
            sc.add_frame(s, f, sd.sem[f], sd.eu[f])
            sc.d_org[s, f % sc.SLOTS] = torch.from_numpy(sd.org[f]).cuda()
        torch.cuda.synchronize()
        x, i, p = w.dev(f)
        e.add_firings_device(w.cols, x, i, p)
        assert e.sync() == 0, e.last_error()
        sc.publish()
        if f == w.nframes - 1:
            for s in range(w.S):
                sc.finish(s)
        steps.append([r for s in range(w.S) for r in sc.records[s][before[s]:]])
    e.close()
    return steps


@pytest.fixture(scope="module")
def three(oracle_lib):
    from continuous_clustering_amd import synth
    return World(64, 256, 4, [dict(seed=77, motion=synth.Motion.translate(5.0)), dict(seed=78, motion=synth.Motion.turn()),
                              dict(seed=79, motion=synth.Motion.static(), nan_first=True)])


def run_one_frame_per_step(w, eval_lanes):
    """-> [step] -> (record rows, table, eval_rounds of the step)"""
    e = w.engine()
    h = batched_for(w, e, eval_lanes=eval_lanes)
    out = []
    for f in range(w.nframes):
        feed(w, e, h, f)
        before = h.counters()["eval_rounds"]
        rec, table = step_ok(h, finish=[1] * w.S if f == w.nframes - 1 else None)
        out.append((rec_rows(rec, w.ids), table, h.counters()["eval_rounds"] - before))
    h.close()
    e.close()
    return out


def check_against_world(w, out, twin):
    total = 0
    for k, (rows, table, _) in enumerate(out):
        want = w.want_step(k)
        assert len(rows) == len(want), (k, rows, want)
        assert np.array_equal(bits(rows), bits(want)), k
        assert np.array_equal(bits(rows), bits(twin[k])), k
        assert not table["error"].any() and not table["lost_columns"].any() and (table["error_column"] == -1).all()
        total += len(rows)
    assert total == sum(sd.nframes for sd in w.sds)   # every frame of every stream, the last one by `finish`
    assert not out[-1][1]["active"].any()


def test_three_streams_one_frame_per_step(three):
    """3 streams of 64 rows, eval_lanes = 1; stream 2 is fed only NaN firings in the first step (an empty range and no record there)."""
    w = three
    out = run_one_frame_per_step(w, eval_lanes=1)
    check_against_world(w, out, twin_device_scatter(w))
    t0 = out[0][1]
    assert t0["col_from"][2] == t0["col_to"][2] and t0["frames_evaluated"][2] == 0
    assert all(rounds == len(rows) for rows, _, rounds in out)                         # one lane: a round per completed frame
    assert any(len(rows) == 3 and rounds == 3 for rows, _, rounds in out[:-1])         # three streams completing a frame in one step
    # a frame's result is not trivial: points were applied
    assert sum(r[2] + r[3] + r[4] + r[5] for rows, _, _ in out for r in rows) > 0.5 * w.sds[0].n_points


@pytest.mark.parametrize("rows,cols", [(128, 192), (8, 256)])
def test_single_stream_other_row_counts(oracle_lib, rows, cols):
    """128 rows: two row trips per column; 8 rows: most lanes idle."""
    from continuous_clustering_amd import synth
    w = World(rows, cols, 4, [dict(seed=91 + rows, motion=synth.Motion.translate(4.0))])
    check_against_world(w, run_one_frame_per_step(w, eval_lanes=2), twin_device_scatter(w))


def test_two_frames_before_one_step(three):
    """slots = 5: two frames fed between steps; a stream then completes two frames in one step, delivered in order."""
    w = three
    groups = [[0, 1], [2, 3]]
    want = [oracle_steps(w.cfg, sd, groups) for sd in w.sds]
    e = w.engine()
    h = batched_for(w, e, slots=5, eval_lanes=8)
    seen_two = False
    for k, group in enumerate(groups):
        for f in group:
            feed(w, e, h, f)
        rec, table = step_ok(h, finish=[1] * w.S if k == len(groups) - 1 else None)
        exp = [r for s in range(w.S) for r in want[s][k]]
        assert np.array_equal(bits(rec_rows(rec, w.ids)), bits(exp)), k
        seen_two = seen_two or int(table["frames_evaluated"].max()) >= 2
    assert seen_two
    h.close()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. capacity
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_is_all_or_nothing(three):
    from continuous_clustering_amd import capi
    w = three
    e, twin = w.engine(), w.engine()
    h, ht = batched_for(w, e), batched_for(w, twin)
    for f in range(2):
        feed(w, e, h, f)
        feed(w, twin, ht, f)
        if f == 0:
            step_ok(h)
            step_ok(ht)
    need = len(w.want_step(1))
    assert need >= 2
    rc, rec, n, table = h.step(capacity=0)
    assert rc == capi.CC_ERR_CAPACITY and n == need and len(rec) == 0
    assert [int(v) for v in table["frames_evaluated"]] == [len(w.want[s][1]) for s in range(w.S)]
    rc2, _, n2, table2 = h.step(capacity=need - 1)
    assert rc2 == capi.CC_ERR_CAPACITY and n2 == need
    assert np.array_equal(table2["col_from"], table["col_from"]) and np.array_equal(table2["previous_frame"], table["previous_frame"])
    rec3, table3 = step_ok(h, capacity=need)
    rect, tablet = step_ok(ht)
    assert np.array_equal(table3["col_from"], table["col_from"])            # no cursor moved
    assert rec3.tobytes() == rect.tobytes() and table3.tobytes() == tablet.tobytes()
    assert np.array_equal(bits(rec_rows(rec3, w.ids)), bits(w.want_step(1)))
    for x in (h, ht, e, twin):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the two errors, by seek
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_errors_by_seek(three):
    from continuous_clustering_amd import evaluation
    w = three
    e = w.engine()
    h = batched_for(w, e)
    got = [[] for _ in range(w.S)]

    def collect(rec):
        for r in rec_rows(rec, w.ids):
            got[w.ids.index(r[0])].append(r)

    def others_as_expected(rec, k):
        rows = [r for r in rec_rows(rec, w.ids) if r[0] != w.ids[1]]
        assert np.array_equal(bits(rows), bits(w.want_step(k, streams=(0, 2)))), k

    for f in range(2):
        feed(w, e, h, f)
        rec, table = step_ok(h)
        collect(rec)
    cursor, prev = int(table["col_to"][1]), int(table["previous_frame"][1])
    assert prev == 1
    # ALREADY_EVALUATED: the columns behind the cursor hold frames 1 and 2, previous_frame says 3
    h.seek(1, cursor, 3)
    feed(w, e, h, 2)
    rec, table = step_ok(h)
    others_as_expected(rec, 2)
    collect(rec)
    assert table["error"][1] == evaluation.REPLAY_ERR_ALREADY_EVALUATED and table["error_column"][1] == cursor
    assert table["frames_evaluated"][1] == 0 and table["col_to"][1] == cursor and not table["error"][[0, 2]].any()
    rec, table = step_ok(h)                                               # it persists, nothing else happens
    assert len(rec) == 0 and table["error"][1] == evaluation.REPLAY_ERR_ALREADY_EVALUATED and table["error_column"][1] == cursor
    h.seek(1, cursor, prev)                                               # consistent again: the delayed record arrives
    rec, table = step_ok(h)
    assert not table["error"].any() and (table["error_column"] == -1).all()
    collect(rec)
    assert np.array_equal(bits(got[1]), bits([r for k in range(3) for r in w.want[1][k]]))
    # TOO_FAR_AHEAD: previous_frame -1 while frames 2 and 3 are being published
    cursor, prev = int(table["col_to"][1]), int(table["previous_frame"][1])
    feed(w, e, h, 3)                                                      # (before the seek: add_frame refuses frame 3 at previous_frame -1)
    h.seek(1, cursor, -1)
    rec, table = step_ok(h, finish=[1, 1, 1])                             # (finish is ignored for the stream with the error)
    others_as_expected(rec, 3)
    collect(rec)
    assert table["error"][1] == evaluation.REPLAY_ERR_TOO_FAR_AHEAD and table["error_column"][1] == cursor
    assert table["active"][1] == 1 and not table["active"][[0, 2]].any()
    rec, table = step_ok(h)
    assert len(rec) == 0 and table["error"][1] == evaluation.REPLAY_ERR_TOO_FAR_AHEAD
    h.seek(1, cursor, prev)
    rec, table = step_ok(h, finish=[0, 1, 0])
    assert not table["error"].any()
    collect(rec)
    for s in range(w.S):
        assert np.array_equal(bits(got[s]), bits([r for k in range(w.nframes) for r in w.want[s][k]])), s
    # the Python surface raises the reference's messages
    e2 = w.engine()
    sc = evaluation.BatchedFrameScatter(e2, w.ids, w.sds[0].n_points, rows=w.rows, cols=w.cols, eval_lanes=2)
    for f in range(3):
        for s, sd in enumerate(w.sds):
            sc.add_frame(s, f, sd.sem[f], sd.eu[f])
            upload(sc.original_index_ptr(s, f), sd.org[f])
        e2.add_firings_device(w.cols, *w.dev(f))
        if f < 2:
            sc.publish()
    assert [len(r) for r in sc.records] == [len(w.want[s][0]) + len(w.want[s][1]) for s in range(w.S)]
    cursor = int(sc.last_table["col_to"][1])                              # behind it: the rest of frame 1, then frame 2
    sc.h.seek(1, cursor, 3)
    with pytest.raises(RuntimeError, match="already evaluated"):
        sc.publish()
    sc.h.seek(1, cursor, -1)
    with pytest.raises(RuntimeError, match="too far ahead"):
        sc.publish()
    assert set(sc.counters()) == {"steps", "kernel_launches", "host_syncs", "eval_rounds"} and sc.counters()["steps"] == 4
    for x in (sc, e2, h, e):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. with cc_engine_reset_streams
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_with_reset_streams(three):
    """Behind step 1 stream 1 is reset and starts another sequence from frame 0; streams 0 and 2 go on."""
    import torch
    from continuous_clustering_amd import synth
    from oracle import pyoracle
    w = three
    other = StreamData(w.rows, w.cols, 2, seed=501, motion=synth.Motion.translate(3.0), sequence=99)
    # stream 1's own expectation: its oracle after reset() (the same object keeps the inclination table, as the engine's stream does)
    o = pyoracle.Oracle(w.cfg, w.rows, IDENTITY)
    first = oracle_steps(w.cfg, w.sds[1], [[0], [1]], finish_last=False, oracle=o)
    o.reset()
    o.set_robot_from_sensor(IDENTITY)
    second = oracle_steps(w.cfg, other, [[0], [1]], finish_last=True, oracle=o)
    e = w.engine()
    h = batched_for(w, e)
    ids = list(w.ids)
    for f in range(w.nframes):
        if f < 2:
            feed(w, e, h, f)
        else:
            g = f - 2
            for s in (0, 2):
                h.add_frame(s, f, w.sds[s].sem[f], w.sds[s].eu[f])
                upload(h.original_index_ptr(s, f), w.sds[s].org[f])
            h.add_frame(1, g, other.sem[g], other.eu[g])
            upload(h.original_index_ptr(1, g), other.org[g])
            parts = [w.sds[0].frame(f), other.frame(g), w.sds[2].frame(f)]
            t = [torch.from_numpy(np.stack([p[k] for p in parts])).cuda() for k in range(3)]
            torch.cuda.synchronize()
            e.add_firings_device(w.cols, *t)
            assert e.sync() == 0, e.last_error()
        rec, table = step_ok(h, finish=[1] * w.S if f == w.nframes - 1 else None)
        rows = rec_rows(rec, ids)
        mine = (first[f] if f < 2 else second[f - 2])
        exp = list(w.want[0][f]) + list(mine) + list(w.want[2][f])
        assert np.array_equal(bits(rows), bits(exp)), f
        if f == 1:
            e.reset_streams([1])
            e.set_robot_from_sensor(IDENTITY, stream=1)
            h.seek(1, 0, 0)
            ids[1] = other.sequence
    assert len(second[0]) + len(second[1]) == 2
    h.close()
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. launch counts do not depend on the number of streams
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_depend_on_streams(three):
    w = three
    per_step = {}
    for S in (2, 5):
        sds = [w.sds[s % 2] for s in range(S)]
        e = w.engine(S)
        h = batched_for(w, e, sds=sds, eval_lanes=8)
        steps = []
        for f in range(2):
            feed(w, e, h, f, sds=sds)
            c0 = h.counters()
            rec, table = step_ok(h)
            c1 = h.counters()
            d = {k: c1[k] - c0[k] for k in c0}
            longest = int((table["col_to"] - table["col_from"]).max())
            rounds = -(-len(rec) // 8)
            # the formula of include/cc_kitti.h
            assert d["steps"] == 1 and d["eval_rounds"] == rounds
            assert d["kernel_launches"] == 3 + (2 if longest > 0 else 0) + 2 * rounds
            assert d["host_syncs"] == 2 + rounds
            steps.append((d["kernel_launches"], d["host_syncs"], d["eval_rounds"]))
            assert len(rec) == sum(len(w.want[s % 2][f]) for s in range(S))
        per_step[S] = steps
        h.close()
        e.close()
    assert per_step[2] == per_step[5]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. the KITTI path
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_kitti_replay_batched_equals_device_and_oracle(tmp_path, oracle_lib):
    from continuous_clustering_amd import kitti, replay
    from continuous_clustering_amd.evaluation import gather_records
    from test_gpu_kitti_replay import expected_records
    lengths = {2: 3, 4: 2}
    want = {}
    for k, (seq, nf) in enumerate(lengths.items()):
        seq_dir, _ = kitti.write_synthetic_sequence(str(tmp_path), seq, nf, seed=700 + 10 * k, motion=(6.0 + k, 0.1 * k, 0.0, 0.1 * (k + 1)),
                                                    cols_per_row=520)
        sc, _, _ = expected_records(seq_dir, seq, nf)
        sc.finish()
        want[seq] = np.array(sc.records)
    allwant = np.concatenate([want[s] for s in sorted(want)])
    batched, totals = replay.replay(str(tmp_path), list(lengths), scatter="batched")
    device, totals_d = replay.replay(str(tmp_path), list(lengths))
    assert totals == totals_d and totals["streams"] == 2 and totals["frames"] == 5
    b, d = gather_records(batched), gather_records(device)
    assert b.shape == d.shape == allwant.shape
    assert np.array_equal(b.view(np.uint64), d.view(np.uint64))
    assert np.array_equal(b.view(np.uint64), allwant.view(np.uint64))
    r0, _ = replay.replay(str(tmp_path), list(lengths), rank=0, world=2, scatter="batched")
    r1, _ = replay.replay(str(tmp_path), list(lengths), rank=1, world=2, scatter="batched")
    assert {int(r[0]) for r in r0} == {2} and {int(r[0]) for r in r1} == {4}
    both = gather_records(list(r0) + list(r1))
    assert np.array_equal(both.view(np.uint64), allwant.view(np.uint64))
