"""Scripts for tests/cpp/dropin_script.cpp: lists of operations that ONE continuous_clustering::ContinuousClustering object and ONE oracle object
go through — resets, configuration and transform changes between two firings, batching modes, enough firings to wrap the class's mirror ring and
to trim its firing log, and inputs that make it throw. Everything is built from the tables of cases.py and reconfigure_streams.py.

An operation is a tuple: ("CONFIG", capi.Config), ("RESET", rows), ("TRANSFORM", tf12), ("BATCH", b), ("FLUSH",), ("FIRINGS", stream, a, b), ("QUERY",).
tests/test_dropin_scripts_cpu.py holds every script to its purpose on the oracle; tests/test_gpu_dropin_scripts.py runs the class on them."""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass, field

import numpy as np

import cases
import reconfigure_streams as rs
from continuous_clustering_amd import capi, synth
from continuous_clustering_amd.synth import Motion, SensorModel

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
CONFIG_FIELDS = [n for n, _ in capi.Config._fields_]       # the 33 fields toPod copies, in the order of the CONFIG record
CODES = {"CONFIG": 1, "RESET": 2, "TRANSFORM": 3, "BATCH": 4, "FLUSH": 5, "FIRINGS": 6, "QUERY": 7}
MAGIC = 0x31435344
# what the reference appends to the oracle's sentence (cc_oracle.cpp:459) in its exception (continuous_clustering.cpp:343-344)
OVERRUN_TAIL = ("; This typically happens when the clustering is not fast enough to handle all the firings. Consider "
                "to play the sensor data more slowly or to adjust the parameters to make the clustering faster.")

LONG_ROTATIONS = 48
LONG_COLUMNS = 256
OVERRUN_FIRINGS = 3000
RESET_AT = rs.SWITCH_AT[0]     # 397: mid-rotation


# ---- streams -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_stream():
    """w_s32_256x12's sensor, motion and configuration over 48 rotations + 40 firings."""
    sen = SensorModel(num_rows=32, num_columns=LONG_COLUMNS, incl_top_deg=10.0, incl_bottom_deg=-30.0)
    return synth.make_stream(LONG_COLUMNS * LONG_ROTATIONS + 40, seed=45, sensor=sen, motion=Motion.translate()), cases._vls(LONG_COLUMNS, max_distance=0.5)


@functools.lru_cache(maxsize=None)
def _built(name):
    return cases.build_case(name)


def _with(cfg, **over):
    c = cfg.copy()
    for k, v in over.items():
        setattr(c, k, v)
    return c


# ---- operations --------------------------------------------------------------------------------------------------------------------------------
def _start(cfg, rows, tf=None):
    return [("CONFIG", cfg), ("RESET", rows), ("QUERY",), ("TRANSFORM", IDENTITY if tf is None else tf)]


def _end():
    return [("FLUSH",), ("QUERY",)]


def stream_ops(stream, cfg, tf=None):
    return _start(cfg, stream.sensor.num_rows, tf) + [("FIRINGS", stream, 0, stream.n_firings)] + _end()


def schedule_ops(stream, schedule):
    """A schedule of util.schedule_oracle_record as operations: the change goes in front of the segment's firings."""
    ops, f = [], 0
    for k, (n, cfg, tf) in enumerate(schedule):
        if k == 0:
            ops += _start(cfg, stream.sensor.num_rows, tf)
        else:
            if cfg is not None:
                ops.append(("CONFIG", cfg))
            if tf is not None:
                ops.append(("TRANSFORM", tf))
        ops.append(("FIRINGS", stream, f, f + n))
        f += n
    return ops + _end()


def _case_ops(name):
    return stream_ops(*_built(name))


def _shape_ops(name):
    (first, cfg1), (second, cfg2) = rs.shape_case(name)
    return (stream_ops(first, cfg1) + [("CONFIG", cfg2), ("QUERY",), ("RESET", second.sensor.num_rows), ("QUERY",), ("TRANSFORM", IDENTITY),
                                        ("FIRINGS", second, 0, second.n_firings)] + _end())


def _reset_same_shape_ops():
    stream, cfg = rs.case_stream(rs.RING_CASE), rs.case_config(rs.RING_CASE)
    rows = stream.sensor.num_rows
    return (_start(cfg, rows) + [("FIRINGS", stream, 0, RESET_AT), ("FLUSH",), ("QUERY",), ("RESET", rows), ("QUERY",), ("TRANSFORM", IDENTITY),
                                 ("FIRINGS", stream, RESET_AT, stream.n_firings)] + _end())


def _threading_switch_ops():
    """is_single_threaded 1 -> 0 -> 1 on the same object: reset_required after each setConfiguration, a worker started and stopped by reset."""
    stream, cfg, _ = _built("g_s64_translate")
    rows, ops = stream.sensor.num_rows, []
    for k, single in enumerate((1, 0, 1)):
        c = _with(cfg, is_single_threaded=single)
        ops += [("CONFIG", c)] + ([("QUERY",)] if k else []) + [("RESET", rows), ("QUERY",), ("TRANSFORM", IDENTITY), ("FIRINGS", stream, 0, stream.n_firings)] + _end()
    return ops


def _no_transform_ops():
    """Firings before any transform, after construction and after a reset; each error is followed by a reset and a clean segment."""
    stream, cfg, _ = _built("g_s64_translate")
    rows = stream.sensor.num_rows
    ops = []
    for k in range(2):
        ops += [("CONFIG", cfg), ("RESET", rows), ("QUERY",), ("FIRINGS", stream, 0, 200), ("FLUSH",), ("QUERY",)]
        ops += [("RESET", rows), ("TRANSFORM", IDENTITY), ("FIRINGS", stream, 0, 500)] + _end()
    return ops


def _overrun_ops():
    """cluster_point_trees_every_nth_column beyond the ring on the first firings of `long`: nothing is published or cleared and the eleventh rotation
    runs into its own tail (tests/test_gpu_ringwrap.py::test_deliberate_ring_overrun). Then reset, transform and a clean segment."""
    stream, cfg = long_stream()
    rows = stream.sensor.num_rows
    bad = _with(cfg, cluster_point_trees_every_nth_column=100000)
    return (_start(bad, rows) + [("FIRINGS", stream, 0, OVERRUN_FIRINGS), ("FLUSH",), ("QUERY",), ("CONFIG", cfg), ("RESET", rows), ("TRANSFORM", IDENTITY),
                                 ("FIRINGS", stream, 0, 3 * LONG_COLUMNS + 40)] + _end())


REST_OF_THE_FIELDS = dict(terrain_max_allowed_z_diff=0.05, use_last_point_for_cluster_stamp=1, supplement_inclination_angle_for_nan_cells=0)


def _rest_of_the_fields_ops(**over):
    """What no table of cases.py or reconfigure_streams.py does: terrain_max_allowed_z_diff changes (with use_terrain on);
    supplement_inclination_angle_for_nan_cells changes without ignore_points_with_too_big_inclination_angle_diff, the one pair of fields that
    holds equal values in every other script; and use_last_point_for_cluster_stamp once more, on a stream with many cluster callbacks."""
    stream, cfg, _ = _built("p_s64_terrain_gaps")
    other = _with(cfg, **{**REST_OF_THE_FIELDS, **over})
    return schedule_ops(stream, rs.cut(stream.n_firings, rs.SWITCH_AT[:1], [(cfg, None), (other, None)]))


def _walk_ops():
    stream, schedule, _ = rs.walk_schedule(*rs.WALKS[0])
    return schedule_ops(stream, schedule)


# name -> (operations, batch modes the GPU test runs it in: n > 0 setBatchSize(n), -1 the asynchronous mode, None as the script says)
SCRIPTS = {
    "long": (lambda: stream_ops(*long_stream()), (1, 97, -1)),
    "in_r_mixed": (lambda: _case_ops("r_mixed__w_s64_240x13"), (97,)),
    "in_jitter_wide": (lambda: _case_ops("j_s64_jitter_wide"), (1,)),
    "in_counterclockwise": (lambda: _case_ops("s64_counterclockwise"), (61,)),
    "in_fog_and_ego": (lambda: _case_ops("g_s64_fog_and_ego"), (-1,)),
    "in_forced_finish_ring": (lambda: _case_ops("s64_forced_finish_ring"), (1, 97)),
    "cfg_everything": (lambda: schedule_ops(*rs.threshold_schedule("everything")[:2]), (97,)),
    **{"cfg_" + sw: ((lambda sw=sw: schedule_ops(*rs.association_schedule(sw, rs.RING_CASE)[:2])), (b,))
       for sw, b in zip(rs.ASSOCIATION_SWITCHES, (97, 1, 61, 97, 1))},
    # (on the wall ring the two window limits change nothing in the output: the same switch where 4 -> 40 -> 4 shows)
    "cfg_steps_in_row_4_40_4_profiles": (lambda: schedule_ops(*rs.association_schedule("steps_in_row_4_40_4", rs.BASE_CASE)[:2]), (61,)),
    "cfg_ego_both": (lambda: schedule_ops(*rs.ego_schedule("both")[:2]), (1, -1)),
    "cfg_walk": (_walk_ops, (97,)),
    "cfg_rest_of_the_fields": (_rest_of_the_fields_ops, (97,)),
    **{"reset_" + n: ((lambda n=n: _shape_ops(n)), (b,)) for n, b in zip(rs.SHAPE_CASES, (97, 1, -1, 97))},
    "reset_same_shape": (_reset_same_shape_ops, (1, -1)),
    "reset_threading_switch": (_threading_switch_ops, (None,)),
    "err_no_transform": (_no_transform_ops, (1, -1)),
    "err_ring_overrun": (_overrun_ops, (1, 97, -1)),     # (97: the failing engine call holds firings behind the one the oracle stops at)
}
ERROR_SCRIPTS = ("err_no_transform", "err_ring_overrun")


@functools.lru_cache(maxsize=None)
def script_ops(name):
    return tuple(SCRIPTS[name][0]())


def with_batch(ops, batch):
    """The operations in a batch mode: -1 = is_single_threaded off in every configuration (the reference's default: the asynchronous mode), n > 0 = a
    BATCH operation behind the first reset."""
    if batch is None:
        return list(ops)
    out, done = [], False
    for op in ops:
        if op[0] == "CONFIG":
            op = ("CONFIG", _with(op[1], is_single_threaded=0 if batch < 0 else 1))
        out.append(op)
        if op[0] == "RESET" and not done and batch > 0:
            out.append(("BATCH", batch))
            done = True
    return out


def n_firings(ops):
    return sum(op[3] - op[2] for op in ops if op[0] == "FIRINGS")


# ---- the input file ------------------------------------------------------------------------------------------------------------------------------
def write_script(path, ops):
    segment, fed = -1, 0
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", MAGIC, len(ops)))
        for op in ops:
            f.write(struct.pack("<i", CODES[op[0]]))
            if op[0] == "CONFIG":
                f.write(np.array([getattr(op[1], n) for n in CONFIG_FIELDS], dtype=np.float64).tobytes())
            elif op[0] == "RESET":
                f.write(struct.pack("<i", op[1]))
                segment, fed = segment + 1, 0
            elif op[0] == "TRANSFORM":
                f.write(np.asarray(op[1], dtype=np.float64).reshape(12).tobytes())
            elif op[0] == "BATCH":
                f.write(struct.pack("<i", op[1]))
            elif op[0] == "FIRINGS":
                _, st, a, b = op
                f.write(struct.pack("<iiii", b - a, st.sensor.num_rows, max(segment, 0), fed))
                f.write(np.ascontiguousarray(st.xyz[a:b], dtype=np.float32).tobytes())
                f.write(np.ascontiguousarray(st.intensity[a:b], dtype=np.uint8).tobytes())
                f.write(np.ascontiguousarray(st.poses[a:b], dtype=np.float64).tobytes())
                fed += b - a


# ---- the dump --------------------------------------------------------------------------------------------------------------------------------------
PUBLISHED_CELL = np.dtype([("id", "<u8"), ("globally_unique_point_index", "<u8"), ("stamp", "<u8"), ("firing_index", "<u8"), ("tree_id", "<u8"),
                           ("global_column_index", "<i8"), ("tree_root_column", "<i8"), ("continuous_azimuth_angle", "<f8"),
                           ("finished_at_continuous_azimuth_angle", "<f8"), ("xyz", "<f4", 3), ("distance", "<f4"), ("inclination_angle", "<f4"),
                           ("azimuth_angle", "<f4"), ("local_column_index", "<i4"), ("row_index", "<i4"), ("tree_root_row", "<i4"),
                           ("number_of_visited_neighbors", "<i4"), ("tree_num_points", "<u4"), ("cluster_width", "<u4"), ("n_child_points", "<u4"),
                           ("n_associated_trees", "<u4"), ("ground_point_label", "u1"), ("debug_ground_point_label", "u1"), ("is_ignored", "u1"),
                           ("intensity", "u1"), ("belongs_to_finished_cluster", "u1")])
LIST_ENTRY = np.dtype([("column_index", "<i8"), ("row_index", "<i4")])
GROUND_CELL = np.dtype([("globally_unique_point_index", "<u8"), ("stamp", "<u8"), ("firing_index", "<u8"), ("global_column_index", "<i8"),
                        ("xyz", "<f4", 3), ("distance", "<f4"), ("inclination_angle", "<f4"), ("azimuth_angle", "<f4"), ("row_index", "<i4"),
                        ("ground_point_label", "u1"), ("debug_ground_point_label", "u1"), ("is_ignored", "u1"), ("intensity", "u1")])
CLUSTER_MEMBER = np.dtype([("id", "<u8"), ("stamp", "<u8"), ("globally_unique_point_index", "<u8"), ("global_column_index", "<i8"), ("row_index", "<i4")])
assert (PUBLISHED_CELL.itemsize, LIST_ENTRY.itemsize, GROUND_CELL.itemsize, CLUSTER_MEMBER.itemsize) == (133, 12, 64, 36)


@dataclass
class DumpSegment:
    """What the callbacks of one reset-to-reset segment showed."""
    rows: int
    order: list = field(default_factory=list)          # (1, column, column) | (2, id, size) | (3, from, to) in callback order
    published: list = field(default_factory=list)      # (from, to, cells [columns, rows], child entries, associated-tree entries)
    ground: list = field(default_factory=list)         # (column, cells [rows])
    clusters: list = field(default_factory=list)       # (stamp, members)


@dataclass
class Dump:
    segments: list
    queries: dict        # operation index -> dict
    exceptions: list     # (operation index, firing index or -1, what())
    counts: tuple        # ground callbacks, cluster callbacks, ground-view violations


def parse_dump(path, ops):
    data = open(path, "rb").read()
    pos, rows = 0, -1
    seg = DumpSegment(rows)
    out = Dump([seg], {}, [], None)
    while pos < len(data):
        (tag,) = struct.unpack_from("<i", data, pos)
        pos += 4
        if tag in (1, 4):
            frm, to = struct.unpack_from("<qq", data, pos)
            pos += 16
            ncol = max(0, to - frm + 1)
            if tag == 4:
                cells = np.frombuffer(data, dtype=GROUND_CELL, count=rows, offset=pos)
                pos += rows * GROUND_CELL.itemsize
                seg.ground.append((frm, cells))
                seg.order.append((1, frm, to))
                continue
            cells = np.frombuffer(data, dtype=PUBLISHED_CELL, count=ncol * rows, offset=pos).reshape(ncol, rows)
            pos += cells.size * PUBLISHED_CELL.itemsize
            lists = []
            for key in ("n_child_points", "n_associated_trees"):
                n = int(cells[key].sum(dtype=np.int64))
                lists.append(np.frombuffer(data, dtype=LIST_ENTRY, count=n, offset=pos))
                pos += n * LIST_ENTRY.itemsize
            seg.published.append((frm, to, cells, lists[0], lists[1]))
            seg.order.append((3, frm, to))
        elif tag == 2:
            cnt, stamp = struct.unpack_from("<QQ", data, pos)
            pos += 16
            members = np.frombuffer(data, dtype=CLUSTER_MEMBER, count=cnt, offset=pos)
            pos += cnt * CLUSTER_MEMBER.itemsize
            seg.clusters.append((stamp, members))
            seg.order.append((2, int(members["id"][0]) if cnt else 0, cnt))
        elif tag == 3:
            out.counts = struct.unpack_from("<qqq", data, pos)
            pos += 24
        elif tag == 5:
            op, req, has, nr, nc, ring, start, end = struct.unpack_from("<iiiiiiqq", data, pos)
            pos += 40
            out.queries[op] = dict(reset_required=req, has_transform=has, num_rows=nr, num_columns=nc, ring_buffer_max_columns=ring,
                                   ring_buffer_start_global_column_index=start, ring_buffer_end_global_column_index=end)
        elif tag == 6:
            op, firing, ln = struct.unpack_from("<iqi", data, pos)
            pos += 16
            out.exceptions.append((op, firing, data[pos:pos + ln].decode()))
            pos += ln
        elif tag == 7:
            op, code = struct.unpack_from("<ii", data, pos)
            pos += 8
            assert code == CODES[ops[op][0]], (op, code, ops[op][0])
            if code == CODES["RESET"]:
                rows = ops[op][1]
                if seg.rows < 0 and not seg.order:
                    seg.rows = rows          # (the first reset opens the first segment)
                else:
                    seg = DumpSegment(rows)
                    out.segments.append(seg)
        else:
            raise AssertionError(f"bad tag {tag} at byte {pos - 4}")
    return out


# ---- the oracle through the same operations ----------------------------------------------------------------------------------------------------
@dataclass
class OracleSegment:
    rows: int
    num_columns: int
    events: np.ndarray
    use_last: np.ndarray            # per event: use_last_point_for_cluster_stamp of the configuration in force when it was emitted
    published_range: tuple          # (from, to), to < from: nothing
    published: dict                 # read_published of that range (None: nothing)
    members: list                   # per cluster event with a callback (> 20 points): (global columns, rows) in the reference's order
    xyz: np.ndarray                 # the raw returns fed in this segment [firings, rows, 3]
    intensity: np.ndarray
    state: dict                     # at the segment's end
    error: tuple = None             # (operation index, firing index in the segment, status, last_error())


def oracle_record(ops):
    """The oracle object through `ops`: (segments, expected QUERY records by operation index). Events and the published record are read before every
    reset, which drops them."""
    from oracle.pyoracle import Oracle
    o, cfg, rows = None, None, None
    segments, queries = [], {}
    events, flags, xyz, inten = [], [], [], []
    has_tf, failed = False, None

    def close_segment():
        ev = np.concatenate(events) if events else np.zeros(0, dtype=capi.EVENT_DTYPE)
        lo, hi = o.published_range()
        all_cl = ev[ev["type"] == capi.EV_CLUSTER]
        members = [o.cluster_members(k) for k, e in enumerate(all_cl) if e["d"] > 20]
        st = o.state()
        segments.append(OracleSegment(rows, st["num_columns"], ev, np.concatenate(flags) if flags else np.zeros(0, dtype=bool), (lo, hi),
                                      o.read_published(lo, hi) if hi >= lo and lo >= 0 else None, members,
                                      np.concatenate(xyz) if xyz else np.zeros((0, rows, 3), np.float32),
                                      np.concatenate(inten) if inten else np.zeros((0, rows), np.uint8), st, failed))
        for lst in (events, flags, xyz, inten):
            lst.clear()

    for k, op in enumerate(ops):
        if op[0] == "CONFIG":
            cfg = op[1]
            if o is not None:
                o.set_config(cfg)
        elif op[0] == "RESET":
            if o is None:
                o = Oracle(cfg, op[1], None)
            else:
                close_segment()
                o.reset(op[1])
            rows, has_tf, failed = op[1], False, None
        elif op[0] == "TRANSFORM":
            o.set_robot_from_sensor(op[1])
            has_tf = True
        elif op[0] == "FIRINGS":
            _, st, a, b = op
            if failed is None:
                rc = o.add_firings(st.xyz[a:b], st.intensity[a:b], st.poses[a:b])
                ev = o.drain_events()
                events.append(ev)
                flags.append(np.full(len(ev), bool(cfg.use_last_point_for_cluster_stamp)))
                xyz.append(np.asarray(st.xyz[a:b], dtype=np.float32))
                inten.append(np.asarray(st.intensity[a:b], dtype=np.uint8))
                if rc != 0:
                    failed = (k, int(o.state()["firings_consumed"]), rc, o.last_error())
        elif op[0] == "QUERY":
            s = o.state()
            queries[k] = dict(reset_required=int(s["reset_required"]), has_transform=int(has_tf), num_rows=s["num_rows"],
                              num_columns=s["num_columns"], ring_buffer_max_columns=s["ring_buffer_max_columns"],
                              ring_buffer_start_global_column_index=s["ring_buffer_start_global_column_index"],
                              ring_buffer_end_global_column_index=s["ring_buffer_end_global_column_index"], failed=failed is not None)
    close_segment()
    return segments, queries


@functools.lru_cache(maxsize=None)
def script_record(name):
    """oracle_record of a script, made once and read-only afterwards (the batch mode does not change it)."""
    return oracle_record(script_ops(name))


def expected_cluster_stamp(stamps, use_last):
    """cc.cpp:1025-1028 from the members' own stamps."""
    lo, hi = int(stamps.min()), int(stamps.max())
    return hi if use_last else lo + (hi - lo) // 2
