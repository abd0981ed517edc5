"""GPU: cc_engine_set_config and cc_engine_set_robot_from_sensor in mid-stream — engine against oracle under the schedules of
reconfigure_streams.py, bit-exact through util.run_schedule_and_compare (events field by field, published columns, state; no tolerances).

The engine keeps configuration outside cc_engine::cfg: the captured small-call graphs and the resident kernel get it at capture / launch,
Geometry::max_distance_squared is a copy, StreamState::assoc_mode is derived from max_steps_in_row, cluster_point_trees_every_nth_column selects
the association kernel family and the lean small call, the fused front of k_insert_par stages seg_pre_cells output that depends on the fog, ego-box
and max_distance fields and on the k_ego record made from robot_from_sensor (k_seg_scan reads it later), and a pipelined call leaves chains to the
next call that must run under the old configuration. A change between two calls must leave none of them stale. The paths are those of
tests/test_gpu_segmentation_sweep.py (PATHS and what its docstring says about each), with the same debug-counter assertions per path.
tests/test_reconfigure_cases_cpu.py shows on the oracle that every schedule changes what is computed."""
import numpy as np
import pytest

import cases
import reconfigure_streams as rs
import util
from continuous_clustering_amd import capi
from test_gpu_segmentation_sweep import ALL_SMALL_ROW_PATHS, PATHS, SMALL, debug_counters

pytestmark = pytest.mark.gpu

IDENTITY = rs.TRANSFORM_TABLE["identity"]
_oracles = {}


def oracle_of(key, stream, schedule):
    """One oracle run per schedule and module; it is only read afterwards."""
    if key not in _oracles:
        _oracles[key] = util.schedule_oracle_record(stream, schedule)
    return _oracles[key]


def run_schedule(key, stream, schedule, path="fused", options=None, chunks=None, after_switch=None, check_counters=True):
    """The schedule on one path of PATHS (options on top of the path's, chunks instead of the path's); the debug-counter assertions are those of
    test_gpu_segmentation_sweep.run_path. Returns (summary, engine): the caller closes the engine."""
    opts, path_chunks = PATHS[path]
    opts = dict(opts, **(options or {}))
    small = chunks is None and path_chunks == SMALL
    if chunks is None:
        chunks = path_chunks or [stream.sensor.num_columns, 97]

    def setup(e):
        for k, v in opts.items():
            e.set_option(k, v)

    summary = util.run_schedule_and_compare(stream, schedule, chunks, engine_setup=setup, oracle=oracle_of(key, stream, schedule), after_switch=after_switch)
    e = summary["engine"]
    assert summary["published_columns"] > stream.n_firings // 2
    if check_counters:
        dbg = debug_counters(e)
        if path in ("fused", "scan_rows") and "parallel_insert" not in opts:
            assert dbg[7] > 0, dbg
            if stream.sensor.num_rows <= 64:
                assert dbg[4] > 0, dbg
        elif path == "seg_pre":
            assert dbg[4] == 0 and dbg[7] > 0, dbg
        elif path == "serial" or small:
            assert dbg[4] == 0 and dbg[7] == 0, dbg
    return summary, e


# ---- a. thresholds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "serial", "small_all"])
@pytest.mark.parametrize("entry", rs.THRESHOLD_ENTRIES)
def test_threshold_there_and_back(entry, path, oracle_lib):
    """base -> entry -> base at firings 397 and 611 of p_s64_profiles: columns inserted (and, fused, staged by seg_pre_cells) under one configuration
    are segmented under the next, trees opened under one window are continued under another."""
    stream, schedule, _ = rs.threshold_schedule(entry)
    run_schedule(("t", entry), stream, schedule, path)[1].close()


@pytest.mark.parametrize("path", [p for p in ALL_SMALL_ROW_PATHS if p not in ("fused", "serial", "small_all")])
@pytest.mark.parametrize("entry", rs.EVERYTHING_ENTRIES)
def test_everything_there_and_back_on_the_other_paths(entry, path, oracle_lib):
    stream, schedule, _ = rs.threshold_schedule(entry)
    run_schedule(("t", entry), stream, schedule, path)[1].close()


# ---- b. association family -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [None, [37, 5, 211]], ids=["columns_97", "37_5_211"])
@pytest.mark.parametrize("options", [{}, {"assoc_batch": 0, "assoc_waves": 1}, {"assoc_batch": 0, "assoc_waves": 3}], ids=["default", "lds", "assoc3"])
@pytest.mark.parametrize("name", rs.ASSOCIATION_CASES)
@pytest.mark.parametrize("switch", list(rs.ASSOCIATION_SWITCHES))
def test_association_family_switch(switch, name, options, chunks, oracle_lib):
    """every-nth-column 1 -> 2 -> 1 (another kernel family, the small call no longer lean), max_steps_in_row 20 -> 40 -> 20 and 4 -> 40 -> 4 (beyond
    the LDS window: assoc_mode goes up, and parity must hold after the value is back), the early stop off and on, the stamp flag (nothing but what
    set_config itself does) — on the profile columns and on the wall ring, whose trees are open at every switch; the batch-parallel kernel in front
    (default), k_assoc_lds and k_assoc3 alone."""
    stream, schedule, _ = rs.association_schedule(switch, name)
    run_schedule(("a", switch, name), stream, schedule, "fused", options, chunks, check_counters=False)[1].close()


# ---- c. ego box and transform -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "seg_pre", "small_all"])
@pytest.mark.parametrize("switch", list(rs.EGO_SWITCHES))
def test_ego_box_and_transform_switch(switch, path, oracle_lib):
    """p_s64_profiles under the moving pose: the transform alone (identity -> ahead and above -> tilted), the box alone, both at once. The k_ego
    record of a firing is made from the transform and the box of the call that inserts it."""
    stream, schedule, _ = rs.ego_schedule(switch)
    run_schedule(("e", switch), stream, schedule, path)[1].close()


@pytest.mark.parametrize("chunks", [[1, 3], [17, 63]], ids=["graphs_1_3", "direct_17_63"])
@pytest.mark.parametrize("switch", ["tf", "both"])
def test_ego_switch_between_small_calls(switch, chunks, oracle_lib):
    """Calls of 1 and 3 firings on both sides of the switches run as captured graphs, which bake the configuration (destroy_small_graphs); calls of
    17 and 63 as direct launches of k_small_all."""
    stream, schedule, _ = rs.ego_schedule(switch)
    run_schedule(("e", switch), stream, schedule, "small_all", chunks=chunks, check_counters=False)[1].close()


@pytest.mark.parametrize("switch", ["tf", "both", "box_huge_box"])
def test_ego_switch_under_the_resident_kernel(switch, oracle_lib):
    """One-firing calls answered by the resident kernel, which got configuration and transform at its launch: a change stops it, and the next call
    runs under the new values (the comparison after every call)."""
    stream, schedule, _ = rs.ego_schedule(switch)
    stopped = []

    def after_switch(e, f):
        stopped.append(not e.resident_counters()["running"])

    s, e = run_schedule(("e", switch), stream, schedule, "small_all", {"resident": 1}, [1], after_switch, check_counters=False)
    c = e.resident_counters()
    e.close()
    assert stopped == [True] * (len(schedule) - 1), stopped
    assert c["launches"] >= len(schedule), c


# ---- d. a change before every call -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", rs.WALKS)
def test_a_change_before_every_call(name, seed, oracle_lib):
    """A seeded walk: before every call the next configuration from reconfigure_streams.CONFIG_TABLE, before every third a transform as well; calls
    of 1 .. 360 firings, events on. p_s128_profiles: two rows per lane."""
    stream, schedule, applied = rs.walk_schedule(name, seed)
    try:
        s = util.run_schedule_and_compare(stream, schedule, [stream.n_firings], oracle=oracle_of(("w", name, seed), stream, schedule))
    except AssertionError as ex:
        raise AssertionError(f"{ex}\napplied (first firing, firings, configuration, transform): {applied}") from None
    s["engine"].close()
    assert s["calls"] == len(schedule) and s["events"] > 0, applied


def test_randomised_sweep_with_reconfiguration(oracle_lib):
    """tools/stress_parity.py --reconfigure on a fixed seed range: random scenes, chunkings and association options, every case with two changes of
    configuration and one of the transform at random firings."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_parity.py"), "--reconfigure", "4", "9300"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "failures: 0" in r.stdout and r.stdout.count("reconfigured") == 4


# ---- e. pipelined, many streams ---------------------------------------------------------------------------------------------------------------------------
def _compare_with_schedule_oracles(e, streams, schedules):
    """The schedule-taking sibling of test_gpu_stress._compare_with_oracles: every stream's state and its last published columns against an oracle
    that ran the stream's schedule."""
    bad = []
    for s, (st, schedule) in enumerate(zip(streams, schedules)):
        o, rc, _ = util.schedule_oracle_record(st, schedule)
        assert rc == 0, o.last_error()
        so, se = o.state(), e.state(s)
        diff = {k: (so[k], se[k]) for k in util.STATE_FIELDS if so[k] != se[k]}
        if diff:
            bad.append((s, diff))
            continue
        hi = se["first_unpublished_global_column_index"] - 1
        lo = max(se["ring_buffer_start_global_column_index"], hi - 1200)
        try:
            util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo, mirror=False)
        except AssertionError as ex:
            bad.append((s, str(ex)[:200]))
    return bad


@pytest.mark.parametrize("lazy", [1, 0], ids=["lazy_gate_on", "lazy_gate_off"])
def test_pipelined_streams_reconfigured_between_calls(lazy, oracle_lib):
    """12 profile streams (the seeds of test_pipelined_profile_streams) through cc_engine_add_firings_device, three calls of 270 firings and no sync
    between them: set_config(everything) between calls 1 and 2, set_robot_from_sensor for four of the streams between calls 2 and 3. A pipelined
    call leaves chains to the next one (deferred tail, lazy gate); they must run under the configuration they were submitted under before it is
    replaced. That something was held back is a condition, not a measurement: at a switch, cc_engine_inputs_released reports fewer released than
    submitted calls immediately before the change. 12 streams meet it."""
    import torch
    from continuous_clustering_amd import Engine
    name, F, S = cases.SWEEP_BASE_CASE, 270, 12
    base, everything = cases.profile_config(name), cases.profile_config(name, **cases.EVERYTHING)
    moved = {2: cases.ROBOT_TF_AHEAD_ABOVE, 5: cases.ROBOT_TF_TILTED, 6: cases.ROBOT_TF_1M_UP, 11: cases.ROBOT_TF_TILTED}
    streams = [cases.profile_stream(name, seed=5000 + s) for s in range(S)]
    assert all(st.n_firings == 3 * F for st in streams)
    e = Engine(base, 64, S)
    e.record_events(False)
    if lazy:
        e.set_option("lazy_gate_from", 1)
    else:
        e.set_option("lazy_gate", 0)
        e.set_option("lazy_gate_from", 0)
    keep, held_back = [], []
    for b in range(3):
        if b > 0:
            held_back.append(e.inputs_released())
        if b == 1:
            e.set_config(everything)
        if b == 2:
            for s, tf in moved.items():
                e.set_robot_from_sensor(tf, stream=s)
        bufs = tuple(torch.from_numpy(np.stack([getattr(st, k)[b * F:(b + 1) * F] for st in streams])).cuda() for k in ("xyz", "intensity", "poses"))
        keep.append(bufs)
        torch.cuda.synchronize()
        e.add_firings_device(F, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())
    assert e.sync() == 0, e.last_error()
    assert e.inputs_released() == (3, 3)
    lazy_batches = e.gate_counters()["lazy_batches"]
    schedules = [[(F, base, None), (F, everything, None), (F, None, moved.get(s))] for s in range(S)]
    bad = _compare_with_schedule_oracles(e, streams, schedules)
    e.close()
    assert not bad, bad[:3]
    assert any(rel < sub for rel, sub in held_back), held_back
    if not lazy:
        assert lazy_batches == 0


# ---- f. changes that raise reset_required -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [None, SMALL], ids=["columns_97", "small"])
@pytest.mark.parametrize("field,value", [("is_single_threaded", 0), ("num_columns", 400), ("sensor_is_clockwise", 0)])
def test_carrying_on_without_the_reset(field, value, chunks, oracle_lib):
    """One of the three fields of cc.cpp:69-74 changed at firing 397 and the rest fed without a reset: status, error text, events, published columns
    and state (reset_required among its fields) equal the oracle's; the geometry stays at 360 columns until reset on both sides."""
    stream = rs.case_stream(rs.BASE_CASE)
    schedule = rs.cut(stream.n_firings, (397,), [(rs.case_config(rs.BASE_CASE), None), (rs.case_config(rs.BASE_CASE, **{field: value}), None)])
    seen = []
    s = util.run_schedule_and_compare(stream, schedule, chunks or [360, 97], oracle=oracle_of(("r", field), stream, schedule),
                                      after_switch=lambda e, f: seen.append(e.state()["reset_required"]))
    e = s["engine"]
    assert e.last_error() == oracle_of(("r", field), stream, schedule)[0].last_error()
    e.close()
    assert seen == [1]
    for st in (s["oracle_state"], s["engine_state"]):
        assert st["reset_required"] == 1 and st["num_columns"] == 360 and st["firings_consumed"] == stream.n_firings, st


def _feed_same_objects(e, o, stream, chunks):
    """`stream` through the oracle (one call) and the engine (calls of `chunks`), both as they are; events and published columns after every call."""
    assert o.add_firings(stream.xyz, stream.intensity, stream.poses) == 0, o.last_error()
    eo = o.drain_events()
    f = i = ev_pos = n_cols = 0
    while f < stream.n_firings:
        m = min(chunks[i % len(chunks)], stream.n_firings - f)
        assert e.add_firings(stream.xyz[f:f + m], stream.intensity[f:f + m], stream.poses[f:f + m]) == 0, e.last_error()
        try:
            ev_pos, pub = util.compare_events(eo, e.drain_events(), ev_pos)
            if pub is not None:
                util.compare_columns(o.read_published(pub[0], pub[1]), e.read_columns(pub[0], pub[1]), pub[0])
                n_cols += pub[1] - pub[0] + 1
        except AssertionError as ex:
            raise AssertionError(f"firings {f} .. {f + m - 1}: {ex}") from None
        f += m
        i += 1
    assert ev_pos == len(eo) and n_cols > stream.n_firings // 2
    so, se = o.state(), e.state()
    for k in util.STATE_FIELDS:
        assert so[k] == se[k], (k, so[k], se[k])


@pytest.mark.parametrize("chunks", [None, [17, 63, 1, 3]], ids=["columns_97", "small"])
@pytest.mark.parametrize("name", list(rs.SHAPE_CASES))
def test_reset_into_another_shape_keeps_the_common_rows_of_the_inclination_table(name, chunks, oracle_lib):
    """set_config (another num_columns: reset_required) or not, reset(rows), the transform again, and a stream of the new shape — engine and the SAME
    oracle object. cc.cpp:46 resizes sc_inclination_angles_between_lasers_: the rows both shapes have keep their values (all of them when only
    num_columns changes), so the first columns' supplemented inclination angles and ignore flags are not those of a fresh object
    (tests/test_reconfigure_cases_cpu.py: 437 + 37 cells for 720 -> 360 columns, 1 for 360 -> 720, 388 + 6 for 64 -> 128 rows, 197 + 2 for 128 -> 64).
    Before cc_engine_reset carried the table across its re-allocation the engine started such a shape with an all-NaN table, like a new engine."""
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    (first, cfg1), (second, cfg2) = rs.shape_case(name)
    e = Engine(cfg1, first.sensor.num_rows, 1, 0, IDENTITY)
    o = Oracle(cfg1, first.sensor.num_rows, IDENTITY)
    _feed_same_objects(e, o, first, [first.sensor.num_columns, 97])
    e.set_config(cfg2)
    o.set_config(cfg2)
    need = int(cfg1.num_columns != cfg2.num_columns)
    assert e.state()["reset_required"] == need == o.state()["reset_required"]
    assert e.state()["num_columns"] == cfg1.num_columns == o.state()["num_columns"]     # (the old geometry until reset)
    e.reset(second.sensor.num_rows)
    o.reset(second.sensor.num_rows)
    e.set_robot_from_sensor(IDENTITY)
    o.set_robot_from_sensor(IDENTITY)
    for st in (e.state(), o.state()):
        assert st["reset_required"] == 0 and st["num_rows"] == second.sensor.num_rows and st["num_columns"] == cfg2.num_columns, st
    _feed_same_objects(e, o, second, chunks or [second.sensor.num_columns, 97])
    e.close()
