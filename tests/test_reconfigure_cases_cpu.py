"""CPU: the schedules of reconfigure_streams.py (configuration and transform changed in mid-stream) held to their purpose on the oracle alone.
tests/test_gpu_reconfigure_parity.py compares the engine with the oracle on exactly these schedules; what is asserted here keeps that comparison
from passing vacuously: a run under a schedule is neither the run under its first nor under its second configuration (at least 100 published cells
— debug label, ignore flag, canonical cluster id, inclination bits — or the event list differ, the bar cases.py states for its sweep entries), the
oracle fed one call per segment equals the oracle fed firing by firing, a change of transform changes labels, and an object that went through
reset() into another shape is not a fresh object (the inclination table, cc.cpp:46)."""
import numpy as np
import pytest

import cases
import reconfigure_streams as rs
import util
from test_profile_cases_cpu import cells_that_differ, events_that_differ

_constant = {}


def record(oracle, events):
    lo, hi = oracle.published_range()
    return oracle.read_published(lo, hi), lo, events, None


def schedule_run(stream, schedule, per_firing=False):
    o, rc, ev = util.schedule_oracle_record(stream, schedule, per_firing)
    assert rc == 0, o.last_error()
    return record(o, ev), o


def constant_run(case, stream, cfg, tf=None):
    """The run of the whole stream under one configuration and transform; one oracle run per (case, configuration bytes, transform) and module."""
    key = (case, bytes(cfg), None if tf is None else np.asarray(tf).tobytes())
    if key not in _constant:
        o, rc = util.run_oracle(stream, cfg, tf)
        assert rc == 0, o.last_error()
        _constant[key] = record(o, o.drain_events())
    return _constant[key]


def assert_identical(a, oa, b, ob):
    (pa, la, ea, _), (pb, lb, eb, _) = a, b
    assert la == lb and ea.tobytes() == eb.tobytes()
    for k in pa:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert oa.state() == ob.state()


def assert_mixed(what, mixed, constants):
    figures = [(cells_that_differ(mixed, c), events_that_differ(mixed, c)) for c in constants]
    print(what, "differs from each constant run in (cells, events):", figures)
    for cells, events in figures:
        assert cells >= 100 or events > 0, (what, figures)
    return figures


# ---- thresholds ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", rs.THRESHOLD_ENTRIES)
def test_threshold_schedule_is_neither_constant_run(entry, oracle_lib):
    """base -> entry -> base at firings 397 and 611 of p_s64_profiles. Measured, cells of 49600 / events of about 1930 that differ from the base run
    and from the entry's run: use_terrain 10695 / 974 and 27681 / 1934; max_slope 0.05: 9375 / 942, 24701 / 1829; 0.21: 4980 / 943, 11715 / 1908;
    1.0: 6215 / 944, 15028 / 1884; first ring max 0.1: 212 / 34, 9210 / 1617; min -0.1: 3116 / 602, 717 / 242; last ground slope 0.1: 4960 / 812,
    15097 / 1835; -10: 208 / 45, 10994 / 1783; last ground distance 0.5: 4236 / 708, 13320 / 1802; close z 0.05: 6836 / 956, 16525 / 1849; close dist
    0.3: 6097 / 962, 11311 / 1439; next obstacle 0: 163 / 20, 10043 / 1697; 3.0: 5086 / 942, 14057 / 1841; no supplement 1713 / 0, 4010 / 0; no
    inclination ignore 366 / 0, 1708 / 0; chessboard 5885 / 944, 13159 / 1862; max_distance 0.05: 7203 / 946, 15380 / 1834; 3.0: 7214 / 944,
    19856 / 1845; fog 4973 / 931, 11069 / 1738; max_steps_in_column 1: 4250 / 844, 11002 / 1933; 3: 2949 / 697, 10949 / 1875; max_steps_in_row 1:
    4590 / 887, 10210 / 1855; 4: 4414 / 927, 7617 / 1537; min steps 5: 4622 / 943, 11085 / 1846; everything 14816 / 955, 29510 / 1854; without
    use_terrain 12390 / 955, 28872 / 1860."""
    stream, schedule, constants = rs.threshold_schedule(entry)
    mixed, o = schedule_run(stream, schedule)
    assert_mixed(entry, mixed, [constant_run(rs.BASE_CASE, stream, c) for c in constants])
    per_firing, o2 = schedule_run(stream, schedule, per_firing=True)
    assert_identical(mixed, o, per_firing, o2)


# ---- association family ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rs.ASSOCIATION_CASES)
@pytest.mark.parametrize("switch", list(rs.ASSOCIATION_SWITCHES))
def test_association_schedule_is_neither_constant_run(switch, name, oracle_lib):
    """On p_s64_profiles the bar of the thresholds. s64_forced_finish_ring is there for its open trees (an unbroken wall around the sensor: one
    cluster that never ends by itself): at every switch the oracle must hold unfinished trees, and columns inserted but not yet segmented or
    clustered; on a clean wall every point finds its neighbour at the first step, so of the four switches only every-nth-column changes its
    output (measured: 2085 / 2771 events against the two constant runs; the window limits and the early stop change nothing). On p_s64_profiles,
    cells / events against the first and the second configuration's run: every nth column 0 / 955, 0 / 1822; steps in row 4 -> 40 -> 4: 4414 / 929,
    7620 / 1535; early stop: 4629 / 943, 11099 / 1846; steps in row 20 -> 40 -> 20 and the stamp flag: nothing (see below)."""
    stream, schedule, constants = rs.association_schedule(switch, name)
    open_trees = []
    o, rc, ev = util.schedule_oracle_record(stream, schedule, at_switch=lambda orc, f: open_trees.append((f, orc.state())))
    assert rc == 0, o.last_error()
    mixed = record(o, ev)
    assert len(open_trees) == len(schedule) - 1
    for f, st in open_trees:
        assert st["n_unfinished_trees"] > 0 and st["first_unfinished_global_column_index"] <= st["ring_buffer_end_global_column_index"], (f, st)
    runs = [constant_run(name, stream, c) for c in constants]
    if name == rs.RING_CASE:
        print((switch, name), "(cells, events) against each constant run:", [(cells_that_differ(mixed, c), events_that_differ(mixed, c)) for c in runs],
              "unfinished trees at the switches:", [st["n_unfinished_trees"] for _, st in open_trees])
        if switch == "nth_column_1_2_1":
            assert_mixed((switch, name), mixed, runs)
    elif switch in ("last_point_stamp_0_1", "steps_in_row_20_40_20"):
        # Two schedules that are there for what the engine does around the change, not for the output. The reference only stamps its cluster
        # messages with use_last_point_for_cluster_stamp; neither the oracle nor the engine models a stamp. And no return of these two streams lies
        # so close to the sensor that its window reaches back more than 20 columns (at 360 columns: closer than 1.4 m, inside the ego box), so
        # max_steps_in_row = 40 computes what 20 computes — but beyond the LDS window it forces StreamState::assoc_mode to the global-memory
        # kernel, which is what the GPU test is after. steps_in_row_4_40_4 is the same switch with an output that shows it.
        for c in runs:
            assert cells_that_differ(mixed, c) == 0 and events_that_differ(mixed, c) == 0
    else:
        assert_mixed((switch, name), mixed, runs)
    per_firing, o2 = schedule_run(stream, schedule, per_firing=True)
    assert_identical(mixed, o, per_firing, o2)


# ---- ego box and transform ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", list(rs.EGO_SWITCHES))
def test_ego_schedule_is_neither_constant_run(switch, oracle_lib):
    """Measured, cells / events against the first and the second segment's run: tf 8233 / 924, 21424 / 1828 (4645 ground labels against the run without
    a change); asymmetric box 3999 / 664, 13101 / 1820; box without sensor 4705 / 685, 13116 / 1816; empty box 4174 / 673, 12947 / 1841; huge box
    13415 / 950, 30653 / 1798; both 2378 / 410, 6650 / 1012 (1223 labels); both_1m_up 3232 / 654, 8230 / 1378 (31 labels)."""
    stream, schedule, held = rs.ego_schedule(switch)
    mixed, o = schedule_run(stream, schedule)
    figures = assert_mixed(switch, mixed, [constant_run(rs.MOVING_CASE, stream, cfg, tf) for cfg, tf in held[:2]])
    if switch in ("tf", "both"):   # (both_1m_up moves the sensor 1 m up in a box that follows it: 31 labels; its bar is the one above)
        # against the run that never changes anything: labels (measured for identity -> ROBOT_TF_AHEAD_ABOVE at 397 on the static pose: 5978 cells)
        pm, lm, _, _ = mixed
        pc, lc, _, _ = constant_run(rs.MOVING_CASE, stream, held[0][0], held[0][1])
        assert lm == lc
        n = min(pm["x"].shape[0], pc["x"].shape[0])
        labels = int((pm["ground_point_label"][:n] != pc["ground_point_label"][:n]).sum())
        print(switch, "ground labels that differ from the run without a change:", labels)
        assert labels >= 100, (labels, figures)
    per_firing, o2 = schedule_run(stream, schedule, per_firing=True)
    assert_identical(mixed, o, per_firing, o2)


def test_transform_alone_on_the_static_pose(oracle_lib):
    """identity -> ROBOT_TF_AHEAD_ABOVE at firing 397 of p_s64_profiles (static identity pose): labels against the run without the change."""
    stream = rs.case_stream(rs.BASE_CASE)
    cfg = rs.case_config(rs.BASE_CASE)
    mixed, _ = schedule_run(stream, rs.cut(stream.n_firings, (397,), [(cfg, None), (None, cases.ROBOT_TF_AHEAD_ABOVE)]))
    pm, lm, _, _ = mixed
    pc, lc, _, _ = constant_run(rs.BASE_CASE, stream, cfg)
    n = min(pm["x"].shape[0], pc["x"].shape[0])
    labels = int((pm["ground_point_label"][:n] != pc["ground_point_label"][:n]).sum())
    print("identity -> ahead_above at 397: labels that differ", labels)
    assert lm == lc and labels >= 100


# ---- a change before every call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", rs.WALKS)
def test_walk_schedules_change_often_and_run_clean(name, seed, oracle_lib):
    """Measured, cells / events against the base configuration's run: seeds 9101 / 9108 / 9124 on p_s64_profiles 19396 / 1748, 7066 / 955, 15469 / 1761;
    seed 9114 on p_s128_profiles 25317 / 1670."""
    stream, schedule, applied = rs.walk_schedule(name, seed)
    assert sum(seg[0] for seg in schedule) == stream.n_firings
    assert len(schedule) >= 10 and len({a[2] for a in applied}) >= 8 and sum(a[3] is not None for a in applied) >= 3, applied
    mixed, o = schedule_run(stream, schedule)
    assert_mixed((name, seed), mixed, [constant_run(name, stream, rs.case_config(name))])
    per_firing, o2 = schedule_run(stream, schedule, per_firing=True)
    assert_identical(mixed, o, per_firing, o2)


# ---- changes that raise reset_required ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,expect_rc", [("is_single_threaded", 0, 0), ("num_columns", 400, 0), ("sensor_is_clockwise", 0, 0)])
def test_carrying_on_without_the_reset(field, value, expect_rc, oracle_lib):
    """The three fields of cc.cpp:69-74 changed at firing 397 and the rest fed without a reset: reset_required is 1, the geometry stays (360 columns
    until reset), all firings are consumed."""
    stream = rs.case_stream(rs.BASE_CASE)
    schedule = rs.cut(stream.n_firings, (397,), [(rs.case_config(rs.BASE_CASE), None), (rs.case_config(rs.BASE_CASE, **{field: value}), None)])
    o, rc, ev = util.schedule_oracle_record(stream, schedule)
    st = o.state()
    print(field, "rc", rc, repr(o.last_error()), {k: st[k] for k in ("reset_required", "firings_consumed", "num_columns")})
    assert st["reset_required"] == 1 and st["num_columns"] == 360
    if expect_rc is not None:
        assert rc == expect_rc
    if rc == 0:
        assert st["firings_consumed"] == stream.n_firings
    if field != "sensor_is_clockwise":
        # neither field is read by the hot path: the run equals the run that never changed it, but for the flag
        lo, hi = o.published_range()
        base = constant_run(rs.BASE_CASE, stream, rs.case_config(rs.BASE_CASE))
        assert cells_that_differ((o.read_published(lo, hi), lo, ev, None), base) == 0 and events_that_differ((None, None, ev), base) == 0


@pytest.mark.parametrize("name", list(rs.SHAPE_CASES))
def test_the_same_object_after_reset_is_not_a_fresh_one(name, oracle_lib):
    """set_config + reset(rows) of the object that ran the first stream against a fresh object, both on the second stream: the inclination table
    keeps the rows both shapes have (cc.cpp:46), so supplemented inclination angles and the too-big-inclination-difference ignore flags of the first
    columns differ. Measured for 720 -> 360 columns (s64_translate, then p_s64_terrain_gaps): 437 inclination_angle cells."""
    from oracle.pyoracle import Oracle, IDENTITY_TF
    (first, cfg1), (second, cfg2) = rs.shape_case(name)
    same = Oracle(cfg1, first.sensor.num_rows, IDENTITY_TF)
    assert same.add_firings(first.xyz, first.intensity, first.poses) == 0
    same.set_config(cfg2)
    assert same.state()["reset_required"] == int(cfg1.num_columns != cfg2.num_columns)
    same.reset(second.sensor.num_rows)      # (Oracle.reset takes the new row count: the next add_firings checks its arrays against it)
    same.set_robot_from_sensor(IDENTITY_TF)
    st = same.state()
    assert st["reset_required"] == 0 and st["num_rows"] == second.sensor.num_rows and st["num_columns"] == cfg2.num_columns
    assert same.add_firings(second.xyz, second.intensity, second.poses) == 0
    fresh, rc = util.run_oracle(second, cfg2)
    assert rc == 0
    lo, hi = same.published_range()
    assert (lo, hi) == fresh.published_range()
    a, b = same.read_published(lo, hi), fresh.read_published(lo, hi)
    incl = a["inclination_angle"].view(np.uint32) != b["inclination_angle"].view(np.uint32)
    ignored = a["is_ignored"] != b["is_ignored"]
    first_cell = tuple(int(v) for v in np.argwhere(incl | ignored)[0]) if (incl | ignored).any() else None
    print(name, "same object vs fresh: inclination_angle cells", int(incl.sum()), "ignore flags", int(ignored.sum()), "first (column, row)", first_cell)
    assert incl.sum() + ignored.sum() > 0
    if name == "columns_720_360":
        assert incl.sum() >= 100


# ---- the second restatement under a schedule -------------------------------------------------------------------------------------------------------------
def test_second_restatement_follows_an_everything_schedule(oracle_lib):
    """tests/test_oracle_independent.py's restatement of insertion and segmentation reads its configuration at every use, so it takes a schedule as it
    is: base -> everything -> base on p_s64_profiles, firing by firing, against the oracle's published columns."""
    from test_oracle_independent import Independent
    from oracle.pyoracle import IDENTITY_TF
    stream, schedule, _ = rs.threshold_schedule("everything")
    (pub, lo, _, _), o = schedule_run(stream, schedule)
    ind, f = None, 0
    for n, cfg, tf in schedule:
        if ind is None:
            ind = Independent(cfg, stream.sensor.num_rows, IDENTITY_TF)
        else:
            ind.cfg = cfg
        for k in range(f, f + n):
            ind.add_firing(stream.xyz[k], stream.intensity[k], stream.poses[k])
        f += n
    so = o.state()
    assert so["first_unfinished_global_column_index"] == ind.first_unfinished and so["ring_buffer_end_global_column_index"] == ind.ring_end
    hi = lo + pub["x"].shape[0] - 1
    assert hi - lo > 600
    for g in range(lo, hi + 1):
        c, s = ind.cells[g] if g in ind.cells else ind.column(g), ind.segmented[g]
        row = g - lo
        util.assert_float_equal(f"inclination_angle of column {g}", s["incl"], pub["inclination_angle"][row])
        util.assert_float_equal(f"distance of column {g}", c["dist"], pub["distance"][row])
        assert np.array_equal(s["ground"], pub["ground_point_label"][row]), g
        assert np.array_equal(s["debug"], pub["debug_ground_point_label"][row]), g
        assert np.array_equal(s["ignored"], pub["is_ignored"][row]), g
