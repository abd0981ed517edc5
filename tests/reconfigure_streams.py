"""Schedules: the configuration and the robot transform change in mid-stream (setConfiguration from the reference node's dynamic-reconfigure
callback, continuous_clustering_node.cpp:180-234, and setTransformRobotFrameFromSensorFrame from its firing callback, :149-155, while firings keep
arriving). Only is_single_threaded, sensor_is_clockwise and num_columns raise reset_required (cc.cpp:66-81); every other field takes effect between
two firings, with columns inserted but not yet segmented and point trees still open.

A schedule is a list of segments (firings, cc_config or None, robot_from_sensor or None), the change applied before the segment's firings
(util.schedule_oracle_record, util.run_schedule_and_compare). Everything here is built from the tables of cases.py; tests/test_reconfigure_cases_cpu.py
holds each schedule to its purpose on the oracle, tests/test_gpu_reconfigure_parity.py runs the engine on them, tools/stress_parity.py --reconfigure
draws from CONFIG_TABLE."""
from __future__ import annotations

import functools

import numpy as np

import cases
import profile_streams
from continuous_clustering_amd.synth import SensorModel

BASE_CASE = cases.SWEEP_BASE_CASE        # p_s64_profiles: 810 firings, 360 columns
MOVING_CASE = "p_s64_profiles_moving"
RING_CASE = "s64_forced_finish_ring"     # an unbroken wall ring: trees are open at every switch
SWITCH_AT = (397, 611)                   # mid-rotation, no multiple of any chunk size the tests use

THRESHOLD_ENTRIES = list(cases.SEGMENTATION_SWEEP) + list(cases.ASSOCIATION_SWEEP) + ["everything", "everything_no_terrain"]
EVERYTHING_ENTRIES = ["everything", "everything_no_terrain"]

# what a draw of "the next configuration" chooses from (overrides of the case's base configuration)
CONFIG_TABLE = {"base": {}, **cases.SEGMENTATION_SWEEP, **cases.ASSOCIATION_SWEEP, "everything": cases.EVERYTHING,
                "everything_no_terrain": cases.EVERYTHING_NO_TERRAIN,
                **{"box_" + k: over for k, (_, over) in cases.EGO_SETTINGS.items() if over},
                "every_2nd_column": dict(cluster_point_trees_every_nth_column=2), "max_steps_in_row_40": dict(max_steps_in_row=40),
                "no_early_stop": dict(stop_after_association_enabled=0)}
TRANSFORM_TABLE = {"identity": np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64), "ahead_above": cases.ROBOT_TF_AHEAD_ABOVE,
                   "tilted": cases.ROBOT_TF_TILTED, "1m_up": cases.ROBOT_TF_1M_UP}

# the association family: (field, values in turn) — the second value selects another kernel family (every nth column: cc_launch.h), forces
# StreamState::assoc_mode up (max_steps_in_row beyond the LDS window) or the exact serial association (no early stop)
ASSOCIATION_SWITCHES = {
    "nth_column_1_2_1": ("cluster_point_trees_every_nth_column", (1, 2, 1)),
    "steps_in_row_20_40_20": ("max_steps_in_row", (20, 40, 20)),
    "steps_in_row_4_40_4": ("max_steps_in_row", (4, 40, 4)),     # (40 computes what 20 computes on these streams; from 4 the switch shows)
    "early_stop_1_0_1": ("stop_after_association_enabled", (1, 0, 1)),
    "last_point_stamp_0_1": ("use_last_point_for_cluster_stamp", (0, 1)),
}
ASSOCIATION_CASES = [BASE_CASE, RING_CASE]

# ego box and transform on the moving pose sequence: name -> the (transform name or None, overrides) of each segment
EGO_SWITCHES = {
    "tf": ((None, {}), ("ahead_above", {}), ("tilted", {})),
    **{"box_" + k: ((None, {}), (None, cases.EGO_SETTINGS[k][1]), (None, {})) for k in ("asymmetric_box", "box_without_sensor", "empty_box", "huge_box")},
    "both": ((None, {}), ("ahead_above", cases.EGO_SETTINGS["sensor_ahead_above"][1]), ("tilted", cases.EGO_SETTINGS["asymmetric_box"][1])),
    "both_1m_up": ((None, {}), ("1m_up", cases.EGO_SETTINGS["sensor_1m_up"][1]), (None, cases.EGO_SETTINGS["height_max_5"][1])),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(stream, configuration) of a case of cases.py or of S128_360 below; made once, read-only afterwards."""
    if name == S128_360:
        sen = SensorModel(num_rows=128, num_columns=360, incl_top_deg=15.0, incl_bottom_deg=-25.0)
        return profile_streams.make_profile_stream(sen, 810, 341), cases._kitti(360)
    stream, cfg, tf = cases.build_case(name)
    assert tf is None
    return stream, cfg


def case_stream(name):
    return _case(name)[0]


def case_config(name, **over):
    """The configuration of the case with fields overridden."""
    cfg = _case(name)[1].copy()
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


# changes of shape: (first case, second case). The first stream runs, then set_config(second configuration) — reset_required where num_columns
# differs —, reset(second row count), the transform again, the second stream. cc.cpp:46 resizes the inclination table: the rows both shapes have keep
# their values, so the same object after reset is not a fresh one.
S128_360 = "p_s128_profiles_360"         # 128 rows at the 360 columns and configuration of p_s64_profiles: only the row count changes
SHAPE_CASES = {
    "columns_720_360": ("s64_translate", "p_s64_terrain_gaps"),
    "columns_360_720": ("p_s64_terrain_gaps", "s64_translate"),
    "rows_64_128": (BASE_CASE, S128_360),
    "rows_128_64": (S128_360, BASE_CASE),
}


def shape_case(name):
    """((first stream, configuration), (second stream, configuration))."""
    a, b = SHAPE_CASES[name]
    return _case(a), _case(b)


def cut(n_firings, switch_at, changes):
    """Segments of a stream of n_firings with `changes` = [(config, transform), ...], the first from firing 0, the others from switch_at on."""
    assert len(changes) == len(switch_at) + 1 and all(0 < a < n_firings for a in switch_at)
    edges = [0] + list(switch_at) + [n_firings]
    return [(edges[k + 1] - edges[k], cfg, tf) for k, (cfg, tf) in enumerate(changes)]


def threshold_schedule(entry, name=BASE_CASE):
    """(stream, schedule, constant configurations): base -> entry -> base at SWITCH_AT."""
    stream = case_stream(name)
    base, other = case_config(name), case_config(name, **cases.sweep_overrides(entry))
    return stream, cut(stream.n_firings, SWITCH_AT, [(base, None), (other, None), (base, None)]), [base, other]


def association_schedule(switch, name):
    stream = case_stream(name)
    field, values = ASSOCIATION_SWITCHES[switch]
    cfgs = [case_config(name, **{field: v}) for v in values]
    return stream, cut(stream.n_firings, SWITCH_AT[:len(values) - 1], [(c, None) for c in cfgs]), cfgs[:2]


def ego_schedule(switch):
    """(stream, schedule, the (configuration, transform) of every segment)."""
    stream = case_stream(MOVING_CASE)
    changes, tf_now = [], None
    for tf_name, over in EGO_SWITCHES[switch]:
        changes.append((case_config(MOVING_CASE, **over), None if tf_name is None else TRANSFORM_TABLE[tf_name]))
    schedule = cut(stream.n_firings, SWITCH_AT, changes)
    held = []
    for cfg, tf in changes:
        tf_now = tf if tf is not None else tf_now
        held.append((cfg, tf_now))
    return stream, schedule, held


# (case, seed) of the walks below: seeds under which the draw makes 11 - 21 calls (the sizes 211 and 360 end a stream of 810 firings quickly)
WALKS = [(BASE_CASE, 9101), (BASE_CASE, 9108), (BASE_CASE, 9124), ("p_s128_profiles", 9114)]


def walk_schedule(name, seed, sizes=(1, 3, 17, 63, 97, 211, 360), table=None, every_nth_transform=3):
    """(stream, schedule, applied): a change before every call — the next configuration drawn from `table` (CONFIG_TABLE) over the case's base,
    every third call a transform as well; the call sizes drawn from `sizes`. `applied`: what was drawn, for the assertion message."""
    rng = np.random.default_rng(seed)
    table = CONFIG_TABLE if table is None else table
    stream = case_stream(name)
    schedule, applied, f, k = [], [], 0, 0
    while f < stream.n_firings:
        n = min(int(rng.choice(sizes)), stream.n_firings - f)
        entry = "base" if k == 0 else str(rng.choice(sorted(table)))
        tf_name = str(rng.choice(sorted(TRANSFORM_TABLE))) if k > 0 and k % every_nth_transform == 0 else None
        schedule.append((n, case_config(name, **table[entry]), None if tf_name is None else TRANSFORM_TABLE[tf_name]))
        applied.append((f, n, entry, tf_name))
        f += n
        k += 1
    return stream, schedule, applied
