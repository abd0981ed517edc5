"""GPU: the ground segmentation on uneven terrain and across its thresholds — engine against oracle, bit-exact, through util.run_and_compare
(events, labels, ignore flags, float bit patterns, ids, state; no tolerances).

Inputs: the slope-controlled columns of profile_streams.py (cases.PROFILE_CASES) under every entry of cases.SEGMENTATION_SWEEP /
cases.ASSOCIATION_SWEEP and the two "everything at once" configurations; tests/test_profile_cases_cpu.py shows on the oracle that each of them
matters. Every input runs through each implementation of the segmentation the engine has. Which kernels a selection reaches was read from
csrc/cc_launch.h (launch_batch, launch_tail, launch_segmentation, launch_small_call) and csrc/cc_engine.hip (use_small_front, add_firings_small):

  fused        default options, calls of `columns` and 97 firings: bp.par (n >= 64) and bp.fuse -> k_ego + k_insert_par with seg_pre_cells in its
               fused front, batches closed as fused skip k_table / k_seg_pre, then k_seg_scan (16-row chunks at 64 rows; the form for row counts
               that are no multiple of 16 / of 8 at 40 / 50 rows; above 64 rows there is no fused front: k_insert_multi, k_table, k_seg_pre<2>,
               k_seg_scan<2>). Asserted: debug counter 4 (batches closed as fused) > 0 up to 64 rows, counter 7 (batches the parallel kernel saw) > 0.
  seg_pre      fuse_front = 0, same calls: k_insert_par without the front, k_table, k_ego, k_seg_pre, k_seg_scan. Asserted: counter 4 == 0, 7 > 0.
  serial       parallel_insert = 0, calls of 211: k_prep + k_insert2, k_table, k_ego, k_seg_pre, k_seg_scan. Asserted: counter 7 == 0.
  small_all    calls of 1, 3, 17, 40, 63 firings, default options: use_small_front (count 1, n <= seg_small_max, rows <= 64) ->
               add_firings_small: up to 8 firings a captured graph, 9 .. 63 a direct launch, of k_small_all — seg_small_body embedded. Where
               the call is not "lean" (assoc_batch = 0 or assoc_waves = 1) launch_small_call takes k_small_front instead.
  small_front  the same calls with small_all = 0: k_small_front (seg_small_body embedded) + k_assocb + k_small_tail.
  seg_small    the same calls with small_front = 0: the general path with n < 64, so no bp.par; launch_segmentation: seg_small -> k_ego and
               k_seg_small as a launch of its own.
  seg_scan     the same calls with seg_small_max = 0: neither use_small_front nor seg_small -> k_table, k_ego, k_seg_pre and k_seg_scan on tiles
               of a few columns.
  scan_rows    (128 rows) scan_packed = 0 on the calls of `fused`: the window scan behind the segmentation as k_scan instead of k_scan2.
No counter tells the four small-call forms apart; they are selected by the options above and by nothing else."""
import ctypes as C

import numpy as np
import pytest

import cases
import util

pytestmark = pytest.mark.gpu

SMALL = [1, 3, 17, 40, 63]
PATHS = {
    "fused": ({}, None),
    "seg_pre": ({"fuse_front": 0}, None),
    "serial": ({"parallel_insert": 0}, [211]),
    "small_all": ({}, SMALL),
    "small_front": ({"small_all": 0}, SMALL),
    "seg_small": ({"small_front": 0}, SMALL),
    "seg_scan": ({"seg_small_max": 0}, SMALL),
    "scan_rows": ({"scan_packed": 0}, None),
}
ALL_SMALL_ROW_PATHS = ["fused", "seg_pre", "serial", "small_all", "small_front", "seg_small", "seg_scan"]

_oracles = {}


def oracle_of(key, stream, cfg, tf):
    """One oracle run per (case, configuration) and module; it is only read afterwards."""
    if key not in _oracles:
        _oracles[key] = util.oracle_record(stream, cfg, tf)
    return _oracles[key]


def debug_counters(e):
    from continuous_clustering_amd import load_library
    L = load_library()
    L.cc_engine_debug_counters.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = np.zeros(16, dtype=np.uint64)
    assert L.cc_engine_debug_counters(e.h, 0, out.ctypes.data) == 0
    return out


def run_path(key, stream, cfg, tf, path, options=None, chunks=None, before_close=None, expect_fused=True):
    """before_close(engine, oracle): called after the comparison, while the engine still exists. expect_fused = False: an input of which no call
    is taken whole by the parallel insertion (firings that leave its shape in every call), so that no batch can be closed as fused; the kernel
    must still have seen the batches (debug counter 7)."""
    opts, path_chunks = PATHS[path]
    opts = dict(opts, **(options or {}))
    if chunks is None:
        chunks = path_chunks or [stream.sensor.num_columns, 97]
    box = {}

    def setup(e):
        for k, v in opts.items():
            e.set_option(k, v)
        box["e"] = e

    summary = util.run_and_compare(stream, cfg, chunks=chunks, robot_tf=tf, engine_setup=setup, oracle=oracle_of(key, stream, cfg, tf))
    assert summary["published_columns"] > stream.n_firings // 2
    dbg = debug_counters(box["e"])
    rows = stream.sensor.num_rows
    if path in ("fused", "scan_rows") and "parallel_insert" not in opts:
        assert dbg[7] > 0, dbg
        if rows <= 64 and expect_fused:
            assert dbg[4] > 0, dbg
    elif path == "seg_pre":
        assert dbg[4] == 0 and dbg[7] > 0, dbg
    elif path == "serial" or chunks == SMALL:
        assert dbg[4] == 0 and dbg[7] == 0, dbg      # (calls below 64 firings never reach the parallel insertion)
    if before_close is not None:
        before_close(box["e"], oracle_of(key, stream, cfg, tf)[0])
    box["e"].close()
    return summary


def sweep_case(entry, name=cases.SWEEP_BASE_CASE):
    return (name, entry), cases.profile_stream(name), cases.profile_config(name, **cases.sweep_overrides(entry)), None


# ---- the sweep table on p_s64_profiles -----------------------------------------------------------------------------------------------------
SEGMENTATION_ENTRIES = ["base"] + list(cases.SEGMENTATION_SWEEP) + ["everything", "everything_no_terrain"]


@pytest.mark.parametrize("path", ALL_SMALL_ROW_PATHS)
@pytest.mark.parametrize("entry", SEGMENTATION_ENTRIES)
def test_segmentation_entry_on_every_path(entry, path, oracle_lib):
    """One field or pair of cc_config off its default (or all of them), on each implementation of the segmentation: seg_pre_cells + k_seg_scan
    (fused, seg_pre, serial, seg_scan) and k_seg_small's fixed point (small_all, small_front, seg_small)."""
    run_path(*sweep_case(entry), path)


@pytest.mark.parametrize("path,options", [("fused", {}), ("small_all", {}), ("fused", {"assoc_batch": 0, "assoc_waves": 1}),
                                          ("fused", {"assoc_batch": 0, "assoc_waves": 3}), ("small_all", {"assoc_batch": 0, "assoc_waves": 1}),
                                          ("small_all", {"assoc_batch": 0, "assoc_waves": 3})])
@pytest.mark.parametrize("entry", list(cases.ASSOCIATION_SWEEP))
def test_association_entry(entry, path, options, oracle_lib):
    """The window limits of the association on the same columns (many short obstacle runs per column): the batch-parallel kernel in front
    (default), and k_assoc_lds (assoc_waves 1) / k_assoc3 (3) alone. Small calls without assoc_batch are not lean: k_small_front + these kernels."""
    run_path(*sweep_case(entry), path, options)


@pytest.mark.parametrize("path", ALL_SMALL_ROW_PATHS)
def test_terrain_mode_five_metre_bound(path, oracle_lib):
    """use_terrain = 1 where its own rule decides: smooth ground with many missing rows, so that "flat, but more than 5 m beyond the previous point"
    makes the first obstacle of most columns (tests/test_profile_cases_cpu.py counts the cells)."""
    stream, cfg, tf = cases.build_case("p_s64_terrain_gaps")
    run_path(("p_s64_terrain_gaps", "own"), stream, cfg, tf, path)


# ---- other row counts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "seg_pre", "serial", "scan_rows"])
@pytest.mark.parametrize("entry", ["base", "use_terrain", "everything", "everything_no_terrain"])
def test_two_rows_per_lane(entry, path, oracle_lib):
    """128 rows (VLS configuration): the two-rows-per-lane instantiations of k_seg_pre and k_seg_scan."""
    run_path(*sweep_case(entry, "p_s128_profiles"), path)


@pytest.mark.parametrize("path", ["fused", "small_all", "seg_small"])
@pytest.mark.parametrize("entry", ["base", "use_terrain", "everything", "everything_no_terrain"])
@pytest.mark.parametrize("name", ["p_s40_profiles", "p_s50_profiles", "p_s16_profiles"])
def test_row_counts_off_the_chunk_size(name, entry, path, oracle_lib):
    """40 rows (a multiple of 8, not of 16), 50 rows (neither) and 16 rows: k_seg_scan's forms for columns that do not fill its 16-row chunks,
    and k_seg_small with lanes that own no row."""
    run_path(*sweep_case(entry, name), path)


# ---- fixed-point depth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [[1], [63]])
@pytest.mark.parametrize("path", ["small_all", "small_front", "seg_small"])
@pytest.mark.parametrize("name", cases.FIXED_POINT_CASES)
def test_columns_that_take_the_label_iteration_deep(name, path, chunks, oracle_lib):
    """p_s64_alternating changes between ground and obstacle on every second valid row (25 changes in the median column; its labels settle after 2 - 3
    rounds); p_s64_label_chains is the input on which k_seg_small's iteration needs up to 33 rounds at 64 rows (the oracle's labels are the
    fixed point, and the rounds are counted, in tests/test_profile_cases_cpu.py). One column per call, and 63."""
    stream, cfg, tf = cases.build_case(name)
    run_path((name, "own"), stream, cfg, tf, path, chunks=chunks)


@pytest.mark.parametrize("name", cases.FIXED_POINT_CASES)
def test_deep_columns_on_the_row_serial_kernel(name, oracle_lib):
    """The same columns through k_seg_scan: behind the serial and the parallel insertion (the first call of an engine starts the ring in the serial
    kernel, the second one is taken by k_insert_par), and on tiles of seven columns."""
    stream, cfg, tf = cases.build_case(name)
    util.run_and_compare(stream, cfg, chunks=[50, 70], robot_tf=tf, oracle=oracle_of((name, "own"), stream, cfg, tf))
    run_path((name, "own"), stream, cfg, tf, "seg_scan", chunks=[7])


# ---- ego box and its skip_r2 bound -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "seg_pre", "small_all"])
@pytest.mark.parametrize("setting", ["plain"] + list(cases.EGO_SETTINGS))
def test_ego_box_under_a_moving_tilting_pose(setting, path, oracle_lib):
    """p_s64_profiles under a pose sequence that drives, yaws, rolls and pitches, with transforms and boxes that put the sensor off the box's centre,
    outside it, and that make the box empty or all-embracing: k_ego's per-firing record (the bound below which a return is inside for certain or
    outside for certain without the exact transform) in front of k_insert_par, in front of k_seg_pre and inside k_small_all."""
    if setting == "plain":
        stream, cfg, tf = cases.build_case("p_s64_profiles_moving")
    else:
        stream, cfg, tf = cases.ego_case(setting)
    run_path(("ego", setting), stream, cfg, tf, path)


# ---- many streams in one launch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["everything", "everything_no_terrain"])
def test_pipelined_profile_streams(entry, oracle_lib):
    """12 profile streams with different seeds through cc_engine_add_firings_device (three calls of 270 firings): the fused front of k_insert_par
    and k_seg_scan where the streams share a launch, every threshold off its default."""
    from continuous_clustering_amd import Engine
    from test_gpu_stress import _compare_with_oracles, _feed_pipelined
    name = cases.SWEEP_BASE_CASE
    cfg = cases.profile_config(name, **cases.sweep_overrides(entry))
    streams = [cases.profile_stream(name, seed=5000 + s) for s in range(12)]
    e = Engine(cfg, 64, len(streams))
    e.record_events(False)
    NB, _slots = _feed_pipelined(e, streams, 270, ring=4)
    assert NB == 3
    assert e.sync() == 0, e.last_error()
    bad = _compare_with_oracles(e, cfg, streams, NB, 270)
    fused = int(debug_counters(e)[4])
    e.close()
    assert not bad, bad[:3]
    assert fused > 0
