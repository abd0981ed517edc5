"""GPU: degenerate and extreme lidar returns — engine against oracle, bit-exact, through test_gpu_segmentation_sweep.run_path /
util.run_and_compare (events, labels, ignore flags, float bit patterns, ids, state; no tolerances), and the error text of both.

The inputs are the r_* cases of cases.py (return_streams.py); tests/test_return_cases_cpu.py shows on the oracle that each of them does what it is
here for. What they reach in the engine that no other input does:
  insertion     prep_point with atan2f of zeros and infinities, a range of 0 / inf / NaN, asinf(0 / 0), the column indices num_columns and INT_MIN
                (f2i_x86 of a NaN azimuth). k_insert_par and k_insert_multi take a firing only when its first valid return's column lies in
                [0, num_columns) and all its rows agree; everything else is handed to the serial k_insert2 in the middle of a batch, so the planted
                firings mostly test that hand-over and k_insert2's arithmetic (read for cir = INT_MIN and cir = num_columns: a ring column is always
                the previous rearmost column's plus an offset within (-2 num_columns, 2 num_columns], corrected once by the ring length of
                10 num_columns; INT_MIN makes the global column negative, which is dropped before any index is formed).
  segmentation  slopes with a range of 0 or inf and an inclination of NaN, in k_seg_scan, k_seg_small and the fused front (selects where the
                reference has nested ifs).
  association   asinf(max_distance / range) of a range of 0, a denormal, inf; inf - inf in the 3-D distances.
  hand-over     Engine.take_points / take_clusters with inf and NaN coordinates (the bounding box's min / max).
The paths (fused, seg_pre, serial, small_all, small_front, seg_small, seg_scan, scan_rows) are those of test_gpu_segmentation_sweep.py."""
import numpy as np
import pytest

import cases
import return_streams as rs
from test_gpu_segmentation_sweep import ALL_SMALL_ROW_PATHS, debug_counters, run_path

pytestmark = pytest.mark.gpu

_built = {}


def case(name):
    """One build per case and module; the streams are only read."""
    if name not in _built:
        _built[name] = cases.build_case(name)
    return _built[name]


def same_error_text(engine, oracle):
    """a dropped return (NaN azimuth: negative global column) leaves the status at 0 and this text, in the oracle and in the engine"""
    assert engine.last_error() == oracle.last_error(), (engine.last_error(), oracle.last_error())


# Classes whose firings keep the shape k_insert_par takes — every return in the firing's own column, strictly ahead of the previous firing: calls
# of them are taken whole and closed as fused, so the fused front segments their ranges of 0, inf and NaN. Every other class moves a return to
# another column, drops it or empties firings, in about every tenth firing or in long runs: no call of 97 firings is taken whole (debug counter 4
# stays 0 on the GPU), the parallel kernel hands the calls over to the serial one on their way.
KEEP_THE_SHAPE = rs.SCALED_CLASSES + rs.ONE_CLASSES + ("z_pinf", "z_ninf", "z_nan", "edge_lo_exact", "edge_hi_below", "dup_rows")


def run_case(name, path, options=None, chunks=None, also=None):
    stream, cfg, tf = case(name)
    cls = name[2:].partition("__")[0]

    def before_close(engine, oracle):
        same_error_text(engine, oracle)
        if also is not None:
            also(engine)

    return run_path((name, "own"), stream, cfg, tf, path, options, chunks, before_close=before_close, expect_fused=cls in KEEP_THE_SHAPE)


# ---- every class on every implementation of the segmentation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ALL_SMALL_ROW_PATHS)
@pytest.mark.parametrize("name", cases.RETURN_S64_CASES)
def test_class_on_every_path(name, path, oracle_lib):
    """64 x 360 profile columns, 2 % of the returns of rotations 2 and 3, in a tenth of their firings, replaced by one class (the per-firing
    classes: 5 % of the firings, or the stated runs). The y = NaN classes leave
    the oracle's error text ("negative global column index", status 0): the engine's state and text are compared like everything else."""
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "serial", "small_all"])
@pytest.mark.parametrize("name", cases.RETURN_CCW_CASES)
def test_zeros_under_the_other_sensor_direction(name, path, oracle_lib):
    """sensor_is_clockwise = 0: azimuth +pi gives inc_az = pi_f + pi_f (column num_columns), -pi gives 0 — the other way round."""
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "seg_pre", "serial", "scan_rows"])
@pytest.mark.parametrize("name", cases.RETURN_S128_CASES)
def test_class_with_two_rows_per_lane(name, path, oracle_lib):
    """128 rows: k_insert_multi instead of the fused front, the two-rows-per-lane forms of k_insert2, k_seg_pre and k_seg_scan."""
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "small_all", "seg_small"])
@pytest.mark.parametrize("name", cases.RETURN_S40_CASES)
def test_class_with_rows_off_the_chunk_size(name, path, oracle_lib):
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "serial", "small_all"])
@pytest.mark.parametrize("name", cases.RETURN_MOVING_CASES)
def test_infinities_under_a_moving_pose(name, path, oracle_lib):
    """no entry of the pose's rotation block is zero: an infinite coordinate gives infinite odom coordinates and an infinite range (67 - 540 such
    published cells per case on the oracle; none for all three at inf, where inf - inf = NaN) instead of the NaN that 0 * inf makes of them under the static pose."""
    run_case(name, path)


# ---- each insertion kernel, planted firings first, last and in the middle of a call ----------------------------------------------------------------
INSERT_CHUNKS = [360, 97, 1, 23]


def _insertion_params():
    """every class on the two parallel forms; the serial kernel alone has every class in test_class_on_every_path, here the thinner set"""
    thin = [f"r_{cls}__{cases.RETURN_BASE_CASE}" for cls in cases.RETURN_THIN_CLASSES]
    return [(name, k) for name in cases.RETURN_S64_CASES for k in (1, 2)] + [(name, 0) for name in thin]


@pytest.mark.parametrize("name,parallel_insert", _insertion_params())
def test_class_on_each_insertion_kernel(name, parallel_insert, oracle_lib):
    """parallel_insert 0: k_prep + k_insert2 alone; 1: k_insert_par, then k_insert_multi, then k_insert2 for what they leave; 2: k_insert_par and
    k_insert2. Calls of 360, 97, 1 and 23 firings in turn: the calls of 64 and more go to the parallel kernels (asserted by debug counter 7), the
    small ones to k_small_all, and the planted firings fall on the first, the last and the inner firings of calls."""
    def counters(e):
        dbg = debug_counters(e)
        assert (dbg[7] > 0) == (parallel_insert != 0), dbg

    run_case(name, "fused", {"parallel_insert": parallel_insert}, INSERT_CHUNKS, also=counters)


@pytest.mark.parametrize("parallel_insert", [1, 2])
@pytest.mark.parametrize("name", cases.RETURN_S128_CASES)
def test_class_on_the_multi_column_insertion(name, parallel_insert, oracle_lib):
    """two rows per lane with k_insert_multi behind k_insert_par (1) and without it (2)"""
    run_case(name, "fused", {"parallel_insert": parallel_insert}, [340, 97, 1, 23])


# ---- the classes that reach clusters, on the association kernels alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("name", [f"r_{cls}__{cases.RETURN_BASE_CASE}" for cls in rs.CLUSTER_CLASSES])
def test_cluster_classes_on_the_association_kernels_alone(name, waves, oracle_lib):
    """scaled, infinite and duplicated returns without the batch-parallel kernel in front: k_assoc_lds (assoc_waves 1) and k_assoc3 (3)."""
    run_case(name, "fused", {"assoc_batch": 0, "assoc_waves": waves})


def _ring_params():
    """the unbroken wall ring (forced finishes): every case on the default association, and with the kernels behind it in turn"""
    out = []
    for i, name in enumerate(cases.RETURN_RING_CASES):
        out.append((name, "fused", None))
        out.append((name, "small_all" if i % 2 else "fused", {"assoc_batch": 0, "assoc_waves": 1 if i % 4 < 2 else 3}))
    return out


@pytest.mark.parametrize("name,path,options", _ring_params())
def test_cluster_classes_in_a_ring_that_is_finished_by_force(name, path, options, oracle_lib):
    run_case(name, path, options)


# ---- all classes at once through the ring wrap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "small_all"])
def test_mixed_classes_through_the_ring_wrap(path, oracle_lib):
    """13 rotations of 64 x 240 through the ring of 10, every class at once at about 2 % of the returns; reset_required and the error text are set
    on the way (tests/test_return_cases_cpu.py) and the stream goes on."""
    run_case(cases.RETURN_MIXED_CASE, path)


# ---- many streams in one launch ---------------------------------------------------------------------------------------------------------------------
def test_pipelined_mixed_streams(oracle_lib):
    """Twelve profile streams with different seeds, each with every class planted under a seed of its own, through cc_engine_add_firings_device,
    four calls of 180 firings: the first starts the rings, the second is taken whole by k_insert_par and closed as fused (the first rotation is the
    parent's), the last two carry the degenerate firings of twelve streams side by side in the launches of the fused front — taken back where a
    firing leaves the shape — and of the kernels behind it."""
    import time
    from continuous_clustering_amd import Engine
    from test_gpu_stress import _compare_with_oracles, _feed_pipelined
    name = cases.RETURN_BASE_CASE
    cfg = cases.profile_config(name)
    t0 = time.perf_counter()
    streams = [rs.plant_mixed(cases.profile_stream(name, seed=7000 + s), 7100 + s)[0] for s in range(12)]
    t1 = time.perf_counter()
    e = Engine(cfg, 64, len(streams))
    e.record_events(False)
    NB, _slots = _feed_pipelined(e, streams, 180, ring=4)
    assert NB == 4
    assert e.sync() == 0, e.last_error()
    t2 = time.perf_counter()
    bad = _compare_with_oracles(e, cfg, streams, NB, 180)
    t3 = time.perf_counter()
    fused = int(debug_counters(e)[4])
    text = e.last_error()
    e.close()
    print(f"streams {t1 - t0:.2f} s, engine {t2 - t1:.2f} s, oracles and comparison {t3 - t2:.2f} s; batches closed as fused {fused}")
    assert not bad, bad[:3]
    assert fused > 0
    assert text == "negative global column index"        # (every stream drops its y = NaN returns; the status above stayed 0)


# ---- points and clusters in device memory ---------------------------------------------------------------------------------------------------------------
TAKE_CASES = [f"r_{cls}__s64_forced_finish_ring" for cls in ("scaled_1e36", "scaled_overflow", "all_inf", "z_nan")]


@pytest.mark.parametrize("name", TAKE_CASES)
def test_take_points_and_clusters_with_extreme_coordinates(name, oracle_lib):
    """Engine.take_points (clustered stage, all returns) and Engine.take_clusters(6) after every rotation of the wall ring: records against the
    oracle's published cells bit for bit (a cell with a NaN range holds no return and is not handed over, on either side), descriptors against
    the oracle's cluster events, bounding boxes against the records (coordinates up to 1e38; a NaN only equals a NaN)."""
    from continuous_clustering_amd import take
    from test_gpu_take import Log, _against_oracle as points_against_oracle
    from test_gpu_take_clusters import FU, ClusterLog, _against_oracle, _counters, _run_device
    stream, cfg, tf = case(name)
    assert tf is None
    cols = stream.sensor.num_columns
    NB = stream.n_firings // cols
    assert NB == 4
    clusters, points = ClusterLog(1, 6), Log(1)

    def per_call(e, b):
        clusters.add(*e.take_clusters(6), counters=_counters(e, 1))
        points.add(*e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS), upper=[e.state(0)[FU]])

    e = _run_device([stream], cfg, NB, per_call)
    fu = e.state(0)[FU]
    n, skipped = _against_oracle(clusters, 0, stream, cfg, NB * cols, fu, what=name)
    n_points = points_against_oracle(points, 0, stream, cfg, NB * cols, fu, what=name)
    e.close()
    print(f"{name}: {n} clusters ({skipped} beyond first_unpublished), {n_points} records")
    assert n - skipped >= 1 and n_points > 0.5 * 64 * fu
    rec = points.of(0)[0]
    if "overflow" in name:
        assert np.isinf(rec["distance"]).sum() >= 500
    if "1e36" in name:
        assert (np.abs(rec["x"]) > 1e36).sum() >= 300
