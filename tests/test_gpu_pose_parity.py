"""GPU: odometry poses far from the origin, not rigid and not finite — engine against oracle, bit-exact, through
test_gpu_segmentation_sweep.run_path / util.run_and_compare (events, labels, ignore flags, float bit patterns, ids, state; no tolerances).

The inputs are the o_* cases of cases.py (pose_streams.py); tests/test_pose_cases_cpu.py shows on the oracle that each of them does what it is here
for. What they reach in the engine that no other input does:
  far offsets   float32 odom coordinates quantised to 3 cm .. 64 m: vertically adjacent cells with the same (x, y), so that k_seg_scan, k_seg_small
                and the fused front divide by zero horizontal steps (+-inf, 0 / 0) where the reference's nested ifs were rewritten into selects;
                distance 0 between different cells in the association; min / max of values near 5e6 in cc_engine_take_clusters.
  corners       returns just inside and just outside the ego box's corners, under rigid, scaled, sheared, float32-rounded and far-away poses:
                ego_record's skip_r2 (csrc/cc_k_segment.h) must not cut a corner off — its finite branch with sigma < 1 and with the translation
                term delta up to 1.4 m, and its +inf branch (scaled_0.7).
  non-finite    NaN / inf in the poses of some firings: the NaN guards of ego_record and whatever the insertion makes of such a firing.
The paths (fused, seg_pre, serial, small_all, small_front, seg_small, seg_scan, scan_rows) are those of test_gpu_segmentation_sweep.py."""
import numpy as np
import pytest

import cases
import pose_streams
from test_gpu_segmentation_sweep import ALL_SMALL_ROW_PATHS, debug_counters, run_path

pytestmark = pytest.mark.gpu

_built = {}


def case(name):
    """One build per case and module; the streams are only read."""
    if name not in _built:
        _built[name] = cases.build_case(name)
    return _built[name]


def run_case(name, path, options=None, chunks=None):
    stream, cfg, tf = case(name)
    return run_path((name, "own"), stream, cfg, tf, path, options, chunks)


def far(parent):
    return [f"o_{off}__{parent}" for off in pose_streams.FAR_OFFSETS]


# ---- far offsets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ALL_SMALL_ROW_PATHS)
@pytest.mark.parametrize("name", far("p_s64_profiles_moving") + ["o_utm__s64_turn", "o_utm__s64_forced_finish_ring", "o_utm__x_s64_refused_attach_rough_wall"])
def test_far_offset_on_every_path(name, path, oracle_lib):
    """Profile columns under the moving pose at every offset (5124 .. 37672 vertical pairs with identical x and y), and at UTM coordinates the turning
    flat-ground scene, the unbroken wall ring (forced finishes) and the posts of the refused attaches: on each implementation of the segmentation."""
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "small_all"])
@pytest.mark.parametrize("name", far("s64_turn")[1:])
def test_turning_scene_at_the_coarser_offsets(name, path, oracle_lib):
    """s64_turn (720 columns) where x and y are quantised to 0.25 m and more: up to 130772 identical pairs, at 1e9 nearly every cell of a column."""
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "seg_pre", "serial", "scan_rows"])
@pytest.mark.parametrize("name", far("p_s128_profiles_moving"))
def test_far_offset_with_two_rows_per_lane(name, path, oracle_lib):
    run_case(name, path)


@pytest.mark.parametrize("path", ["fused", "small_all", "seg_small"])
@pytest.mark.parametrize("name", far("p_s40_profiles"))
def test_far_offset_with_rows_off_the_chunk_size(name, path, oracle_lib):
    run_case(name, path)


@pytest.mark.parametrize("chunks", [[1], [63]])
@pytest.mark.parametrize("path", ["small_all", "small_front", "seg_small"])
@pytest.mark.parametrize("name", cases.FAR_FIXED_POINT_CASES)
def test_far_offset_on_columns_that_take_the_label_iteration_deep(name, path, chunks, oracle_lib):
    """k_seg_small's fixed point over the labels on the staircases and the label chains with quantised coordinates: one column per call, and 63."""
    run_case(name, path, chunks=chunks)


@pytest.mark.parametrize("name", cases.FAR_FIXED_POINT_CASES)
def test_far_offset_deep_columns_on_the_row_serial_kernel(name, oracle_lib):
    run_case(name, "seg_scan", chunks=[7])


UTM_PROFILES = "o_utm__p_s64_profiles_moving"


@pytest.mark.parametrize("path", ["fused", "small_all"])
@pytest.mark.parametrize("entry", ["everything", "everything_no_terrain"])
def test_utm_profiles_with_every_threshold_off_its_default(entry, path, oracle_lib):
    stream, _, tf = case(UTM_PROFILES)
    cfg = cases.profile_config(cases.SWEEP_BASE_CASE, **cases.sweep_overrides(entry))
    run_path((UTM_PROFILES, entry), stream, cfg, tf, path)


@pytest.mark.parametrize("path", ["fused", "small_all"])
@pytest.mark.parametrize("waves", [1, 3])
def test_utm_profiles_on_the_association_kernels_alone(waves, path, oracle_lib):
    """distance 0 between different cells without the batch-parallel kernel in front: k_assoc_lds (assoc_waves 1) and k_assoc3 (3)."""
    run_case(UTM_PROFILES, path, {"assoc_batch": 0, "assoc_waves": waves})


# ---- returns at the ego box's corners -----------------------------------------------------------------------------------------------------------
def _corner_params():
    """every (pose, box) on the fused front; k_seg_pre and k_small_all on every pose, with the boxes in turn"""
    out = [(name, "fused") for name in cases.CORNER_CASES]
    for i, variant in enumerate(pose_streams.POSE_VARIANTS):
        n = len(cases.CORNER_BOXES)
        out.append((f"o_corner__{variant}__{cases.CORNER_BOXES[i % n]}", "seg_pre"))
        out.append((f"o_corner__{variant}__{cases.CORNER_BOXES[(i + 1) % n]}", "small_all"))
    return out


@pytest.mark.parametrize("name,path", _corner_params())
def test_returns_at_the_ego_box_corners(name, path, oracle_lib):
    """48 returns 2 permille inside / outside the eight corners of the box (tests/test_pose_cases_cpu.py: 44 - 48 of them are published, all inner ones
    EGO below 100 m of translation). A skip_r2 that is too small loses exactly these labels."""
    run_case(name, path)


# ---- non-finite poses -----------------------------------------------------------------------------------------------------------------------------
def _non_finite_params():
    return [(name, path) for name in cases.NON_FINITE_CASES for path in ("fused", "serial", "small_all")
            if path != "serial" or name.endswith("__s64_turn")]


@pytest.mark.parametrize("name,path", _non_finite_params())
def test_non_finite_poses(name, path, oracle_lib):
    """NaN / inf in the translation of 20 firings, in one rotation entry, in a whole pose: the oracle accepts them (status 0) and so must the engine,
    with the same cells, events and counters."""
    run_case(name, path)


# ---- many streams in one launch ---------------------------------------------------------------------------------------------------------------------
def test_pipelined_corner_streams_of_every_pose(oracle_lib):
    """The twelve corner streams of POSE_VARIANTS (default box) through cc_engine_add_firings_device, four calls of 270 firings: per-firing ego records
    of twelve different poses — finite bounds, +inf, UTM — side by side in the launches of the fused front."""
    from continuous_clustering_amd import Engine
    from test_gpu_stress import _compare_with_oracles, _feed_pipelined
    names = [f"o_corner__{variant}__default" for variant in pose_streams.POSE_VARIANTS]
    assert len(names) == 12
    streams = [case(n)[0] for n in names]
    cfg = case(names[0])[1]
    e = Engine(cfg, 64, len(streams))
    e.record_events(False)
    NB, _slots = _feed_pipelined(e, streams, 270, ring=4)
    assert NB == 4
    assert e.sync() == 0, e.last_error()
    bad = _compare_with_oracles(e, cfg, streams, NB, 270)
    fused = int(debug_counters(e)[4])
    e.close()
    assert not bad, bad[:3]
    assert fused > 0


# ---- clusters in device memory ----------------------------------------------------------------------------------------------------------------------
def test_take_clusters_at_utm_coordinates(oracle_lib):
    """s64_turn at UTM coordinates through Engine.take_clusters(6) after every rotation: descriptors against the oracle's cluster events, bounding
    boxes (min / max of values near 5.4e6) against the records, records against the published cells."""
    from test_gpu_take_clusters import FU, ClusterLog, _against_oracle, _counters, _run_device
    stream, cfg, tf = case("o_utm__s64_turn")
    assert tf is None
    cols = stream.sensor.num_columns
    NB = stream.n_firings // cols
    assert NB == 3
    log = ClusterLog(1, 6)
    e = _run_device([stream], cfg, NB, lambda e, b: log.add(*e.take_clusters(6), counters=_counters(e, 1)))
    fu = e.state(0)[FU]
    n, skipped = _against_oracle(log, 0, stream, cfg, NB * cols, fu, what="utm s64_turn")
    e.close()
    d = log.descriptors(0)
    print(f"{n} clusters, {skipped} beyond first_unpublished at the end; y from {d['min_y'].min()} to {d['max_y'].max()}")
    assert n - skipped >= 100, (n, skipped)
    assert d["min_x"].min() > 4.0e5 and d["min_y"].min() > 5.3e6
