"""CPU: conditions on the pose cases (pose_streams.py, cases.FAR_CASES / CORNER_CASES / NON_FINITE_CASES), measured on the oracle alone.
tests/test_gpu_pose_parity.py compares the engine with the oracle on exactly these inputs; what is asserted here keeps that comparison from passing
emptily: the far offsets do collapse vertically adjacent cells onto one (x, y) and change the result, the planted returns are published and sit
on either side of the ego box, both branches of ego_record's skip_r2 (finite bound / +inf) are reached, and a non-finite pose changes the output."""
import numpy as np
import pytest

import cases
import pose_streams
import util
from continuous_clustering_amd import capi

_runs = {}


def oracle_run(name):
    """(published columns, first published column, stream) of a named case; the oracle must accept it. One run per case and module."""
    if name not in _runs:
        stream, cfg, tf = cases.pose_parent(name) if not name.startswith("o_") else cases.build_case(name)
        o, rc = util.run_oracle(stream, cfg, tf)
        assert rc == 0, (name, rc, o.last_error())
        lo, hi = o.published_range()
        assert hi - lo + 1 > stream.n_firings // 2, (name, lo, hi)
        ev = o.drain_events()
        _runs[name] = (o.read_published(lo, hi), lo, stream, int((ev["type"] == capi.EV_CLUSTER).sum()))
    return _runs[name]


def identical_xy_pairs(pub):
    """Pairs of vertically adjacent returns of a column (the next row up that has a return) whose x and y are bit-identical; and those whose z is too."""
    pairs = same_z = 0
    has = ~np.isnan(pub["distance"])
    xb, yb, zb = pub["x"].view(np.uint32), pub["y"].view(np.uint32), pub["z"].view(np.uint32)
    for c in range(has.shape[0]):
        r = np.nonzero(has[c])[0]
        eq = (xb[c][r[1:]] == xb[c][r[:-1]]) & (yb[c][r[1:]] == yb[c][r[:-1]])
        pairs += int(eq.sum())
        same_z += int((eq & (zb[c][r[1:]] == zb[c][r[:-1]])).sum())
    return pairs, same_z


def cells_that_differ(a, b, fields=("ground_point_label", "debug_ground_point_label")):
    """Cells of the common published range whose labels or canonical cluster ids differ between two runs."""
    (pa, la), (pb, lb) = a[:2], b[:2]
    lo = max(la, lb)
    hi = min(la + pa["x"].shape[0], lb + pb["x"].shape[0])
    assert hi - lo >= 30, (lo, hi)
    sa, sb = slice(lo - la, hi - la), slice(lo - lb, hi - lb)
    diff = np.zeros(pa["x"][sa].shape, bool)
    for f in fields:
        diff |= pa[f][sa] != pb[f][sb]
    diff |= util.canonical_ids(pa["id"][sa]) != util.canonical_ids(pb["id"][sb])
    return diff


# ---- far offsets ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.FAR_CASES)
def test_far_offset_collapses_adjacent_cells_and_changes_the_result(name, oracle_lib):
    """Every far-offset case against the case it was made from: at least 1000 vertically adjacent pairs of returns with bit-identical x and y where
    the parent has fewer than 10, at least 100 published cells with another label or canonical id, oracle status 0. Measured — pairs (of them with
    equal z too) / parent's pairs / cells that differ / clusters (parent's):
      p_s64_profiles_moving   utm 5124 (3) / 0 / 15743 / 533 (297); 3e6_-7e6 13036 / 0 / 17970 / 546; 2^24 22858 / 0 / 24379 / 853; 1e9 37672 / 0 / 34774 / 272
      p_s128_profiles_moving  utm 11176 (17) / 0 / 16991 / 392 (395); 3e6_-7e6 25552 / 0 / 20175 / 371; 2^24 42498 / 0 / 27288 / 789; 1e9 75343 / 0 / 47882 / 408
      p_s40_profiles          utm 2157 (1) / 0 / 7597 / 342 (250); 3e6_-7e6 4720 / 0 / 7981 / 321; 2^24 10284 / 0 / 12328 / 586; 1e9 23268 / 0 / 21095 / 167
      s64_turn                utm 31234 (36) / 4 / 47353 / 838 (227); 3e6_-7e6 63601 / 4 / 76354 / 993; 2^24 99344 / 4 / 126674 / 1249; 1e9 130772 / 4 / 131702 / 245
      p_s64_label_chains utm 3314 (96) / 0 / 4813 / 18 (3); s64_forced_finish_ring utm 31028 (36) / 1 / 31622 / 406 (3)
      p_s64_alternating 2^24 2742 / 0 / 3535 / 105 (71) — under the UTM offset it has 6 pairs (its 120 firings look along -x, quantised to 3 cm), so it
      takes the 2^24 offset; x_s64_refused_attach_rough_wall utm 16168 (2555) / 2 / 20032 / 729 (62) — x_s64_refused_attach itself has 14890 pairs
      without any offset (a wall without range noise), so its wall returns get 0.2 permille of range noise first (cases.pose_parent)."""
    parent = name.partition("__")[2]
    far, near = oracle_run(name), oracle_run(parent)
    pairs, same_z = identical_xy_pairs(far[0])
    parent_pairs, _ = identical_xy_pairs(near[0])
    cells = int(cells_that_differ(far, near).sum())
    print(f"{name}: identical-xy pairs {pairs} (z too: {same_z}), parent {parent_pairs}; cells that differ {cells}; clusters {far[3]}, parent {near[3]}")
    assert pairs >= 1000 and parent_pairs < 10, (pairs, parent_pairs)
    assert cells >= 100, cells


# ---- returns at the ego box's corners ---------------------------------------------------------------------------------------------------------------
def planted_labels(name):
    """(ground_point_label, inner?) of every planted return that was published"""
    _, variant, box = name.split("__")
    pub, lo, stream, _ = oracle_run(name)
    planted = cases.corner_case(variant, box)[3]
    assert len(planted) == 48
    out = []
    for firing, row, inner in planted:
        c = np.nonzero((pub["source_firing"][:, row] == firing) & ~np.isnan(pub["distance"][:, row]))[0]
        assert len(c) <= 1
        if len(c):
            # the cell is the planted return, not a neighbour's: its sensor-frame range is the planted one
            p = stream.xyz[firing, row].astype(np.float64)
            T = stream.poses[firing].reshape(3, 4)
            assert abs(pub["distance"][c[0], row] - np.linalg.norm(T[:, :3] @ p)) <= 1e-4, name
            out.append((int(pub["ground_point_label"][c[0], row]), inner))
    return out


@pytest.mark.parametrize("name", cases.CORNER_CASES)
def test_planted_corner_returns_are_published_on_the_right_side(name, oracle_lib):
    """Every corner case publishes at least 40 of its 48 planted returns (the cell found through source_firing is the planted return: its range is
    checked). Translation below 100 m (NEAR_VARIANTS): every published inner return is GP_EGO_VEHICLE, no outer one is. UTM_VARIANTS: at least 3
    EGO and at least 3 not among them. Measured: 44 or 48 published in every case. NEAR_VARIANTS, all boxes: inner all EGO, outer none. far_1e5: inner 17 of 22 (default box), 21 of 24
    (sensor_ahead_above), 24 of 24 (tilted_tf, asymmetric_box), outer 0; scaled_1.1_far_1e5: inner 19 of 22 / 24 / 22 of 22 / 24, outer 0. utm and
    utm_f32_rotation: inner 5 of 22, outer 5 of 22 (default); 6 and 6 of 24 (sensor_ahead_above); 6 and 3 (tilted_tf); 12 and 0 (asymmetric_box);
    utm_yaw90: 6 and 3 of 22; 6 and 3; 6 and 3; 18 and 0. The asymmetric box under the UTM poses is planted with a margin of 3 percent instead of
    2 permille: with 2 permille none of the 48 returns of utm and utm_f32_rotation ends inside the box (cases.corner_case)."""
    variant = name.split("__")[1]
    got = planted_labels(name)
    inner = [lab == capi.GP_EGO_VEHICLE for lab, inn in got if inn]
    outer = [lab == capi.GP_EGO_VEHICLE for lab, inn in got if not inn]
    print(f"{name}: published {len(got)} of 48; inner EGO {sum(inner)} of {len(inner)}, outer EGO {sum(outer)} of {len(outer)}")
    assert len(got) >= 40, len(got)
    if variant in pose_streams.NEAR_VARIANTS:
        assert np.abs(pose_streams.POSE_VARIANTS[variant][[3, 7, 11]]).max() < 100.0
        assert all(inner) and not any(outer), (inner, outer)
    if variant in pose_streams.UTM_VARIANTS:
        ego = sum(inner) + sum(outer)
        assert ego >= 3 and len(got) - ego >= 3, (ego, len(got))


def test_corner_variants_reach_both_branches_of_the_skip_radius():
    """ego_record (csrc/cc_k_segment.h) gives a finite skip_r2 when the Gram deviations of the pose's and the transform's rotation blocks are below
    0.5 and +inf otherwise. From the poses alone: scaled_0.7 deviates by 0.883 (+inf); scaled_0.9 0.329, scaled_1.1 and scaled_1.1_far_1e5 0.364,
    sheared 0.134, f32_rotation and utm_f32_rotation 7e-8, the rigid ones below 1e-15 (finite). Of the transforms tilted_tf deviates by 1e-16."""
    dev = {v: pose_streams.gram_deviation(p.reshape(3, 4)) for v, p in pose_streams.POSE_VARIANTS.items()}
    print({v: float(f"{d:.3g}") for v, d in dev.items()})
    infinite = sorted(v for v, d in dev.items() if not d < 0.5)
    assert infinite == ["scaled_0.7"], infinite
    assert sum(1e-3 < d < 0.5 for d in dev.values()) >= 3          # finite, with sigma visibly below 1
    assert sum(1e-9 < d < 1e-6 for d in dev.values()) >= 2         # rounded to float32
    assert sum(d < 1e-12 for d in dev.values()) >= 4               # rigid
    for box in cases.CORNER_BOXES:
        tf = None if box == "default" else cases.EGO_SETTINGS[box][0]
        assert tf is None or pose_streams.gram_deviation(np.asarray(tf).reshape(3, 4)) < 1e-12, box


# ---- non-finite poses ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NON_FINITE_CASES)
def test_non_finite_pose_is_accepted_and_changes_published_columns(name, oracle_lib):
    """NaN / inf in the poses: the oracle returns 0, and at least one published column differs from the finite parent's (labels, canonical ids or
    which cells hold a return). Measured columns that differ (cells with another label or id / cells that lost their return), NaN and inf alike
    unless noted — s64_turn (2151 columns published either way): translation_run 21 (1304 / 1253), rotation_entry 902 (15035 / 61; inf: 15034 / 0),
    whole_pose 613 (10560 / 62); p_s64_profiles_moving (775 columns): translation_run 555 (8342 / 1209), rotation_entry 1 (54 / 54; inf: 42 / 0),
    whole_pose 193 (2411 / 56). The returns of such a firing have a NaN range (inf - inf, NaN); cc.cpp:204-238 writes them into cells that hold
    nothing valid — x, y, z, firing index, NaN distance — and they are published like that: the engine has to show the same."""
    parent = name.partition("__")[2]
    bad, good = oracle_run(name), oracle_run(parent)
    assert not np.isfinite(bad[2].poses).all() and np.isfinite(good[2].poses).all()
    diff = cells_that_differ(bad, good)
    lo = max(bad[1], good[1])
    hi = min(bad[1] + bad[0]["x"].shape[0], good[1] + good[0]["x"].shape[0])
    nan_returns = (np.isnan(bad[0]["distance"][lo - bad[1]:hi - bad[1]]) != np.isnan(good[0]["distance"][lo - good[1]:hi - good[1]]))
    columns = int((diff | nan_returns).any(axis=1).sum())
    print(f"{name}: columns that differ {columns} (cells: labels / ids {int(diff.sum())}, returns lost {int(nan_returns.sum())}); published {bad[0]['x'].shape[0]}, parent {good[0]['x'].shape[0]}")
    assert columns >= 1


# ---- the helpers themselves ---------------------------------------------------------------------------------------------------------------------------
def test_pose_helpers_change_what_they_say_and_nothing_else():
    stream = cases.build_case("p_s64_profiles_moving")[0]
    far = pose_streams.with_offset(stream, pose_streams.UTM)
    d = (far.poses - stream.poses).reshape(-1, 3, 4)
    assert np.array_equal(d[:, :, :3], np.zeros_like(d[:, :, :3])) and np.abs(d[:, :, 3] - np.array(pose_streams.UTM)).max() < 1e-9 * 5.4e6
    assert far.xyz is stream.xyz and far.intensity is stream.intensity and not np.array_equal(far.poses, stream.poses)
    rigid = pose_streams.with_constant_pose(stream, pose_streams.POSE_VARIANTS["rigid"])
    for name, fn in (("scaled_0.9", lambda R: 0.9 * R), ("sheared", lambda R: R @ pose_streams.SHEAR), ("f32_rotation", lambda R: R.astype(np.float32))):
        mapped = pose_streams.with_pose_map(rigid, fn)
        assert np.array_equal(mapped.poses, np.tile(pose_streams.POSE_VARIANTS[name], (stream.n_firings, 1))), name
    bad = pose_streams.with_non_finite(stream, np.inf, "translation_run")
    assert int((~np.isfinite(bad.poses)).sum()) == 20 and np.isfinite(stream.poses).all()
