"""CPU: conditions on the slope-controlled cases (profile_streams.py, cases.PROFILE_CASES) and on the threshold sweep (cases.SEGMENTATION_SWEEP,
cases.ASSOCIATION_SWEEP, cases.EGO_SETTINGS), measured on the oracle alone. tests/test_gpu_segmentation_sweep.py compares the engine with the oracle
on exactly these inputs; what is asserted here keeps that comparison from passing vacuously: every label of the segmentation occurs, the columns
change between ground and obstacle many times, every swept value changes the oracle's output, and every return lies on its laser's ray."""
import math

import numpy as np
import pytest

import cases
import profile_streams
import util
from continuous_clustering_amd import capi
from test_oracle_independent import Independent

LABELS = ("GRAY", "ORANGE", "GREEN", "YELLOWGREEN", "YELLOW", "RED", "DARKRED", "VIOLET")
DBG = Independent._debug_values()
_runs = {}


def oracle_run(key, build):
    """(published columns as arrays, first published column, events) of a case under a configuration; one oracle run per key and module."""
    if key not in _runs:
        stream, cfg, tf = build()
        o, rc = util.run_oracle(stream, cfg, tf)
        assert rc == 0, o.last_error()
        lo, hi = o.published_range()
        assert hi - lo + 1 > stream.n_firings // 2, (lo, hi)
        _runs[key] = (o.read_published(lo, hi), lo, o.drain_events(), cfg)
    return _runs[key]


def sweep_run(entry, name=cases.SWEEP_BASE_CASE):
    return oracle_run((name, entry), lambda: (cases.profile_stream(name), cases.profile_config(name, **cases.sweep_overrides(entry)), None))


def shares(pub):
    d = pub["debug_ground_point_label"]
    return {n: float((d == DBG[n]).mean()) for n in DBG}


def changes_per_column(pub):
    g = pub["ground_point_label"]
    out = []
    for c in range(g.shape[0]):
        lab = g[c][(g[c] == capi.GP_GROUND) | (g[c] == capi.GP_OBSTACLE)]
        out.append(int((lab[1:] != lab[:-1]).sum()))
    return np.array(out)


# ---- census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.PROFILE_CASES)
def test_every_label_occurs_and_columns_change_often(name, oracle_lib):
    """Shares of the published cells (all rows of every published column, cells without a return included). Measured: p_s64 GRAY 0.70 %, ORANGE 0.86,
    GREEN 5.1, YELLOWGREEN 23.8, YELLOW 9.7, RED 41, DARKRED 4.1, VIOLET 2.6, median 8 changes per column (max 18); p_s128 GRAY 0.37, ORANGE 0.41,
    YELLOW 5.8, YELLOWGREEN 12.4, median 10; p_s40 YELLOW 6.0, median 6; p_s50 median 7; p_s16 YELLOW 8.9, median 3."""
    pub, _, ev, _ = sweep_run("base", name)
    sh = shares(pub)
    ch = changes_per_column(pub)
    print(name, {k: round(100 * v, 2) for k, v in sh.items()}, "changes median", np.median(ch), "max", ch.max(), "clusters", int((ev["type"] == capi.EV_CLUSTER).sum()))
    for lab in LABELS:
        assert sh[lab] >= 0.003, (lab, sh[lab])
    assert sh["YELLOW"] >= 0.05 and sh["YELLOWGREEN"] >= 0.05, sh
    assert np.median(ch) >= (4 if pub["x"].shape[1] == 64 else 2), np.median(ch)
    assert (ev["type"] == capi.EV_CLUSTER).sum() >= 50


@pytest.mark.parametrize("name", cases.PROFILE_CASES)
def test_fog_thresholds_cut_through_the_data(name, oracle_lib):
    pub, _, _, _ = sweep_run("fog", name)
    sh = shares(pub)
    print(name, "LIGHTGRAY", round(100 * sh["LIGHTGRAY"], 2))
    assert sh["LIGHTGRAY"] >= 0.003
    # ... through it, not around it: returns that pass each of the three thresholds alone remain
    has = ~np.isnan(pub["distance"]) & (pub["debug_ground_point_label"] != DBG["LIGHTGRAY"]) & (pub["debug_ground_point_label"] != DBG["VIOLET"])
    assert (has & (pub["distance"] < 12.0) & (pub["inclination_angle"] > -0.25)).sum() >= 100   # bright ones
    assert (has & (pub["distance"] < 12.0) & (pub["inclination_angle"] <= -0.25)).sum() >= 100
    assert (has & (pub["distance"] >= 12.0) & (pub["inclination_angle"] > -0.25)).sum() >= 100


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------
def cells_that_differ(a, b):
    """Cells of the common published range in which two oracle runs differ: debug label, ignore flag, canonical cluster id, inclination bits."""
    (pa, la, _, _), (pb, lb, _, _) = a, b
    lo = max(la, lb)
    hi = min(la + pa["x"].shape[0], lb + pb["x"].shape[0])
    assert hi - lo > 300
    sa, sb = slice(lo - la, hi - la), slice(lo - lb, hi - lb)
    diff = np.zeros(pa["x"][sa].shape, bool)
    for f in ("debug_ground_point_label", "is_ignored"):
        diff |= pa[f][sa] != pb[f][sb]
    diff |= util.canonical_ids(pa["id"][sa]) != util.canonical_ids(pb["id"][sb])
    diff |= pa["inclination_angle"][sa].view(np.uint32) != pb["inclination_angle"][sb].view(np.uint32)
    return int(diff.sum())


def events_that_differ(a, b):
    ea, eb = a[2], b[2]
    n = min(len(ea), len(eb))
    same = np.ones(n, bool)
    for f in ("type", "a", "b", "c", "d", "column"):
        same &= ea[f][:n] == eb[f][:n]
    return int((~same).sum()) + abs(len(ea) - len(eb))


SWEEP_ENTRIES = list(cases.SEGMENTATION_SWEEP) + list(cases.ASSOCIATION_SWEEP) + ["everything", "everything_no_terrain"]


@pytest.mark.parametrize("entry", SWEEP_ENTRIES)
def test_every_sweep_entry_changes_the_oracles_output(entry, oracle_lib):
    """At least 100 cells of p_s64_profiles differ from the base configuration's run. Not in the sweep: use_last_point_for_cluster_stamp — the engine
    (like the oracle) does not read it, the reference only stamps its cluster messages with it; cluster_point_trees_every_nth_column has a case of its
    own (s64_every_2nd_column). Measured cells: use_terrain 29467, max_slope 0.05 / 0.21 / 1.0: 26541 / 12525 / 18367, first ring max 0.1 / min -0.1:
    9332 / 3737, last ground slope 0.1 / -10: 16449 / 11191, last ground distance 0.5: 13406, close z 0.05 / dist 0.3: 17118 / 11654, next obstacle
    0 / 3.0: 10206 / 14241, no supplement 5723, no inclination ignore 2074 (ignore flags of points whose clusters stay below the size that gets an
    id: no event differs), chessboard 16172, max_distance 0.05 / 3.0: 20625 / 20229, fog 11980, max_steps_in_column 1 / 3: 11308 / 11037,
    max_steps_in_row 1 / 4: 10337 / 7620, min steps 5: 11085, everything 37776 (without use_terrain 36209) of 49600 cells; the association
    entries also change 1537 - 1933 of 1932 events."""
    base, run = sweep_run("base"), sweep_run(entry)
    cells, events = cells_that_differ(base, run), events_that_differ(base, run)
    print(entry, "cells", cells, "events", events)
    assert cells >= 100 or (entry in cases.ASSOCIATION_SWEEP and events >= 100), (entry, cells, events)


def test_sweep_values_are_the_ones_of_the_base_config_moved(oracle_lib):
    """Every entry names fields of cc_config and moves them off the base configuration's values (a typo would otherwise be a silent no-op)."""
    base = cases.profile_config(cases.SWEEP_BASE_CASE)
    names = {n for n, _ in capi.Config._fields_}
    for entry in SWEEP_ENTRIES:
        over = cases.sweep_overrides(entry)
        assert over and set(over) <= names, entry
        assert any(getattr(base, k) != type(getattr(base, k))(v) for k, v in over.items()), entry


def test_terrain_gaps_case_is_decided_by_the_five_metre_bound(oracle_lib):
    """p_s64_terrain_gaps (use_terrain = 1): cells that are RED although they continue the previous point at a slope below max_slope — which only the
    5 m bound of the terrain mode does. None of the p_*_profiles cases has such a cell in front of its column's first obstacle (an engine without the
    bound in k_seg_scan passed them all), so this case carries that rule. Measured: 3095 such cells, in 792 of 805 columns."""
    pub, _, _, cfg = oracle_run(("p_s64_terrain_gaps", "own"), lambda: cases.build_case("p_s64_terrain_gaps"))
    cells = cols = 0
    for c in range(pub["x"].shape[0]):
        dbg = pub["debug_ground_point_label"][c]
        rows = [r for r in range(63, -1, -1) if not np.isnan(pub["distance"][c][r]) and dbg[r] != DBG["VIOLET"]]
        x2 = np.sqrt(pub["x"][c].astype(np.float64) ** 2 + pub["y"][c].astype(np.float64) ** 2)
        z = pub["z"][c].astype(np.float64)
        n = 0
        for below, r in zip(rows, rows[1:]):
            dx, dz = x2[r] - x2[below], z[r] - z[below]
            if dbg[r] == DBG["RED"] and dx >= 5.001 and abs(dz / dx) < 0.199:
                n += 1
        cells += n
        cols += n > 0
    print("cells", cells, "columns", cols, "of", pub["x"].shape[0])
    assert cells >= 100 and cols >= 100


# ---- ego box -----------------------------------------------------------------------------------------------------------------------
def ego_run(setting):
    return oracle_run(("ego", setting), lambda: cases.ego_case(setting))


def test_ego_settings_move_the_violet_cells(oracle_lib):
    """p_s64_profiles under the moving pose sequence: the cells inside the ego box differ between any two of the settings, the empty box holds none,
    the box larger than every return holds every return. (The case's own box, which the sweep runs under, is not in the pairs: no laser looks up by
    more than 2 degrees, so next to a sensor at the robot's origin nothing returns from above its 0.5 m; the two settings with the sensor 1 m up
    are the pair that differs in height_ref_to_maximum_ alone.)"""
    plain = oracle_run(("ego", "plain"), lambda: cases.build_case("p_s64_profiles_moving"))
    masks = {"plain": plain}
    masks.update({s: ego_run(s) for s in cases.EGO_SETTINGS})
    violet = {}
    lo = max(v[1] for v in masks.values())
    hi = min(v[1] + v[0]["x"].shape[0] for v in masks.values())
    assert hi - lo > 300
    for s, (pub, l0, _, _) in masks.items():
        violet[s] = pub["debug_ground_point_label"][lo - l0:hi - l0] == DBG["VIOLET"]
    print({s: int(v.sum()) for s, v in violet.items()})
    names = list(cases.EGO_SETTINGS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (violet[a] != violet[b]).sum() >= 100, (a, b, int((violet[a] != violet[b]).sum()))
    assert violet["empty_box"].sum() == 0
    pub, l0 = masks["huge_box"][0], masks["huge_box"][1]
    assert np.array_equal(violet["huge_box"], ~np.isnan(pub["distance"][lo - l0:hi - l0]))
    assert violet["plain"].sum() >= 100


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.PROFILE_CASES + cases.FIXED_POINT_CASES)
def test_every_return_lies_on_its_ray_and_the_generator_is_deterministic(name):
    stream, _, _ = cases.build_case(name)
    again, _, _ = cases.build_case(name)
    assert np.array_equal(stream.xyz.view(np.uint32), again.xyz.view(np.uint32)) and np.array_equal(stream.intensity, again.intensity)
    sen = stream.sensor
    incl = profile_streams.inclinations(sen)
    az = profile_streams.firing_azimuths(sen, stream.n_firings)
    x, y, z = (stream.xyz[..., i].astype(np.float64) for i in range(3))
    has = ~np.isnan(x)
    assert 0.5 < has.mean() < 0.99                       # (returns are missing, but most are there)
    t = np.sqrt(x * x + y * y + z * z)
    assert t[has].min() > profile_streams.T_MIN * 0.999 and t[has].max() < profile_streams.T_MAX * 1.001
    # coordinates are rounded to f32 (relative 2^-24 each): the angles recomputed from them are off by a few 2^-24 at most
    tol = 4 * 2.0 ** -24
    d_incl = np.arcsin(z / np.where(has, t, 1.0)) - incl[None, :]
    d_az = np.arctan2(y, x) - az[:, None]
    d_az = (d_az + math.pi) % (2 * math.pi) - math.pi
    assert np.abs(d_incl[has]).max() <= tol, np.abs(d_incl[has]).max()
    assert (np.abs(d_az) * np.cos(incl)[None, :])[has].max() <= tol
    assert stream.intensity.min() == 0 and stream.intensity.max() == 255
    if name in cases.PROFILE_SENSORS:
        other = cases.profile_stream(name, seed=77)
        assert not np.array_equal(np.isnan(other.xyz), np.isnan(stream.xyz))


# ---- fixed-point depth ---------------------------------------------------------------------------------------------------------------
def label_iteration_rounds(x2, z, valid, cfg, height_sensor_to_ground):
    """The labels of one column as the fixed point k_seg_small iterates to (csrc/cc_k_segment.h: seg_small_body), restated row by row in Python:
    every round each row recomputes its label from the labels the rows below it had in the round before. Returns (rounds until nothing changed,
    {row: label name}) — the labels before the downward fix-up, i.e. with DARKRED cells still ground."""
    F = np.float32
    idx = [r for r in range(len(x2)) if valid[r]]
    if not idx:
        return 0, {}
    prev = {r: min((q for q in idx if q > r), default=None) for r in idx}
    first = max(idx)
    h = F(z[first] - height_sensor_to_ground)
    first_ground = bool(h > F(cfg.first_ring_as_ground_min_allowed_z_diff) and h < F(cfg.first_ring_as_ground_max_allowed_z_diff))
    geo = {}
    with np.errstate(all="ignore"):
        for r in idx:
            if prev[r] is not None:
                px, py = F(x2[r] - x2[prev[r]]), F(z[r] - z[prev[r]])
                sl = F(py / px)
                geo[r] = (bool(abs(sl) < F(cfg.max_slope) and px > 0 and (not cfg.use_terrain or px < 5)),
                          bool(sl > F(cfg.last_ground_point_slope_higher_than) and abs(px) < F(cfg.last_ground_point_distance_smaller_than)))
    d = {r: ("GREEN" if geo[r][0] else "RED") for r in idx if r != first}
    d[first] = "GRAY" if first_ground else "ORANGE"
    rounds = 0
    for rounds in range(1, len(x2) + 2):
        new = dict(d)
        for r in idx:
            if r == first:
                continue
            below = [q for q in idx if q > r]
            fod = (not first_ground) or any(d[q] == "RED" for q in below)
            upd = [q for q in below if (first_ground if q == first else d[q] in ("GREEN", "YELLOWGREEN") and geo[q][1] and d[prev[q]] != "YELLOW")]
            lgx, lgz = (x2[min(upd)], z[min(upd)]) if upd else (F(0), height_sensor_to_ground)
            with np.errstate(all="ignore"):
                lx, lz = F(x2[r] - lgx), F(z[r] - lgz)
                flat_lg = bool(abs(F(lz / lx)) < F(cfg.max_slope) and lx > 0)
            green = (not fod) and geo[r][0]
            yg = (not green) and (not cfg.use_terrain) and fod and geo[r][0] and flat_lg
            ye = (not green) and (not yg) and (not cfg.use_terrain) and bool(
                abs(lx) < F(cfg.ground_because_close_to_last_certain_ground_max_dist_diff) and abs(lz) < F(cfg.ground_because_close_to_last_certain_ground_max_z_diff))
            new[r] = "GREEN" if green else "YELLOWGREEN" if yg else "YELLOW" if ye else "RED"
        if new == d:
            break
        d = new
    return rounds, d


def iteration_rounds_of_case(name):
    """Rounds per published column (static identity pose: the sensor stays at the origin), and the iteration's labels checked against the oracle's."""
    pub, _, _, cfg = oracle_run((name, "own"), lambda: cases.build_case(name))
    rounds = []
    for c in range(pub["x"].shape[0]):
        dbg = pub["debug_ground_point_label"][c]
        valid = ~np.isnan(pub["distance"][c]) & (dbg != DBG["VIOLET"]) & (dbg != DBG["LIGHTGRAY"])
        x, y = pub["x"][c], pub["y"][c]
        x2 = np.sqrt((x * x + y * y).astype(np.float32)).astype(np.float32)
        n, labels = label_iteration_rounds(x2, pub["z"][c], valid, cfg, np.float32(cfg.height_ref_to_ground_))
        for r, lab in labels.items():
            assert dbg[r] == DBG[lab] or dbg[r] == DBG["DARKRED"], (c, r, lab, dbg[r])
        rounds.append(n)
    return np.array(rounds), pub


def test_alternating_case_changes_on_every_second_row(oracle_lib):
    """64 rows, two rows of riser, two rows of tread: 2 changes per 4 rows = 32 at most; the five lasers above the horizon return nothing and 4 %
    of the rows are missing, so at least 24 in the median column (measured: 25, the maximum too). The labels settle in 2 - 3 rounds all the same:
    how often a column changes is not what makes the iteration deep — see the next test."""
    rounds, pub = iteration_rounds_of_case("p_s64_alternating")
    ch = changes_per_column(pub)
    print("changes median", np.median(ch), "max", ch.max(), "rounds median", np.median(rounds), "max", rounds.max())
    assert np.median(ch) >= 24
    assert pub["x"].shape[0] >= 90


def test_label_chain_case_needs_about_half_as_many_rounds_as_rows(oracle_lib):
    """A period of four rows (wall YELLOW, flat, wall RED, flat that moves the last ground point) settles every two rounds: rows / 2 = 32 rounds for
    a complete column, fewer where a row is missing or the column is plain ground. Measured: median 20, 90th percentile and maximum 33
    (flat-ground scenes: 2; p_s64_profiles: median 5, maximum 13)."""
    rounds, pub = iteration_rounds_of_case("p_s64_label_chains")
    print("rounds median", np.median(rounds), "p90", np.percentile(rounds, 90), "max", rounds.max())
    assert rounds.max() >= 32
    assert np.median(rounds) >= 16
    assert pub["x"].shape[0] >= 90
