"""CPU: conditions on the degenerate and extreme returns (return_streams.py, cases.RETURN_CASES), measured on the oracle alone.
tests/test_gpu_return_parity.py compares the engine with the oracle on exactly these inputs; what is asserted here keeps that comparison from passing
emptily: every class is accepted (status 0), its planted returns are there in number, they reach published cells under their own firing index (or,
for a NaN azimuth, are dropped with the error text), and the values the class is about — infinite ranges and coordinates, NaN ranges, the column
index num_columns, reset_required — do occur. Every minimum below is 80 % of what the oracle gave (MEASURED), never a figure of the engine.

What the oracle showed that the classes' names do not say:
  x, y = +-inf      atan2f gives 0, +-pi/2 or pi: all planted returns of a rotation aim at one column. An infinite range never replaces a return and is
                    never replaced by the shift rule, so 1 - 7 of 350 - 1700 stay in published cells. Under a pose whose rotation block has a zero in the
                    row (the static identity pose of the profile streams) 0 * inf = NaN: the cell holds (inf, NaN, NaN) and a NaN range; the range is
                    infinite only under the moving pose (r_*__p_s64_profiles_moving), where no entry is zero.
  all three inf     under the identity pose every odom coordinate is NaN (0 * inf), so no published cell holds an infinity: counted by its NaN
                    coordinates under the planted firing index instead.
  z = NaN           every odom coordinate has the term r_i2 * z: x, y and z of the cell are NaN under any pose, the range is NaN, the firing index is
                    the planted one. "NaN range with finite x, y" cannot occur.
  x 1e36            ranges are below 150 m here, so the float32 range stays finite (it would overflow from 340 m on): scaled_overflow scales every
                    return so that its range is 1.02 x FLT_MAX with finite coordinates and gives the infinite ranges.
  (-0, -0, -0)      column num_columns (clockwise) or 0 (counter-clockwise); reset_required needs that column to lie more than half a rotation behind
                    the firing's own, which where every firing has a return takes a lost firing at half a rotation: planted with the class.
  gap > half        after a run of num_columns / 2 + 1 empty firings every return counts as one rotation back and is dropped as too far behind,
                    until the sensor is back at the column behind the previous rearmost one: the rest of that rotation is lost (415 of 810
                    columns published), without reset_required and with status 0. That is the reference's behaviour and the one to match."""
import numpy as np
import pytest

import cases
import return_streams as rs
import util
from continuous_clustering_amd import capi
from test_oracle_independent import check_against_the_oracle

# name -> (planted returns, planted returns in published cells under their own firing index, published cells with an infinite coordinate or range,
#          with an infinite range, with a NaN range under a firing index, clusters, published columns, reset_required) — the oracle's figures
MEASURED = {
    "r_zero__p_s64_profiles": (423, 105, 0, 0, 0, 308, 775, 0),
    "r_negzero__p_s64_profiles": (613, 121, 0, 0, 0, 315, 775, 1),
    "r_ypos0_xneg__p_s64_profiles": (470, 112, 0, 0, 0, 311, 775, 0),
    "r_yneg0_xneg__p_s64_profiles": (443, 111, 0, 0, 0, 311, 775, 0),
    "r_xpos0__p_s64_profiles": (345, 97, 0, 0, 0, 324, 775, 0),
    "r_xneg0__p_s64_profiles": (550, 158, 0, 0, 0, 314, 775, 0),
    "r_scaled_1e-42__p_s64_profiles": (448, 440, 0, 0, 0, 317, 775, 0),
    "r_scaled_1e-30__p_s64_profiles": (444, 398, 0, 0, 0, 316, 775, 0),
    "r_scaled_1e6__p_s64_profiles": (540, 482, 0, 0, 0, 315, 775, 0),
    "r_scaled_1e18__p_s64_profiles": (436, 410, 0, 0, 0, 314, 775, 0),
    "r_scaled_1e36__p_s64_profiles": (536, 490, 0, 0, 0, 313, 775, 0),
    "r_scaled_overflow__p_s64_profiles": (659, 607, 542, 542, 0, 310, 775, 0),
    "r_x_pinf__p_s64_profiles": (408, 6, 6, 0, 6, 308, 775, 0),
    "r_x_ninf__p_s64_profiles": (549, 4, 4, 0, 4, 310, 775, 0),
    "r_y_pinf__p_s64_profiles": (345, 3, 3, 0, 3, 310, 775, 0),
    "r_y_ninf__p_s64_profiles": (589, 6, 6, 0, 6, 312, 775, 0),
    "r_z_pinf__p_s64_profiles": (446, 386, 386, 0, 386, 318, 775, 0),
    "r_z_ninf__p_s64_profiles": (534, 534, 534, 0, 534, 308, 775, 0),
    "r_all_inf__p_s64_profiles": (691, 7, 0, 0, 7, 310, 775, 0),
    "r_z_nan__p_s64_profiles": (474, 458, 0, 0, 458, 312, 775, 0),
    "r_y_nan__p_s64_profiles": (595, 0, 0, 0, 0, 312, 775, 0),
    "r_yz_nan__p_s64_profiles": (441, 0, 0, 0, 0, 313, 775, 0),
    "r_edge_lo_exact__p_s64_profiles": (909, 909, 0, 0, 0, 315, 775, 0),
    "r_edge_lo_below__p_s64_profiles": (1070, 1070, 0, 0, 0, 316, 775, 0),
    "r_edge_hi_exact__p_s64_profiles": (843, 843, 0, 0, 0, 310, 775, 0),
    "r_edge_hi_below__p_s64_profiles": (1069, 1009, 0, 0, 0, 316, 775, 0),
    "r_edge_hi_above__p_s64_profiles": (729, 669, 0, 0, 0, 312, 775, 0),
    "r_edge_straddle__p_s64_profiles": (727, 727, 0, 0, 0, 322, 775, 0),
    "r_dup_rows__p_s64_profiles": (1408, 1408, 0, 0, 0, 324, 775, 0),
    "r_dup_firings__p_s64_profiles": (2405, 1002, 0, 0, 0, 328, 797, 0),
    "r_one_row0__p_s64_profiles": (22, 19, 0, 0, 0, 316, 775, 0),
    "r_one_last__p_s64_profiles": (22, 21, 0, 0, 0, 310, 775, 0),
    "r_one_mid__p_s64_profiles": (22, 20, 0, 0, 0, 318, 775, 0),
    "r_gap_1__p_s64_profiles": (617, 0, 0, 0, 0, 314, 775, 0),
    "r_gap_10__p_s64_profiles": (6167, 0, 0, 0, 0, 306, 777, 0),
    "r_gap_half_minus__p_s64_profiles": (9994, 0, 0, 0, 0, 244, 775, 0),
    "r_gap_half_plus__p_s64_profiles": (10104, 0, 0, 0, 0, 183, 415, 0),
    "r_gap_rotation__p_s64_profiles": (20624, 0, 0, 0, 0, 178, 415, 0),
    "r_zero__p_s64_profiles_ccw": (511, 117, 0, 0, 0, 307, 775, 0),
    "r_negzero__p_s64_profiles_ccw": (503, 118, 0, 0, 0, 316, 775, 1),
    "r_ypos0_xneg__p_s64_profiles_ccw": (441, 114, 0, 0, 0, 313, 775, 0),
    "r_yneg0_xneg__p_s64_profiles_ccw": (610, 121, 0, 0, 0, 313, 775, 0),
    "r_xpos0__p_s64_profiles_ccw": (483, 162, 0, 0, 0, 317, 775, 0),
    "r_xneg0__p_s64_profiles_ccw": (656, 155, 0, 0, 0, 316, 775, 0),
    "r_zero__p_s128_profiles": (909, 237, 0, 0, 0, 395, 733, 0),
    "r_yneg0_xneg__p_s128_profiles": (1063, 191, 0, 0, 0, 392, 733, 0),
    "r_edge_hi_exact__p_s128_profiles": (1440, 1440, 0, 0, 0, 398, 733, 0),
    "r_edge_straddle__p_s128_profiles": (1436, 1323, 0, 0, 0, 428, 733, 0),
    "r_scaled_1e-42__p_s128_profiles": (1062, 954, 0, 0, 0, 390, 733, 0),
    "r_scaled_1e36__p_s128_profiles": (943, 854, 0, 0, 0, 390, 733, 0),
    "r_all_inf__p_s128_profiles": (1234, 20, 0, 0, 20, 391, 733, 0),
    "r_z_nan__p_s128_profiles": (653, 589, 0, 0, 589, 392, 733, 0),
    "r_y_nan__p_s128_profiles": (966, 0, 0, 0, 0, 392, 733, 0),
    "r_dup_firings__p_s128_profiles": (4987, 1884, 0, 0, 0, 392, 735, 0),
    "r_gap_half_plus__p_s128_profiles": (19132, 0, 0, 0, 0, 243, 393, 0),
    "r_one_mid__p_s128_profiles": (21, 19, 0, 0, 0, 383, 733, 0),
    "r_zero__p_s40_profiles": (277, 79, 0, 0, 0, 251, 799, 0),
    "r_yneg0_xneg__p_s40_profiles": (319, 61, 0, 0, 0, 252, 799, 0),
    "r_edge_hi_exact__p_s40_profiles": (555, 555, 0, 0, 0, 246, 800, 0),
    "r_edge_straddle__p_s40_profiles": (492, 492, 0, 0, 0, 248, 799, 0),
    "r_scaled_1e-42__p_s40_profiles": (295, 285, 0, 0, 0, 247, 799, 0),
    "r_scaled_1e36__p_s40_profiles": (319, 312, 0, 0, 0, 250, 799, 0),
    "r_all_inf__p_s40_profiles": (316, 7, 0, 0, 7, 247, 799, 0),
    "r_z_nan__p_s40_profiles": (333, 329, 0, 0, 329, 243, 799, 0),
    "r_y_nan__p_s40_profiles": (357, 0, 0, 0, 0, 248, 799, 0),
    "r_dup_firings__p_s40_profiles": (1861, 633, 0, 0, 0, 256, 803, 0),
    "r_gap_half_plus__p_s40_profiles": (6061, 0, 0, 0, 0, 143, 439, 0),
    "r_one_mid__p_s40_profiles": (22, 22, 0, 0, 0, 243, 799, 0),
    "r_scaled_1e-42__s64_forced_finish_ring": (1627, 1099, 0, 0, 0, 3, 1080, 0),
    "r_scaled_1e-30__s64_forced_finish_ring": (1387, 920, 0, 0, 0, 3, 1080, 0),
    "r_scaled_1e6__s64_forced_finish_ring": (1293, 805, 0, 0, 0, 3, 1080, 0),
    "r_scaled_1e18__s64_forced_finish_ring": (1360, 951, 0, 0, 0, 5, 1080, 0),
    "r_scaled_1e36__s64_forced_finish_ring": (1274, 830, 0, 0, 0, 3, 1080, 0),
    "r_scaled_overflow__s64_forced_finish_ring": (1337, 940, 745, 745, 0, 3, 1080, 0),
    "r_x_pinf__s64_forced_finish_ring": (1316, 3, 3, 0, 3, 3, 1080, 0),
    "r_x_ninf__s64_forced_finish_ring": (1284, 1, 1, 0, 1, 3, 1080, 0),
    "r_y_pinf__s64_forced_finish_ring": (1337, 1, 1, 0, 1, 3, 1080, 0),
    "r_y_ninf__s64_forced_finish_ring": (1168, 3, 3, 0, 3, 3, 1080, 0),
    "r_z_pinf__s64_forced_finish_ring": (1525, 994, 994, 0, 994, 3, 1080, 0),
    "r_z_ninf__s64_forced_finish_ring": (1295, 813, 813, 0, 813, 3, 1080, 0),
    "r_all_inf__s64_forced_finish_ring": (1664, 3, 0, 0, 3, 3, 1080, 0),
    "r_dup_rows__s64_forced_finish_ring": (3456, 2240, 0, 0, 0, 3, 1080, 0),
    "r_dup_firings__s64_forced_finish_ring": (7164, 2765, 0, 0, 0, 36, 1426, 0),
    "r_z_nan__s64_forced_finish_ring": (1312, 838, 0, 0, 838, 3, 1080, 0),
    "r_x_pinf__p_s64_profiles_moving": (596, 68, 68, 68, 0, 297, 775, 0),
    "r_x_ninf__p_s64_profiles_moving": (534, 67, 67, 67, 0, 298, 775, 0),
    "r_y_pinf__p_s64_profiles_moving": (577, 69, 69, 69, 0, 299, 775, 0),
    "r_y_ninf__p_s64_profiles_moving": (545, 68, 68, 68, 0, 300, 775, 0),
    "r_z_pinf__p_s64_profiles_moving": (436, 386, 386, 386, 0, 297, 775, 0),
    "r_z_ninf__p_s64_profiles_moving": (554, 540, 540, 540, 0, 303, 775, 0),
    "r_all_inf__p_s64_profiles_moving": (542, 7, 0, 0, 7, 298, 775, 0),
    "r_mixed__w_s64_240x13": (4296, 1809, 225, 55, 244, 2079, 3116, 1),
}


def measure(name):
    stream, cfg, tf, mask = cases.return_case(name)
    o, rc = util.run_oracle(stream, cfg, tf)
    lo, hi = o.published_range()
    pub = o.read_published(lo, hi)
    ev = o.drain_events()
    rows = stream.sensor.num_rows
    src = pub["source_firing"].astype(np.int64)
    keys = np.where(src >= 0, src * rows + np.arange(rows)[None, :], -1)
    f, r = np.nonzero(mask)
    own = np.isin(keys, f * rows + r)
    inf = np.isinf(pub["distance"]) | np.isinf(pub["x"]) | np.isinf(pub["y"]) | np.isinf(pub["z"])
    nan_range = np.isnan(pub["distance"]) & (src >= 0)
    return dict(rc=rc, error=o.last_error(), state=o.state(), stream=stream, mask=mask, pub=pub, own=own, lo=lo, cfg=cfg,
                figures=(int(mask.sum()), int(own.sum()), int(inf.sum()), int(np.isinf(pub["distance"]).sum()), int(nan_range.sum()),
                         int((ev["type"] == capi.EV_CLUSTER).sum()), hi - lo + 1, int(o.state()["reset_required"])))


def class_of(name):
    return name[2:].partition("__")[0]


def empty_runs(stream):
    """lengths of the runs of firings without any return"""
    empty = np.isnan(stream.xyz[..., 0]).all(axis=1)
    runs, k = [], 0
    for e in empty:
        if e:
            k += 1
        elif k:
            runs.append(k)
            k = 0
    return runs + ([k] if k else [])


@pytest.mark.parametrize("name", cases.RETURN_CASES)
def test_planted_returns_reach_the_cells_or_are_dropped(name, oracle_lib):
    """Per case, on the oracle: status 0; at least 100 planted returns (the one_* classes: at least 20 firings with exactly one return; the gap_*
    classes: runs of exactly the stated length); at least 80 % of MEASURED's planted returns in published cells under their own firing index — none
    for the NaN azimuths, which leave the error text; at least 80 % of MEASURED's infinite and NaN-range cells; reset_required as in MEASURED."""
    cls = class_of(name)
    m = measure(name)
    planted, own, inf, inf_range, nan_range, clusters, columns, reset = m["figures"]
    print(f'"{name}": {m["figures"]},')
    assert m["rc"] == 0, (m["rc"], m["error"])
    want = MEASURED[name]
    stream, mask = m["stream"], m["mask"]
    cols = stream.sensor.num_columns
    if cls in rs.GAP_CLASSES:
        runs = empty_runs(stream)
        assert runs and all(k == rs.gap_length(cls, cols) for k in runs), runs
    elif cls in rs.ONE_CLASSES:
        lone = (~np.isnan(stream.xyz[..., 0])).sum(axis=1) == 1
        assert planted >= 20 and lone[mask.any(axis=1)].all() and lone.sum() == planted
        row = {"one_row0": 0, "one_last": stream.sensor.num_rows - 1, "one_mid": stream.sensor.num_rows // 2}[cls]
        assert mask[:, row].sum() == planted
    else:
        assert planted >= 100, planted
    assert not mask[:cols].any()                         # the first rotation is the parent's
    if cls in rs.DROPPED_CLASSES:
        assert m["error"] == "negative global column index" and own == 0
    elif cls not in rs.GAP_CLASSES:
        assert want[1] >= 1 and own >= 0.8 * want[1], (own, want[1])
        if cls != "mixed":
            assert m["error"] == ""
    if cls in rs.INF_CLASSES + ("scaled_overflow", "mixed"):
        assert inf >= 0.8 * want[2] and inf_range >= 0.8 * want[3], (inf, inf_range, want)
        if cls != "all_inf":
            assert want[2] >= 1
    if cls in ("scaled_overflow", "mixed") or (cls in ("x_pinf", "x_ninf", "y_pinf", "y_ninf") and name.endswith("_moving")):
        assert want[3] >= 3
    if cls in ("z_nan", "all_inf", "mixed") or (cls in rs.INF_CLASSES and not name.endswith("_moving")):
        # NaN range under the planted firing index; z = NaN and all-inf: x and y are NaN too (0 * inf, r_i2 * NaN)
        assert want[4] >= 1 and nan_range >= 0.8 * want[4], (nan_range, want[4])
        if cls in ("z_nan", "all_inf") and not name.endswith("_moving"):
            cells = m["own"] & np.isnan(m["pub"]["distance"])
            assert cells.sum() >= 0.8 * want[4] and np.isnan(m["pub"]["x"][cells]).all() and np.isnan(m["pub"]["y"][cells]).all()
    if cls == "negzero":
        assert reset == 1
    assert reset == want[7], (reset, want[7])
    assert clusters >= 0.8 * want[5] and columns >= 0.8 * want[6]


def test_measured_table_lists_every_case():
    assert sorted(MEASURED) == sorted(cases.RETURN_CASES)


@pytest.mark.parametrize("num_columns", [240, 360, 720, 2200])
def test_column_index_num_columns_occurs(num_columns):
    """inc_az = pi_f + pi_f (azimuth -pi of a clockwise sensor: y = -0 with x < 0) divided by the float32 az_width: the quotient is exactly
    num_columns at 240, 360, 720 and 2200 columns (of the column counts the cases use it is one float32 below at 340 and 680), so the column index
    num_columns does occur, and 0 for the azimuth +pi. The r_* cases have 360 and 240 columns."""
    q = rs.column_quotient(-3.0, -0.0, num_columns, True)
    print(num_columns, repr(q), repr(rs.az_width(num_columns)))
    assert int(q) == num_columns
    assert int(rs.column_quotient(-3.0, 0.0, num_columns, True)) == 0
    assert int(rs.column_quotient(-3.0, 0.0, num_columns, False)) == num_columns and int(rs.column_quotient(-3.0, -0.0, num_columns, False)) == 0
    for odd in (340, 680):
        assert int(rs.column_quotient(-3.0, -0.0, odd, True)) == odd - 1


@pytest.mark.parametrize("cls", rs.EDGE_CLASSES)
def test_edge_returns_land_where_the_boundary_says(cls, oracle_lib):
    """The planted firings of an edge class on the oracle: every planted return's quotient inc_az / az_width is exactly the integer or its float32
    neighbour, and its published cell lies in the column that quotient truncates to, or — the shift rule — in the next one. Firings of the last
    column of a rotation on their upper boundary give the column index num_columns: published in column 0 of the next rotation (edge_hi_exact,
    edge_straddle: at least 25 such returns; measured 55 and 28)."""
    name = f"r_{cls}__{cases.RETURN_BASE_CASE}"
    m = measure(name)
    stream, mask, pub, cols = m["stream"], m["mask"], m["pub"], m["stream"].sensor.num_columns
    rows = stream.sensor.num_rows
    where = {}
    for c, r in np.argwhere(m["own"]):
        where[(int(pub["source_firing"][c, r]), int(r))] = int(pub["global_column_index"][c, r])
    on_boundary = wrapped = shifted = 0
    for f, r in np.argwhere(mask):
        q = rs.column_quotient(stream.xyz[f, r, 0], stream.xyz[f, r, 1], cols, True)
        k = round(float(q))
        assert abs(float(q) - k) <= 2 * float(np.spacing(np.float32(max(k, 1)))), (f, r, q)
        on_boundary += int(float(q) == k)
        if (f, r) in where:
            rotation = f // cols
            expected = rotation * cols + int(q)
            assert where[(f, r)] in (expected, expected + 1), (f, r, q, where[(f, r)], expected)
            shifted += int(where[(f, r)] == expected + 1)
            wrapped += int(int(q) == cols)
    print(f"{cls}: planted {int(mask.sum())}, published {len(where)}, exactly on the boundary {on_boundary}, moved on by the shift rule {shifted}, column index num_columns {wrapped}")
    assert len(where) >= 500
    if cls in ("edge_lo_exact", "edge_hi_exact"):
        assert on_boundary == int(mask.sum())
    if cls in ("edge_hi_exact", "edge_straddle"):
        assert wrapped >= 25, wrapped


def test_mixed_case_holds_every_class():
    """The ring-wrap case: every class of MIXED_CLASSES planted at least once, together 1.5 - 3 % of the valid returns, through 13 rotations."""
    stream, cfg, tf = cases.build_case(cases.RETURN_MIXED_PARENT)
    planted, mask, counts = rs.plant_mixed(stream, cases.return_seed(cases.RETURN_MIXED_CASE))
    print(counts, int(mask.sum()))
    assert sorted(counts) == sorted(rs.MIXED_CLASSES) and all(v > 0 for v in counts.values()), counts
    share = mask.sum() / (~np.isnan(stream.xyz[..., 0])).sum()
    assert 0.015 < share < 0.03, share
    assert stream.n_firings == 13 * 240 and cfg.num_columns == 240
    assert np.array_equal(mask, cases.return_case(cases.RETURN_MIXED_CASE)[3])


def test_plant_leaves_its_argument_and_the_rest_alone():
    stream = cases.build_case(cases.RETURN_BASE_CASE)[0]
    before = stream.xyz.copy()
    for cls in ("zero", "y_nan", "scaled_overflow", "dup_rows", "one_mid", "gap_10"):
        planted, mask = rs.plant(stream, cls, 5)
        assert np.array_equal(stream.xyz, before, equal_nan=True)
        changed = rs.changed_returns(planted, stream)
        if cls in rs.RETURN_CLASSES:
            assert np.array_equal(changed, mask)
        again, mask2 = rs.plant(stream, cls, 5)
        assert np.array_equal(again.xyz, planted.xyz, equal_nan=True) and np.array_equal(mask, mask2)
    over = rs.plant(stream, "scaled_overflow", 5)[0].xyz
    assert np.isfinite(over[~np.isnan(over)]).all()


# ---- the independent restatement of insertion + segmentation on the planted classes -----------------------------------------------------------------
@pytest.mark.parametrize("name", cases.RETURN_S64_CASES + [f"r_{cls}__{cases.RETURN_BASE_CASE}_ccw" for cls in ("negzero", "ypos0_xneg")])
def test_second_restatement_agrees_with_the_oracle_on_planted_returns(name, oracle_lib):
    """tests/test_oracle_independent.py's restatement against the oracle on every class (64 x 360 parent): equal in every published column's
    geometry bits, firing indices, labels, ignore flags and in the ring bookkeeping, for every class. (Its comparison of the firing indices used to
    mask cells without a valid range; a return with a NaN range is published with its firing index, so the mask is gone.)"""
    with np.errstate(all="ignore"):                      # (the restatement computes with inf and NaN on purpose)
        check_against_the_oracle(*cases.build_case(name))
