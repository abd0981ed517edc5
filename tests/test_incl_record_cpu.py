"""CPU: the streams of tests/test_gpu_incl_record.py do what that test needs them to do — checked on the oracle alone.

A cell's inclination has one copy, .w of its record, and the record outlives the clearing of its column. The GPU test can only catch a
stale record if, in the oracle, the stale row's published inclination of pass p + 1 really differs from what pass p left in the same ring
slot; if the NaN-range returns, the two-column firings and the overrun are really there; and if the table entry the overrun test looks at
really comes from before the reset."""
import numpy as np
import pytest

import incl_record_streams as irs
from continuous_clustering_amd import capi
from oracle.pyoracle import Oracle

ROWS = (8, 12)


def _oracle(stream, cfg):
    o = Oracle(cfg, stream.sensor.num_rows)
    assert o.add_firings(stream.xyz, stream.intensity, stream.poses) == 0, o.last_error()
    return o


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("multi_column", [False, True])
def test_stale_row_has_every_return_of_the_even_passes_and_none_of_the_odd(rows, multi_column, oracle_lib):
    st = irs.stale_stream(rows, multi_column=multi_column)
    r = irs.stale_row(rows)
    odd = irs.in_odd_pass(st.n_firings)
    assert st.n_firings >= 12 * irs.RING
    assert np.isnan(st.xyz[odd, r]).all() and not np.isnan(st.xyz[~odd, r]).any()
    assert (~np.isnan(st.xyz[:, r - 1, 0])).mean() > 0.8 and (~np.isnan(st.xyz[:, r + 1, 0])).mean() > 0.8


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("supplement", [True, False])
@pytest.mark.parametrize("multi_column", [False, True])
def test_published_inclination_differs_between_two_passes_over_a_ring_slot(rows, supplement, multi_column, oracle_lib):
    """Pass p (even): the stale row's cells carry a return and its raw inclination. Pass p + 1, same ring slots: no return; the published
    inclination is NaN, or with the option the supplemented value — in no cell what pass p published there."""
    st = irs.stale_stream(rows, multi_column=multi_column)
    o = _oracle(st, irs.config(supplement))
    r = irs.stale_row(rows)
    lo, hi = o.published_range()
    assert lo == 0 and hi >= 12 * irs.RING
    edge = irs.EDGE + 4   # (the row below is altered from EDGE firings into the pass on, and a laser's offset moves its returns up to two columns)
    checked = 0
    for p in (2, 6, 10):
        even = o.read_published(p * irs.RING, (p + 1) * irs.RING - 1)
        odd = o.read_published((p + 1) * irs.RING, (p + 2) * irs.RING - 1)
        sl = slice(edge, irs.RING - edge)
        de, do_ = even["distance"][sl, r], odd["distance"][sl, r]
        ie, io = even["inclination_angle"][sl, r], odd["inclination_angle"][sl, r]
        assert not np.isnan(de).any() and not np.isnan(ie).any()
        assert np.isnan(do_).all()
        if supplement:
            filled = ~np.isnan(io)
            assert filled.mean() > 0.8   # (NaN where the row below has none either, down to the last row, and the table has no entry yet)
            same = filled & (io.view(np.uint32) == ie.view(np.uint32))
            print(f"rows {rows} pass {p}: {int(filled.sum())} supplemented cells, {int(same.sum())} equal to the previous tenant's raw value")
            assert same.sum() == 0
        else:
            assert np.isnan(io).all()
        checked += irs.RING - 2 * edge
    assert checked >= 3 * (irs.RING - 24)


@pytest.mark.parametrize("rows", ROWS)
def test_nan_range_returns_are_published_without_a_distance(rows, oracle_lib):
    st = irs.nan_range_stream(rows)
    planted = ~np.isnan(st.xyz[..., 0]) & np.isnan(st.xyz[..., 2])
    assert planted.sum() > 200 and planted[:, irs.stale_row(rows)].sum() > 20
    o = _oracle(st, irs.config(True))
    lo, hi = o.published_range()
    cols = o.read_published(lo, hi)
    # (the NaN goes through the pose into x, y and z of the odom frame: what tells such a cell from one without a return is its source firing)
    shown = np.isnan(cols["distance"]) & (cols["source_firing"] >= 0)
    print(f"rows {rows}: {int(planted.sum())} planted, {int(shown.sum())} published with their firing but no distance, "
          f"{int((~np.isnan(cols['inclination_angle'][shown])).sum())} of them with a supplemented inclination")
    assert shown.sum() > 150
    assert np.isnan(cols["z"][shown]).all()
    assert (~np.isnan(cols["inclination_angle"][shown])).sum() > 10   # (most have another such cell or the last row below them: NaN)


@pytest.mark.parametrize("rows", ROWS)
def test_rollback_firings_fill_two_columns(rows, oracle_lib):
    st = irs.rollback_stream(rows)
    fs = irs.rollback_firings(st.n_firings)
    assert len(fs) == 5
    o = _oracle(st, irs.config(True))
    lo, hi = o.published_range()
    for f in fs:
        assert lo <= f and f + 1 <= hi
        cols = o.read_published(f, f + 1)
        src = cols["source_firing"]
        assert (src[1, ::2] == f).sum() >= 2, (f, src)          # the even rows of firing f lie in the next firing's column ...
        assert (src[0, 1::2] == f).sum() >= 2, (f, src)         # ... the odd ones in its own


@pytest.mark.parametrize("rows", ROWS)
def test_overrun_and_the_table_behind_the_reset(rows, oracle_lib):
    a, b = irs.overrun_streams(rows)
    cfg = irs.overrun_config(True)
    o = Oracle(cfg, rows)
    assert o.add_firings(a.xyz, a.intensity, a.poses) == capi.CC_ERR_RING_OVERRUN, o.last_error()
    assert f", {irs.RING}" in o.last_error()
    r = irs.stale_row(rows)

    def behind_reset(oracle):
        oracle.set_config(irs.config(True))
        oracle.reset(rows)
        oracle.set_robot_from_sensor(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64))
        assert oracle.add_firings(b.xyz, b.intensity, b.poses) == 0, oracle.last_error()
        lo, hi = oracle.published_range()
        assert hi - lo > 2 * irs.COLS
        return oracle.read_published(lo, hi)["inclination_angle"][:, r]

    kept = behind_reset(o)
    fresh = behind_reset(Oracle(irs.config(True), rows))
    # the stale row never has a return behind the reset: a fresh object has no table entry for it and publishes NaN, the object that went
    # through the overrun supplements with the entry it kept
    assert np.isnan(fresh).all()
    assert (~np.isnan(kept)).mean() > 0.8
