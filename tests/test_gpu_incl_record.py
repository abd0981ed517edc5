"""GPU: a cell's inclination lives in its record only (Planes::sc_rec.w, cc_device.h), and the record is not cleared with its column.

Every case compares EVERY field of the column view with the oracle (util.compare_columns) on the smallest shapes a stale record can show
at: 8 and 12 rows, 64 columns per rotation (a ring of 640 columns), 13 passes over the ring (tests/incl_record_streams.py;
tests/test_incl_record_cpu.py shows on the oracle alone that the streams do what these cases need). What must never be seen is the
previous tenant's record behind a cell that is cleared, or not written yet:
  * the stale row (a return in every column of pass p, none in pass p + 1), supplement on and off, on the fused path (single-column firings,
    three block shapes of k_insert_par) and on the unfused path, where k_table and k_seg_pre read the ring (multi-column firings; the fused
    front off; the serial insertion), in calls of 128, 97, 5 and 1 firings;
  * a column read through the view while it is filled but not segmented;
  * returns with a NaN range; firings that make the block-parallel insertion take cells back; an overrun of the ring and the table behind
    the reset; four streams side by side through the device entry."""
import re

import numpy as np
import pytest

import incl_record_streams as irs
import util
from continuous_clustering_amd import capi

pytestmark = pytest.mark.gpu

ROWS = (8, 12)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
# block shapes of k_insert_par: one stream by default gets 8 blocks of 16 wavefronts; one such block; one block of 8 wavefronts, the shape of
# launches of more than 160 streams
SHAPES = {"split8": None, "wide1": ("insert_split_blocks", 1), "narrow": ("insert_wide_max_streams", 0)}
CHUNKS = [128, 97, 5, 1]   # (a call stays well below the ring: what a call publishes must still be there when the host reads it)

_streams, _records = {}, {}


def _stream(kind, rows, multi_column=False):
    key = (kind, rows, multi_column)
    if key not in _streams:
        make = {"stale": irs.stale_stream, "nan_range": irs.nan_range_stream, "rollback": irs.rollback_stream}[kind]
        _streams[key] = make(rows, multi_column=True) if multi_column else make(rows)
    return _streams[key]


def _record(kind, rows, supplement, multi_column=False):
    """(stream, configuration, the oracle's record of it): computed once, shared by the cases, never changed."""
    key = (kind, rows, supplement, multi_column)
    if key not in _records:
        st, cfg = _stream(kind, rows, multi_column), irs.config(supplement)
        _records[key] = (st, cfg, util.oracle_record(st, cfg))
    return _records[key]


def _debug_counters(e):
    import ctypes as C
    from continuous_clustering_amd import load_library
    L = load_library()
    L.cc_engine_debug_counters.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    out = np.zeros(16, dtype=np.uint64)
    L.cc_engine_debug_counters(e.h, 0, out.ctypes.data)
    return out


def _run(kind, rows, supplement, option=None, multi_column=False, chunks=CHUNKS):
    st, cfg, rec = _record(kind, rows, supplement, multi_column)
    box = {}

    def setup(e):
        box["e"] = e
        if option is not None:
            e.set_option(*option)

    s = util.run_and_compare(st, cfg, chunks=chunks, engine_setup=setup, oracle=rec)
    assert s["published_columns"] > 12 * irs.RING, "fewer than 12 passes over the ring"
    assert s["engine_state"]["ring_buffer_start_global_column_index"] > 11 * irs.RING
    return s, int(_debug_counters(box["e"])[4])   # (batches k_insert_par closed as fused)


def _calls(n, chunks):
    sizes, f, i = [], 0, 0
    while f < n:
        sizes.append(min(chunks[i % len(chunks)], n - f))
        f += sizes[-1]
        i += 1
    return sizes


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("supplement", [True, False], ids=["supplement", "plain"])
@pytest.mark.parametrize("rows", ROWS)
def test_stale_record_behind_a_cleared_cell_fused(rows, supplement, shape, oracle_lib):
    s, fused = _run("stale", rows, supplement, SHAPES[shape])
    big = sum(1 for m in _calls(_stream("stale", rows).n_firings, CHUNKS) if m >= 64)
    assert fused >= big - 2, (fused, big)   # (every call of 64 firings or more but the first one or two)


@pytest.mark.parametrize("path", ["multi_column", "fuse_front_off", "serial_insert"])
@pytest.mark.parametrize("supplement", [True, False], ids=["supplement", "plain"])
@pytest.mark.parametrize("rows", ROWS)
def test_stale_record_behind_a_cleared_cell_unfused(rows, supplement, path, oracle_lib):
    """k_table and k_seg_pre read the ring: a stream that starts out of the steady state and whose firings span three columns (no batch is
    fused), and the single-column stream with the fused front off and with the serial insertion kernel."""
    option = {"multi_column": None, "fuse_front_off": ("fuse_front", 0), "serial_insert": ("parallel_insert", 0)}[path]
    s, fused = _run("stale", rows, supplement, option, multi_column=path == "multi_column")
    assert fused == 0, fused


@pytest.mark.parametrize("rows", ROWS)
def test_column_read_before_it_is_segmented(rows, oracle_lib):
    """After a call the column of its last firing is filled but not segmented. Through the view it shows the returns it has — distance, x, y,
    z, source firing and RAW inclination as the oracle publishes them later — and NaN in every other cell, the stale row of the odd passes
    included, behind which the previous pass's record lies."""
    from continuous_clustering_amd import Engine
    st, cfg, (oracle, orc, _) = _record("stale", rows, True)
    assert orc == 0
    e = Engine(cfg, rows)
    r = irs.stale_row(rows)
    f, seen_odd, seen_even = 0, 0, 0
    for m in _calls(5 * irs.RING, [120, 64, 1, 77]):
        assert e.add_firings(st.xyz[f:f + m], st.intensity[f:f + m], st.poses[f:f + m]) == 0, e.last_error()
        f += m
        se = e.state()
        g = se["first_unfinished_global_column_index"]
        assert g == f - 1   # (single-column firings from column 0 on)
        v, pub = e.read_columns(g, g), oracle.read_published(g, g)
        has = ~np.isnan(pub["distance"])
        assert has.sum() >= rows // 2
        for fld in ("x", "y", "z", "distance"):
            util.assert_float_equal(f"{fld} of unsegmented column {g}", np.where(has, pub[fld], np.float32(np.nan)), v[fld])
        util.assert_float_equal(f"inclination_angle of unsegmented column {g}", np.where(has, pub["inclination_angle"], np.float32(np.nan)),
                                v["inclination_angle"])
        assert np.array_equal(v["source_firing"], np.where(has, pub["source_firing"], -1))
        assert (v["global_column_index"] == np.where(has, g, -1)).all() and (v["is_ignored"] == 0).all() and (v["id"] == 0).all()
        if (g // irs.RING) % 2 == 1 and g >= irs.RING:
            seen_odd += 1
            assert not has[0, r] and np.isnan(v["inclination_angle"][0, r])
        elif g >= 2 * irs.RING:
            seen_even += 1
            assert has[0, r]
    assert seen_odd >= 4 and seen_even >= 2
    e.close()


@pytest.mark.parametrize("option", [None, ("fuse_front", 0)], ids=["fused", "unfused"])
@pytest.mark.parametrize("rows", ROWS)
def test_returns_with_a_nan_range(rows, option, oracle_lib):
    """x, y, z and source firing of such a return are published, its inclination is the oracle's (NaN, or the supplemented value)."""
    _run("nan_range", rows, True, option)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("rows", ROWS)
def test_roll_back_of_firings_behind_one_that_leaves_the_shape(rows, shape, oracle_lib):
    """par_take_back: state and columns equal the oracle's after every call, the calls behind it included."""
    s, fused = _run("rollback", rows, True, SHAPES[shape], chunks=[128, 97])
    assert fused >= 4


@pytest.mark.parametrize("chunks", [[97], [128, 5]], ids=["calls_of_97", "calls_of_128_5"])
@pytest.mark.parametrize("rows", ROWS)
def test_overrun_then_reset_restores_the_inclination_table(rows, chunks, oracle_lib):
    """The recipe of tests/test_gpu_ringwrap.py::test_deliberate_ring_overrun on the smallest ring, then reset (which keeps the table of
    inclination steps, cc.cpp:46) and a stream whose stale row has no return: its supplemented inclinations are the table entry of before the
    reset plus the row below, so they show whether the table was rebuilt as of the column in front of the stale one."""
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    a, b = irs.overrun_streams(rows)
    cfg = irs.overrun_config(True)
    o = Oracle(cfg, rows)
    assert o.add_firings(a.xyz, a.intensity, a.poses) == capi.CC_ERR_RING_OVERRUN, o.last_error()
    stale, col, ring = (int(v) for v in re.search(r": (-?\d+), (-?\d+), (\d+)", o.last_error()).groups())
    assert ring == irs.RING and stale == col - ring
    e = Engine(cfg, rows)
    rc = f = 0
    for m in _calls(a.n_firings, chunks):
        rc = e.add_firings(a.xyz[f:f + m], a.intensity[f:f + m], a.poses[f:f + m])
        f += m
        if rc != 0:
            break
    assert rc == capi.CC_ERR_RING_OVERRUN, (rc, e.last_error())
    assert f"{stale}, {col}, {ring}" in e.last_error(), (e.last_error(), o.last_error())
    o.drain_events()
    for x in (o, e):
        x.reset(rows)
        x.set_config(irs.config(True))
        x.set_robot_from_sensor(IDENTITY)
    e.drain_events()
    assert o.add_firings(b.xyz, b.intensity, b.poses) == 0, o.last_error()
    eo = o.drain_events()
    f = ev_pos = 0
    shown = []
    for m in _calls(b.n_firings, chunks):
        assert e.add_firings(b.xyz[f:f + m], b.intensity[f:f + m], b.poses[f:f + m]) == 0, e.last_error()
        f += m
        ev_pos, pub = util.compare_events(eo, e.drain_events(), ev_pos)
        if pub is not None:
            got = e.read_columns(*pub)
            util.compare_columns(o.read_published(*pub), got, pub[0])
            shown.append(got["inclination_angle"][:, irs.stale_row(rows)])
    assert ev_pos == len(eo)
    so, se = o.state(), e.state()
    for k in util.STATE_FIELDS:
        assert so[k] == se[k], (k, so[k], se[k])
    incl = np.concatenate(shown)
    assert len(incl) > 2 * irs.COLS and (~np.isnan(incl)).mean() > 0.8   # (the kept table entry at work: tests/test_incl_record_cpu.py)
    e.close()


@pytest.mark.parametrize("rows", ROWS)
def test_four_streams_through_the_device_entry(rows, oracle_lib):
    """Events off, batches overlapping on the engine's chains: two stale streams, the roll-back stream and the NaN-range stream side by
    side, 65 calls of two rotations each; after every 13th call every stream is in the oracle's state with the oracle's columns in the
    retained part of the ring."""
    import torch
    from continuous_clustering_amd import Engine
    recs = [_record("stale", rows, True), _record("rollback", rows, True), _record("nan_range", rows, True), _record("stale", rows, True)]
    streams = [r[0] for r in recs]
    cfg = recs[0][1]
    S, F, NB = len(streams), 2 * irs.COLS, 5 * irs.PASSES
    e = Engine(cfg, rows, S)
    e.record_events(False)
    xyz = torch.from_numpy(np.stack([st.xyz[:NB * F].reshape(NB, F, rows, 3) for st in streams], axis=1)).cuda()
    inten = torch.from_numpy(np.stack([st.intensity[:NB * F].reshape(NB, F, rows) for st in streams], axis=1)).cuda()
    poses = torch.from_numpy(np.stack([st.poses[:NB * F].reshape(NB, F, 12) for st in streams], axis=1)).cuda()
    torch.cuda.synchronize()
    from oracle.pyoracle import Oracle
    oracles = [Oracle(cfg, rows) for _ in range(3)] + [None]   # (stream 3 is stream 0 again)
    fed = 0
    for b in range(NB):
        e.add_firings_device(F, xyz[b], inten[b], poses[b])
        if (b + 1) % 13 and b + 1 < NB:
            continue
        # every 13 calls (and at the end), in even and in odd passes of the stale row
        assert e.sync() == 0, e.last_error()
        upto = (b + 1) * F
        for s, st in enumerate(streams):
            if oracles[s] is not None:
                assert oracles[s].add_firings(st.xyz[fed:upto], st.intensity[fed:upto], st.poses[fed:upto]) == 0
            o = oracles[s] or oracles[0]
            so, se = o.state(), e.state(s)
            for k in util.STATE_FIELDS:
                assert so[k] == se[k], (b, s, k, so[k], se[k])
            lo, hi = se["ring_buffer_start_global_column_index"], se["first_unpublished_global_column_index"] - 1
            assert hi > lo + irs.COLS // 2   # (about one rotation is retained, cc.cpp:1077-1091)
            util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo, mirror=False)
        fed = upto
    assert e.state(0)["ring_buffer_start_global_column_index"] > 12 * irs.RING
    e.close()
