"""GPU: parity past 2^15 passes over the ring — nine hours of a 10 Hz sensor.

A cell carries the pass over the ring that filled it in 15 bits (csrc/cc_k_base.h: cell_tag, 0x8000 | pass mod 2^15), where the reference keeps
the 64-bit global column; after 32 768 passes the tag goes from 0xFFFF back to 0x8000. The streams of longrun_streams.py (8 columns, 4 rows, one
pass = 80 firings) cross that point after 2 621 440 firings with cluster ids above 200 000 and continuous azimuths above 2 * 10^6 rad. The oracle
runs each stream once (longrun_streams.record: per-call event counts, CRCs and states outside a window of 17 passes around the wrap, every event
and every published column inside); every engine run below is put against that record, bit for bit as everywhere else.

What runs where at this shape (read from csrc/cc_engine.hip and csrc/cc_launch.h, and asserted from the counters):
  host path    cc_engine_add_firings cuts a call into parts of 2 * num_columns = 16 firings, so the block-parallel insertion (>= 64 firings) never
               runs: k_prep + k_insert2, k_seg_small, the window scan, k_assocb with k_assoc3 behind it (a quarter of the batches bail out to it),
               publishing and the deferred clearing; in the window calls of 1 .. 63 firings are small calls (k_small_all as a captured graph up to
               8 firings, as a direct launch above), the call of 97 firings takes the general path.
  device path  cc_engine_add_firings_device, events off: k_insert_par with its fused segmentation front (debug counter 6: firings it took,
               7: batches it saw; it takes the first firings of a call, k_insert2 the rest in continuation passes of 16 columns), k_seg_scan, k_scan2, k_assocb / k_assoc3, k_take_* and k_tc_*.
k_insert_multi (parallel_insert = 1 on sensors above 64 rows) is not brought to the wrap: it wants firings that span many columns.

Every run is 2.6 million firings in passes of 16 columns (limit_columns = 2 * num_columns), 0.15 - 0.22 ms each: 25 - 38 s per test on an MI355X
(each docstring has its figure), and 10 s per stream for the oracle's record on the host. 32 768 passes are the point; the runs are not shortened,
there are three of them instead."""
import time

import numpy as np
import pytest

import longrun_streams as ls
import test_gpu_take as tk
import test_gpu_take_clusters as tkc
import util
from continuous_clustering_amd import capi, take
from test_gpu_segmentation_sweep import debug_counters

pytestmark = pytest.mark.gpu

W0, W1 = ls.WIN_FROM * ls.PASS, ls.WIN_TO * ls.PASS
END = ls.N_PASSES * ls.PASS


def _assert_state(ref, got, where):
    for k in util.STATE_FIELDS:
        assert ref[k] == got[k], f"{where}: state.{k}: oracle {ref[k]} engine {got[k]}"


def _compare_window_columns(rec, e, lo, hi, stream=0, mirror=True):
    """columns lo .. hi of the engine against the record, in pieces the ring can hold"""
    n = 0
    for c0 in range(lo, hi + 1, ls.PASS - 1):
        c1 = min(hi, c0 + ls.PASS - 2)
        util.compare_columns(rec.columns_of(c0, c1), e.read_columns(c0, c1, stream=stream), c0, mirror=mirror)
        n += c1 - c0 + 1
    return n


# ---- a: the host path ---------------------------------------------------------------------------------------------------------------------------
def test_host_path_across_the_tag_wrap(oracle_lib):
    """The default engine (events and mirror fields on): 4000-firing calls before and behind the window — after each the number of events, their
    CRC and the state are the record's —, calls of 1, 3, 2, 17, 40, 97 firings in turn through the window — every event field, every column a call
    published that the ring still holds when the call returns (a call of more than 16 firings is cut into parts, and the later parts clear what
    the earlier ones published, cc_hip.h), raw ids, the state at the end of the window and of the run.
    Measured: 36 s on the MI355X (657 calls of 4000 firings = 164 000 parts of 16 firings, 0.22 ms each), 10 s for the oracle; 306 window columns
    compared, 46 small calls."""
    import zlib
    from continuous_clustering_amd import Engine
    rec = ls.record(ls.WALL_SEEDS[0])
    st = rec.stream
    e = Engine(rec.cfg, ls.ROWS)
    t0 = time.time()
    ev_pos = n_cols = small = 0
    pubs = set()
    dbg0 = None
    for f, n, inside in ls.call_plan():
        if f == W0:
            dbg0 = debug_counters(e)
        rc = e.add_firings(*st.firings(f, n))
        where = f"call of firings {f} .. {f + n - 1}"
        assert rc == 0, (where, e.last_error())
        ee = e.drain_events()
        if not inside:
            cnt, crc, state = rec.calls[(f, n)]
            assert len(ee) == cnt, (where, len(ee), cnt)
            assert zlib.crc32(ee.tobytes()) == crc, where
            _assert_state(state, e.state(), where)
            continue
        small += n < 64
        try:
            ev_pos, pub = util.compare_events(rec.events, ee, ev_pos)
            if pub is not None:
                lo = max(pub[0], e.state()["ring_buffer_start_global_column_index"])
                n_cols += _compare_window_columns(rec, e, lo, pub[1])
                pubs.update(range(lo, pub[1] + 1))
        except AssertionError as ex:
            raise AssertionError(where + ": " + str(ex)) from None
        if f + n == W1:
            assert ev_pos == len(rec.events), (ev_pos, len(rec.events))
            _assert_state(rec.state_at[W1], e.state(), "end of the window")
    _assert_state(rec.final_state, e.state(), "end of the run")
    dbg1 = debug_counters(e)
    print("host path:", round(time.time() - t0, 1), "s; window columns compared", n_cols, "small calls", small, "debug counters", list(dbg1), e.batch_counters())
    # columns of both passes at the wrap were compared, and ids beyond 16 bits among them
    for p in (ls.WRAP - 1, ls.WRAP):
        assert sum(1 for c in pubs if c // ls.PASS == p) >= ls.COLS, p
    assert n_cols >= 200 and small > 40                     # (a call compares at least min(what it published, one rotation) columns)
    # no call of the host path reaches the block-parallel insertion at 8 columns: the serial insertion and the small-call kernels crossed the wrap
    assert dbg1[6] == 0 and dbg1[7] == 0 and dbg0[6] == 0
    assert e.batch_counters()["batch_columns"] > 0          # k_assocb took columns (and bailed out to k_assoc3 for others)
    e.close()


# ---- b: the pipelined device path --------------------------------------------------------------------------------------------------------------
def _device_buffers(torch, periods, n):
    """[S][n] firings from phase 0 of every stream (n is a multiple of the period wherever it is used)"""
    assert n % ls.PASS == 0
    parts = [p.firings(0, n) for p in periods]
    out = [torch.from_numpy(np.ascontiguousarray(np.stack([q[k] for q in parts]))).cuda() for k in range(3)]
    torch.cuda.synchronize()
    return out


def _device_run(options):
    import torch
    from continuous_clustering_amd import Engine
    recs = [ls.record(seed) for seed in ls.WALL_SEEDS]
    periods = [r.stream for r in recs] + [ls.Periodic(ls.nan_period())]
    S = len(periods)
    cfg = recs[0].cfg
    e = Engine(cfg, ls.ROWS, S)
    e.record_events(False)
    for k, v in options.items():
        e.set_option(k, v)
    assert W0 % ls.PASS == 0 and ls.PREFIX % ls.PASS == 0 and ls.SUFFIX % ls.PASS == 0
    buf = {n: _device_buffers(torch, periods, n) for n in {ls.CALL, W0 - ls.PREFIX, ls.PASS, ls.SUFFIX - W1}}
    t0 = time.time()

    def feed(n):
        e.add_firings_device(n, *buf[n])

    def check_states(f, where):
        assert e.sync() == 0, (where, e.last_error())
        for s, r in enumerate(recs):
            ref = r.state_at[f] if f in r.state_at else (r.final_state if f == END else r.calls[(f - ls.CALL, ls.CALL)][2])
            _assert_state(ref, e.state(s), f"{where}, stream {s}")
        idle = e.state(S - 1)
        assert idle["firings_consumed"] == f and idle["first_unpublished_global_column_index"] < 0 and idle["cells_published"] == 0, idle

    f = 0
    while f < ls.PREFIX:
        feed(ls.CALL)
        f += ls.CALL
    check_states(f, "end of the prefix")
    feed(W0 - f)
    f = W0
    check_states(f, "start of the window")
    # what was published and finished before the window is taken and dropped: the cursors stand at the window's first column
    e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS)
    e.take_clusters(6)
    dbg0 = debug_counters(e)
    clog = tkc.ClusterLog(S, 6)
    clog.next_id = [int(e.take_clusters_cursor(s)[0]) for s in range(S)]
    col_to = [e.state(s)["first_unpublished_global_column_index"] for s in range(S)]
    n_cols = n_rec = 0
    at_wrap = None
    while f < W1:
        before = debug_counters(e) if f == ls.WRAP * ls.PASS else None
        feed(ls.PASS)
        f += ls.PASS
        where = f"window call ending at firing {f}"
        check_states(f, where)
        if before is not None:
            at_wrap = [int(b - a) for a, b in zip(before, debug_counters(e))]
        records, table = e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS)
        got_all = tk._host(records)
        for s, r in enumerate(recs):
            se = e.state(s)
            lo, hi = se["ring_buffer_start_global_column_index"], se["first_unpublished_global_column_index"] - 1
            n_cols += _compare_window_columns(r, e, lo, hi, stream=s, mirror=False)
            # the hand-over of the published points: a call of 80 firings runs in passes of 16 columns, whose clearing overtakes the cursor —
            # the columns that are gone are counted, the others are the oracle's, return for return
            t = table[s]
            assert t["error"] == 0 and t["col_to"] == hi + 1 and t["col_from"] - t["lost_columns"] == col_to[s], (where, s, t, col_to[s])
            assert 0 < t["col_to"] - t["col_from"] and t["lost_columns"] < ls.PASS, (where, s, t)
            col_to[s] = int(t["col_to"])
            got = got_all[int(t["first_record"]):int(t["first_record"] + t["n_records"])]
            ref, ref_gcol = tk._reference_records(r.columns_of(int(t["col_from"]), hi), int(t["col_from"]))
            tk._assert_records_equal(got, got["column"].astype(np.int64) + int(t["col_from"]), ref, ref_gcol, what=(where, s))
            assert np.array_equal(got["intensity"], r.stream.per.intensity[got["source_firing"].astype(np.int64) % ls.PASS, got["row"]]), (where, s)
            n_rec += len(got)
        assert table[S - 1]["n_records"] == 0
        clog.add(*e.take_clusters(6), counters=[e.state(s)["cluster_counter"] for s in range(S)], lost_ok=True)
    dbg1 = debug_counters(e)
    # the clusters handed over in the window against the oracle's cluster events and published cells
    matched = 0
    for s, r in enumerate(recs):
        ev = r.events[r.events["type"] == capi.EV_CLUSTER]
        by_id = {int(x["c"]): x for x in ev}
        cells = tkc._by_id(*tk._reference_records(r.columns, r.col_lo))
        d = clog.descriptors(s)
        assert len(d) > 0 and (d["id"] > 65536).all()
        for i in range(len(d)):
            x = by_id.get(int(d[i]["id"]))
            if x is None:
                assert int(d[i]["id"]) < int(ev["c"].min()), (s, d[i])     # finished before the window
                continue
            last = int(d[i]["col_from"]) + int(d[i]["n_columns"]) - 1
            assert last == x["b"] and d[i]["col_from"] >= x["a"], (s, d[i], x)
            if d[i]["col_from"] != x["a"] or d[i]["n_points"] != x["d"]:
                continue                                                   # (its first columns were cleared before the take: handed over in part)
            matched += 1
            if d[i]["col_from"] >= r.col_lo and last <= r.col_hi:
                ref, ref_gcol = cells[int(d[i]["id"])]
                got = clog.rec[s][i]
                tkc._assert_records_equal(got, got["column"].astype(np.int64) + int(d[i]["col_from"]), ref, ref_gcol, None, (s, int(d[i]["id"])))
    assert len(clog.desc[S - 1]) == 0
    feed(ls.SUFFIX - W1)
    f = ls.SUFFIX
    while f < END:
        feed(ls.CALL)
        f += ls.CALL
    check_states(f, "end of the run")
    took = int(dbg1[6] - dbg0[6])
    print("debug counters of the call that begins pass 32 768:", at_wrap)
    print("device path", options, round(time.time() - t0, 1), "s; window columns compared", n_cols, "records", n_rec, "whole clusters", matched,
          "debug counters in the window", [int(b - a) for a, b in zip(dbg0, dbg1)], e.batch_counters())
    assert n_cols >= 2 * (ls.WIN_TO - ls.WIN_FROM) * ls.COLS and n_rec > 500 and matched >= ls.WIN_TO - ls.WIN_FROM
    if options.get("parallel_insert", 1) != 0:
        # the block-parallel insertion sees every window call and takes its first firings (at this shape about three of a call: the rest goes
        # to k_insert2 in the continuation passes); the call that begins with the first firing of pass 32 768 is one of them: k_insert_par
        # wrote the first cells tagged 0x8000 beside pass 32 767's, and its front checked the column left open against the wrapped tag
        assert took >= ls.WIN_TO - ls.WIN_FROM and at_wrap[6] > 0 and at_wrap[7] > 0, (took, at_wrap)
        assert e.batch_counters()["batch_columns"] > 0
    else:
        assert took == 0 and dbg1[7] == dbg0[7] and at_wrap[6] == 0 and e.batch_counters()["batch_columns"] == 0
    e.close()


def test_device_path_across_the_tag_wrap(oracle_lib):
    """add_firings_device with events off on three streams — the two of longrun_streams and one without a single return, which never starts —
    from one 4000-firing device buffer per stream (the streams are periodic); through the window calls of one pass. State against the record at
    the end of the prefix, after every window call and at the end; after every window call the columns the ring holds (mirror fields off),
    take_points (CLUSTERED) and take_clusters against the oracle's window columns and cluster events.
    Measured: 25 s on the MI355X (10 s more for the second stream's oracle record); 272 window columns, 1700 records and 102 whole clusters
    compared; k_insert_par took 102 of stream 0's window firings, 6 of them in the call that begins pass 32 768. The same run with parallel_insert = 0 and assoc_batch = 0 (k_prep / k_insert2, k_assoc3 alone) passed in 21 s
    when this test was written and is not kept: every run is 2.6 million firings, and the host path already crosses the wrap on k_insert2."""
    _device_run({})


def test_first_device_call_longer_than_the_ring(oracle_lib):
    """The call that starts a stream had no emission limit (k_insert2 took limit_base from first_unfinished, which is -1 until the first return):
    a first add_firings_device call of more than a ring of firings wrote pass after pass over columns nobody had segmented, and the stream
    stopped with "not cleared: -2621360, 0, 80" (a cell of pass 1 met at column 0). Five passes in one call on fresh streams."""
    import torch
    from continuous_clustering_amd import Engine
    from oracle.pyoracle import Oracle
    n = 5 * ls.PASS
    periods = [ls.Periodic(ls.period(seed)) for seed in ls.WALL_SEEDS]
    e = Engine(ls.config(), ls.ROWS, len(periods))
    e.record_events(False)
    buf = _device_buffers(torch, periods, n)
    e.add_firings_device(n, *buf)
    assert e.sync() == 0, e.last_error()
    for s, p in enumerate(periods):
        o = Oracle(ls.config(), ls.ROWS)
        assert o.add_firings(*p.firings(0, n)) == 0
        so, se = o.state(), e.state(s)
        _assert_state(so, se, f"stream {s}")
        lo, hi = se["ring_buffer_start_global_column_index"], se["first_unpublished_global_column_index"] - 1
        assert hi > 4 * ls.PASS
        util.compare_columns(o.read_published(lo, hi), e.read_columns(lo, hi, stream=s), lo, mirror=False)
    e.close()


# ---- d: the overrun at the wrap -------------------------------------------------------------------------------------------------------------------
def test_deliberate_ring_overrun_at_the_tag_wrap(oracle_lib):
    """cluster_point_trees_every_nth_column = 100000 from pass 32 768 on: nothing is published or cleared any more, insertion meets the cells of
    pass 32 767 (tag 0xFFFF) while it writes pass 32 768 (tag 0x8000), and segmentation must refuse column 2 621 505 because of the stale column
    2 621 425 — the engine rebuilds that number from the two tags. Prefix in 4000-firing host calls, 80-firing calls behind the switch.
    The message comes from the segmentation kernel's own check; the check in k_insert_par's fused front (cc_k_insert.h, "as in k_seg_pre") cannot
    produce it: that kernel takes no firing whose ring slot is not known to be cleared, so the column it finishes first is never a stale one.
    Measured: 35 s on the MI355X, 10 s for the oracle."""
    from continuous_clustering_amd import Engine
    r = ls.overrun_record()
    assert r.rc == capi.CC_ERR_RING_OVERRUN and r.col // ls.PASS == ls.WRAP and r.stale == r.col - ls.PASS, r.error
    st = r.stream
    e = Engine(ls.config(), ls.ROWS)
    t0 = time.time()
    f = 0
    while f < r.switch:
        n = min(ls.CALL, r.switch - f)
        assert e.add_firings(*st.firings(f, n)) == 0, (f, e.last_error())
        e.drain_events()
        f += n
    _assert_state(r.state_at_switch, e.state(), "at the switch")
    e.set_config(ls.overrun_config())
    assert e.state()["reset_required"] == 0
    rc = 0
    while rc == 0 and f < r.switch + 4 * ls.PASS:
        rc = e.add_firings(*st.firings(f, ls.PASS))
        f += ls.PASS
    print("overrun:", round(time.time() - t0, 1), "s;", e.last_error())
    assert rc == capi.CC_ERR_RING_OVERRUN, (rc, e.last_error())
    se = e.state()
    assert (se["error_a"], se["error_b"]) == (r.stale, r.col), (se, r.error)
    # the text: the C ABI words it differently ("stream 0: ...") and the drop-in class composes the reference's wording from the state
    # (csrc/continuous_clustering.cpp: check); what both carry of the reference's text are the three numbers behind the last colon
    tail = r.error.rsplit(": ", 1)[1]
    assert "not cleared" in e.last_error() and e.last_error().rsplit(": ", 1)[1] == tail, (e.last_error(), r.error)
    assert r.error == r.error.rsplit(": ", 1)[0] + f": {se['error_a']}, {se['error_b']}, {se['ring_buffer_max_columns']}"
    assert f - ls.PASS < r.firings <= f                      # in the call that holds the firing at which the oracle stopped
    e.close()
