"""Streams that run past 2^15 passes over the ring: nine hours of a 10 Hz sensor. Pure numpy; a stream is kept as one period and a repeat count
and is never materialised whole.

The engine keeps per cell which pass over the ring filled it in 15 bits (csrc/cc_k_base.h: cell_tag); the tag goes from 0xFFFF back to 0x8000
after 32 768 passes, whatever num_columns is. A pass is 10 * num_columns firings, so the smallest stream that reaches the wrap has the smallest
num_columns at which clusters still form: a return is ignored below max_distance (cc.cpp:567-616) and has to lie within max_distance of its
neighbour in the next column, 2 r sin(pi / num_columns) < max_distance <= r, hence num_columns > 6. 8 columns, 4 rows.

One period is one pass: synth.make_stream(80) of the static default scene; in 70 % of the firings (default_rng(wall_seed)) every ray is rescaled
to range 1.0 m — a shell around the sensor whose neighbouring columns are 0.77 m apart, inside max_distance = 0.9; the other firings keep the
scene and cut the shell into clusters. The ego box is switched off (it would swallow the shell). After 32 768 passes cluster ids are above
200 000 and continuous azimuths above 2 * 10^6 rad (tests/test_longrun_cases_cpu.py holds the streams to that).

What the GPU tests need of the oracle is bounded (LongrunRecord): outside a window of passes around the wrap per 4000-firing call the number of
events, their CRC and the state; inside the window all events and every column as it was published."""
from __future__ import annotations

import zlib

import numpy as np

from continuous_clustering_amd import capi, synth

ROWS, COLS = 4, 8
PASS = 10 * COLS                      # firings of one pass over the ring = one period of the stream
WRAP = 1 << 15                        # passes after which cell_tag repeats
CALL = 4000                           # firings of an ordinary call: 50 passes
N_PASSES = 32850                      # 657 calls: 82 passes beyond the wrap
WIN_FROM, WIN_TO = 32760, 32777       # the window: passes 32 760 .. 32 776, 1360 firings
assert CALL % PASS == 0 and (N_PASSES * PASS) % CALL == 0 and WIN_FROM < WRAP < WIN_TO
# calls of CALL firings reach to PREFIX; then the window's start is reached in one shorter call; the window; one call up to the next multiple of
# CALL; calls of CALL firings to the end
PREFIX = (WIN_FROM * PASS) // CALL * CALL
SUFFIX = -(-(WIN_TO * PASS) // CALL) * CALL
WINDOW_CHUNKS = (1, 3, 2, 17, 40, 97)
WALL_SEEDS = (4, 11)                  # the two streams of the multi-stream variants


def sensor():
    return synth.SensorModel(num_rows=ROWS, num_columns=COLS, incl_top_deg=20.0, incl_bottom_deg=-20.0)


def config():
    cfg = capi.Config.kitti()
    cfg.num_columns = COLS
    cfg.max_distance = 0.9
    cfg.length_ref_to_front_end_ = cfg.length_ref_to_rear_end_ = 0.0
    cfg.width_ref_to_left_mirror_ = cfg.width_ref_to_right_mirror_ = 0.0
    return cfg


def overrun_config():
    """nothing is published or cleared any more (cc.cpp:841-842): the next pass runs into its own tail"""
    cfg = config()
    cfg.cluster_point_trees_every_nth_column = 100000
    return cfg


def period(wall_seed=WALL_SEEDS[0]):
    """one pass (80 firings) as a synth.Stream"""
    st = synth.make_stream(PASS, seed=1, sensor=sensor(), motion=synth.Motion.static())
    wall = np.random.default_rng(wall_seed).random(PASS) < 0.7
    xyz = st.xyz.astype(np.float64)
    rng_ = np.sqrt((xyz * xyz).sum(-1, keepdims=True))
    xyz[wall] = xyz[wall] / rng_[wall] * 1.0
    return synth.Stream(xyz=xyz.astype(np.float32), intensity=st.intensity, poses=st.poses, sensor=st.sensor, hit=st.hit)


def nan_period():
    """a stream without a single return: it never starts"""
    st = period()
    return synth.Stream(xyz=np.full_like(st.xyz, np.nan), intensity=st.intensity, poses=st.poses, sensor=st.sensor)


class Periodic:
    """`per` repeated for ever; firings(f0, n): the arrays of firings f0 .. f0 + n - 1 (n <= CALL; cut from one tiled buffer)"""

    def __init__(self, per):
        self.per, self.sensor = per, per.sensor
        k = CALL // PASS + 2
        self._xyz, self._inten, self._poses = np.tile(per.xyz, (k, 1, 1)), np.tile(per.intensity, (k, 1)), np.tile(per.poses, (k, 1))

    def firings(self, f0, n):
        assert 0 < n <= CALL
        a = f0 % PASS
        return self._xyz[a:a + n], self._inten[a:a + n], self._poses[a:a + n]


def call_plan(window_chunks=WINDOW_CHUNKS, n_passes=N_PASSES):
    """[(first firing, firings, in the window?)] of a whole run: CALL firings per call outside the window, `window_chunks` in turn inside"""
    plan, f = [], 0
    w0, w1, end = WIN_FROM * PASS, WIN_TO * PASS, n_passes * PASS
    while f < w0:
        n = min(CALL, w0 - f)
        plan.append((f, n, False))
        f += n
    i = 0
    while f < w1:
        n = min(window_chunks[i % len(window_chunks)], w1 - f)
        plan.append((f, n, True))
        f, i = f + n, i + 1
    while f < end:
        n = min(CALL - f % CALL, end - f)
        plan.append((f, n, False))
        f += n
    return plan


class LongrunRecord:
    """The oracle's run of one stream, bounded. calls: {(first firing, firings): (events, crc32 of the event bytes, state)} of the calls outside
    the window; events: the window's events, one array; state_at: {firing count: state} after every rotation inside the window (and at its
    ends); columns: every column published inside the window, as published (columns col_lo .. col_hi, [n, ROWS] per field)."""

    def __init__(self, wall_seed, n_passes=N_PASSES):
        from oracle.pyoracle import Oracle
        import util
        self.stream = Periodic(period(wall_seed))
        self.cfg = config()
        o = Oracle(self.cfg, ROWS)
        o.keep_published_tail(4 * PASS)                                   # (the snapshots of 2.6 million columns would be a gigabyte)
        self.calls, self.state_at, self.rc = {}, {}, 0
        events, cols = [], []
        self.col_lo = None
        nxt = None
        for f, n, inside in call_plan((COLS,), n_passes):
            self.rc = o.add_firings(*self.stream.firings(f, n))
            assert self.rc == 0, (f, o.last_error())
            ev = o.drain_events()
            st = o.state()
            if not inside:
                self.calls[(f, n)] = (len(ev), zlib.crc32(ev.tobytes()), {k: st[k] for k in util.STATE_FIELDS})
                if f + n == WIN_FROM * PASS:
                    self.state_at[f + n] = st
                    nxt = st["first_unpublished_global_column_index"]
                    self.col_lo = nxt
                continue
            events.append(ev)
            self.state_at[f + n] = st
            hi = st["first_unpublished_global_column_index"] - 1
            if hi >= nxt:
                cols.append(o.read_published(nxt, hi))
                nxt = hi + 1
        self.col_hi = nxt - 1
        self.events = np.concatenate(events)
        self.columns = {k: np.concatenate([c[k] for c in cols]) for k in cols[0]}
        self.final_state = o.state()
        self.oracle = o

    def columns_of(self, c0, c1):
        assert self.col_lo <= c0 <= c1 <= self.col_hi, (c0, c1, self.col_lo, self.col_hi)
        return {k: v[c0 - self.col_lo:c1 - self.col_lo + 1] for k, v in self.columns.items()}


class OverrunRecord:
    """The oracle under the overrun schedule: config() for `switch_pass` passes, overrun_config() from then on, until it refuses a column.
    rc, error (the reference's text), stale / col / ring (the three numbers of the text), firings (fed when it stopped), state."""

    def __init__(self, wall_seed=WALL_SEEDS[0], switch_pass=WRAP, passes_behind=12):
        import re
        from oracle.pyoracle import Oracle
        self.stream = Periodic(period(wall_seed))
        self.switch = switch_pass * PASS
        o = Oracle(config(), ROWS)
        o.keep_published_tail(4 * PASS)
        f = 0
        while f < self.switch:
            n = min(CALL, self.switch - f)
            assert o.add_firings(*self.stream.firings(f, n)) == 0, (f, o.last_error())
            o.drain_events()
            f += n
        self.state_at_switch = o.state()
        o.set_config(overrun_config())
        self.reset_required_after_switch = o.state()["reset_required"]
        self.rc = 0
        while self.rc == 0 and f < self.switch + passes_behind * PASS:
            self.rc = o.add_firings(*self.stream.firings(f, 1))
            f += 1
        self.firings, self.error, self.state = f, o.last_error(), o.state()
        m = re.search(r": (-?\d+), (-?\d+), (\d+)", self.error)
        self.stale, self.col, self.ring = (int(v) for v in m.groups()) if m else (None, None, None)


_records = {}


def record(wall_seed):
    """one oracle run per stream and process"""
    if wall_seed not in _records:
        _records[wall_seed] = LongrunRecord(wall_seed)
    return _records[wall_seed]


def overrun_record():
    if "overrun" not in _records:
        _records["overrun"] = OverrunRecord()
    return _records["overrun"]
