"""CPU: the streams of longrun_streams.py held to their purpose on the oracle alone. tests/test_gpu_longrun_parity.py puts the engine against
these records across the wrap of its 15-bit pass tag (csrc/cc_k_base.h: cell_tag); what is asserted here keeps that comparison from passing
vacuously: the streams run cleanly past pass 32 800, cluster ids have left 16 bits behind and continuous azimuths are beyond 2 * 10^6 rad before
the window, every pass of the window finishes clusters and publishes ids, the ring holds returns of both passes when the tag wraps, and the
overrun schedule makes the reference refuse a column of pass 32 768 (tag 0x8000) because of a stale cell of pass 32 767 (tag 0xFFFF).

The second restatement (test_oracle_independent.py) is not put against the oracle here: it is fed firing by firing in Python from column 0 and
keeps every column it has seen, 2.6 million firings of it take far longer than a minute."""
import numpy as np
import pytest

import longrun_streams as ls
from continuous_clustering_amd import capi

WINDOW_PASSES = range(ls.WIN_FROM, ls.WIN_TO)


@pytest.mark.parametrize("wall_seed", ls.WALL_SEEDS)
def test_stream_runs_past_the_wrap(wall_seed, oracle_lib):
    """Measured (wall seed 4 / 11): 229 950 / 361 350 clusters at the end, 229 320 / 360 360 before the window; about 2840 / 2910 events in
    the window; 10 s of oracle time each."""
    r = ls.record(wall_seed)
    fs = r.final_state
    assert r.rc == 0 and fs["reset_required"] == 0 and fs["error"] == 0
    assert fs["firings_consumed"] == ls.N_PASSES * ls.PASS and fs["first_unpublished_global_column_index"] > 32800 * ls.PASS
    before = r.state_at[ls.WIN_FROM * ls.PASS]
    print(wall_seed, "clusters before the window", before["clusters_finished"], "at the end", fs["clusters_finished"], "window events", len(r.events))
    assert before["clusters_finished"] > 65536 and before["cluster_counter"] > 65536
    # every call of the record is there: 4000-firing calls, the two shorter ones next to the window
    assert sum(n for (_, n) in r.calls) + (ls.WIN_TO - ls.WIN_FROM) * ls.PASS == ls.N_PASSES * ls.PASS
    assert all(c[0] > 0 for c in r.calls.values())


@pytest.mark.parametrize("wall_seed", ls.WALL_SEEDS)
def test_every_pass_of_the_window_clusters_and_publishes(wall_seed, oracle_lib):
    r = ls.record(wall_seed)
    ev = r.events
    cl = ev[ev["type"] == capi.EV_CLUSTER]
    assert (cl["c"] > 65536).all()
    ids = r.columns["id"]
    gcol = np.arange(r.col_lo, r.col_hi + 1)
    assert r.col_lo <= ls.WIN_FROM * ls.PASS + ls.PASS and r.col_hi >= (ls.WIN_TO - 1) * ls.PASS
    for p in WINDOW_PASSES:
        assert ((cl["column"] // ls.PASS) == p).any(), f"no cluster finished while pass {p} was inserted"
        inside = (gcol // ls.PASS) == p
        if p > ls.WIN_FROM and p < ls.WIN_TO - 1:
            assert inside.sum() == ls.PASS
        assert (ids[inside] > 65536).any(), f"no id published in pass {p}"
    assert (ids[ids != 0] > 65536).all() and ids.max() < 2 ** 32
    # the azimuths the engine carries as a double base plus a float fraction
    caz = r.columns["continuous_azimuth_angle"]
    assert np.nanmin(caz) > 2.0e6
    fin = r.columns["finished_at_continuous_azimuth_angle"]
    assert np.nanmax(fin) > 2.0e6


@pytest.mark.parametrize("wall_seed", ls.WALL_SEEDS)
def test_both_passes_hold_returns_at_the_wrap(wall_seed, oracle_lib):
    """cells of pass 32 767 (tag 0xFFFF) and of pass 32 768 (tag 0x8000) are published with a return; and after the first rotation of pass
    32 768 the ring still holds columns of pass 32 767 (the two tags lie side by side)"""
    r = ls.record(wall_seed)
    gcol = np.arange(r.col_lo, r.col_hi + 1)
    has = ~np.isnan(r.columns["distance"])
    for p in (ls.WRAP - 1, ls.WRAP):
        n = int(has[(gcol // ls.PASS) == p].sum())
        assert n > ls.PASS, (p, n)
        assert (r.columns["global_column_index"][(gcol // ls.PASS) == p][has[(gcol // ls.PASS) == p]] // ls.PASS == p).all()
    at_wrap = r.state_at[ls.WRAP * ls.PASS + ls.COLS]
    assert at_wrap["ring_buffer_start_global_column_index"] < ls.WRAP * ls.PASS <= at_wrap["ring_buffer_end_global_column_index"]


def test_overrun_schedule_stops_at_the_wrap(oracle_lib):
    """Measured: 'not cleared ...: 2621425, 2621505, 80', 77 firings behind the switch."""
    r = ls.overrun_record()
    assert r.reset_required_after_switch == 0
    assert r.rc == capi.CC_ERR_RING_OVERRUN, (r.rc, r.error)
    assert "not cleared" in r.error and r.ring == ls.PASS
    assert r.col // ls.PASS == ls.WRAP and r.stale // ls.PASS == ls.WRAP - 1 and r.stale == r.col - ls.PASS
    assert r.firings - r.switch < 2 * ls.PASS
    # up to the switch the schedule is the plain stream
    plain = ls.record(ls.WALL_SEEDS[0])
    assert {k: r.state_at_switch[k] for k in plain.state_at[r.switch]} == plain.state_at[r.switch]
