"""GPU: the engine's grow-only scratch and pinned blocks over their whole life (csrc/cc_buffers.h) — prewarmed, grown past the prewarmed size,
dropped by a reset into another shape and built again — with every result along the way compared with the oracle.

One stream, 16 then 32 rows, 600 columns. The small calls (1, 8 and 40 firings: a captured graph, the largest captured graph, one direct launch)
go through the pinned staging and the per-slot ego records; read_columns over more than 512 columns grows the view scratch (device and pinned
halves) past what "prewarm_small_graphs" sized; gather_cluster_points uses the gather scratch; cc_engine_reset(32) frees every block tied to
the shape (free_all) and the calls behind it allocate them again."""
import functools

import numpy as np
import pytest

import util
from continuous_clustering_amd import capi, synth

COLUMNS = 600
FIRINGS = 2 * COLUMNS + 200
CALL_SIZES = (1, 8, 40)


@functools.lru_cache(maxsize=None)
def _case(rows):
    """(config, stream, oracle, the oracle's events) of the scene at `rows` rows: computed once, read-only afterwards."""
    cfg = capi.Config.kitti()
    cfg.num_columns = COLUMNS
    sensor = synth.SensorModel(num_rows=rows, num_columns=COLUMNS)
    stream = synth.make_stream(FIRINGS, seed=4100 + rows, sensor=sensor, motion=synth.Motion.translate())
    oracle, rc = util.run_oracle(stream, cfg)
    assert rc == 0, oracle.last_error()
    return cfg, stream, oracle, oracle.drain_events()


@pytest.mark.parametrize("rows", [16, 32])
def test_the_scene_finishes_clusters_and_publishes_more_than_the_prewarmed_view(rows, oracle_lib):
    """CPU, oracle alone: what the GPU test below gathers and reads is not vacuous at this size."""
    _, _, oracle, events = _case(rows)
    clusters = events[events["type"] == capi.EV_CLUSTER]
    assert len(clusters) >= 3 and int(clusters["d"].max()) > 5
    st = oracle.state()
    assert st["first_unpublished_global_column_index"] - max(st["ring_buffer_start_global_column_index"], 0) > 512


def _small_calls_and_queries(e, rows, reads, same_object=None):
    """Feed the scene in small calls; compare events, published columns and gathered clusters with the oracle; then one read of everything
    that is published. `reads`: read_columns calls made on this engine so far (view_counters counts every one, on one side or the other).
    `same_object`: (oracle, events) of an oracle object that went through the engine's history and then ran this scene, instead of a fresh one."""
    cfg, stream, oracle, eo = _case(rows)
    if same_object is not None:
        oracle, eo = same_object
    oracle_clusters = {int(ev["c"]): int(ev["d"]) for ev in eo[eo["type"] == capi.EV_CLUSTER]}

    def healthy():
        vc = e.view_counters()
        assert e.last_error() == "" and vc["mirror"] + vc["kernel"] == reads, (e.last_error(), vc, reads)

    f = i = ev_pos = 0
    gathered = {}
    while f < FIRINGS:
        m = min(CALL_SIZES[i % len(CALL_SIZES)], FIRINGS - f)
        assert e.add_firings(stream.xyz[f:f + m], stream.intensity[f:f + m], stream.poses[f:f + m]) == 0, e.last_error()
        f += m
        i += 1
        ee = e.drain_events()
        ref = eo[ev_pos:ev_pos + len(ee)]
        assert len(ref) == len(ee)
        for fld in ("type", "a", "b", "c", "d", "column"):
            assert np.array_equal(ref[fld], ee[fld]), (f, fld)
        ev_pos += len(ee)
        pub = ee[(ee["type"] == capi.EV_PUBLISH_COLUMNS) & (ee["b"] >= ee["a"])]
        if len(pub):
            lo, hi = int(pub["a"].min()), int(pub["b"].max())
            util.compare_columns(oracle.read_published(lo, hi), e.read_columns(lo, hi), lo)
            reads += 1
        cl = ee[ee["type"] == capi.EV_CLUSTER]
        if len(cl):
            offsets, gcol, row = e.gather_cluster_points(cl)
            for k, c in enumerate(cl):
                g, r = gcol[offsets[k]:offsets[k + 1]], row[offsets[k]:offsets[k + 1]]
                assert len(g) == c["d"] == oracle_clusters[int(c["c"])]
                assert (g >= c["a"]).all() and (g <= c["b"]).all() and (r >= 0).all() and (r < rows).all()
                assert (np.diff(g * rows + r) > 0).all(), "points must come sorted by (column, row), without duplicates"
                gathered[int(c["c"])] = g * rows + r
        healthy()
    assert ev_pos == len(eo) and len(gathered) == len(oracle_clusters) >= 3
    so, se = oracle.state(), e.state()
    for k in util.STATE_FIELDS:
        assert so[k] == se[k], k
    # everything that is published, in one read: more columns than the prewarmed 512, so the view scratch grows here
    lo, hi = max(se["ring_buffer_start_global_column_index"], 0), se["first_unpublished_global_column_index"] - 1
    assert hi - lo + 1 > 512
    before = e.view_counters()["kernel"]
    cols = e.read_columns(lo, hi)
    reads += 1
    assert e.view_counters()["kernel"] == before + 1
    util.compare_columns(oracle.read_published(lo, hi), cols, lo)
    # the published cells that carry a cluster's id are gathered members of that cluster (clusters of at most 5 points keep id 0, cc.cpp:936)
    ids, checked = cols["id"].reshape(hi - lo + 1, rows), 0
    for cid, key in gathered.items():
        inside = key[(key // rows >= lo) & (key // rows <= hi)]
        if len(key) > 5 and len(inside):
            assert (ids[inside // rows - lo, inside % rows] == cid).all()
            published = np.argwhere(ids == cid)
            assert np.isin((published[:, 0] + lo) * rows + published[:, 1], key).all()
            checked += 1
    assert checked >= 1
    healthy()
    return reads


@pytest.mark.gpu
def test_prewarm_small_calls_growth_and_reshape(oracle_lib):
    from continuous_clustering_amd import Engine, IDENTITY_TF
    cfg = _case(16)[0]
    e = Engine(cfg, 16, 1, 0, IDENTITY_TF)
    assert e.last_error() == ""
    e.set_option("prewarm_small_graphs", 8)
    assert e.last_error() == "" and e.view_counters() == {"mirror": 0, "kernel": 0}
    reads = _small_calls_and_queries(e, 16, 0)
    e.reset(32)  # another shape: free_all, then allocate
    e.set_robot_from_sensor(IDENTITY_TF)
    assert e.last_error() == "" and e.state()["num_rows"] == 32
    # the yardstick of the second scene is an oracle object with the same history: reset(32) keeps the 16 rows of the inclination table that both
    # shapes have (cc.cpp:46)
    first, second = _case(16)[1], _case(32)[1]
    same, rc = util.run_oracle(first, cfg)
    assert rc == 0
    same.reset(32)
    same.set_robot_from_sensor(IDENTITY_TF)
    assert same.add_firings(second.xyz, second.intensity, second.poses) == 0, same.last_error()
    _small_calls_and_queries(e, 32, reads, (same, same.drain_events()))
    e.close()
