"""GPU: the C++ drop-in class through the scripts of tests/dropin_scripts.py — resets, configuration and transform changes between two firings,
both threading modes, enough firings to wrap its mirror ring and to trim its firing log, and inputs that make it throw. tests/cpp/dropin_script.cpp
runs a script on one ContinuousClustering object and dumps what the callbacks and the public members show; the oracle object goes through the same
operations. Every comparison is exact (floats bitwise with the NaN pattern). Point::associated_trees is the one field the oracle keeps no record of
(it records the clusters, not the links between their trees): it is held to its structure — only roots have entries, sorted, every entry a root of
the same cluster that names this root in turn, and the roots of every published cluster connected through them."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import dropin_scripts as ds
import util
from continuous_clustering_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "cpp", "dropin_script")
RUNS = [(name, batch) for name, (_, batches) in ds.SCRIPTS.items() for batch in batches]
_stopped = []     # why no further harness process is started: one of them ended by a signal or ran into its time limit


def run_harness(tmp_path, ops):
    """One harness process at a time, under a time limit sized from the firing count; after a run that ended by signal or time limit none is started."""
    if _stopped:
        pytest.skip("not started: " + _stopped[0])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "continuous_clustering_amd", "csrc")], stdout=subprocess.DEVNULL)
    inp, outp = str(tmp_path / "script.bin"), str(tmp_path / "dump.bin")
    ds.write_script(inp, ops)
    limit = 60 + ds.n_firings(ops) // 100
    try:
        r = subprocess.run([HARNESS, inp, outp], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _stopped.append(f"an earlier harness run did not end within {limit} s")
        raise AssertionError(_stopped[0]) from None
    if r.returncode < 0:
        _stopped.append(f"an earlier harness run ended by signal {-r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return ds.parse_dump(outp, ops)


@functools.lru_cache(maxsize=None)
def _libm():
    libm = C.CDLL("libm.so.6")
    libm.atan2f.restype = C.c_float
    libm.atan2f.argtypes = [C.c_float, C.c_float]
    return libm


@functools.lru_cache(maxsize=None)
def expected_azimuth(name, k):
    """atan2f of the raw return behind every published cell with a source (cc.cpp:142), from the host's libm; NaN elsewhere."""
    seg = ds.script_record(name)[0][k]
    src = seg.published["source_firing"]
    out = np.full(src.shape, np.nan, dtype=np.float32)
    atan2f = _libm().atan2f
    rowidx = np.broadcast_to(np.arange(seg.rows), src.shape)
    has = src >= 0
    raw = seg.xyz[src[has], rowidx[has]]
    out[has] = np.array([atan2f(float(y), float(x)) for x, y in zip(raw[:, 0].tolist(), raw[:, 1].tolist())], dtype=np.float32)
    out.setflags(write=False)
    return out


def expected_order(ev):
    out = []
    for e in ev:
        if e["type"] == capi.EV_GROUND_COLUMN:
            out.append((1, int(e["a"]), int(e["a"])))
        elif e["type"] == capi.EV_CLUSTER and e["d"] > 20:       # cc.cpp:1023
            out.append((2, int(e["c"]), int(e["d"])))
        elif e["type"] == capi.EV_PUBLISH_COLUMNS:
            out.append((3, int(e["a"]), int(e["b"])))
    return out


def eq(name, got, ref):
    bad = np.argwhere(np.asarray(got) != np.asarray(ref))
    assert bad.size == 0, f"{name}: {len(bad)} differ, first at {tuple(bad[0])}: class {np.asarray(got)[tuple(bad[0])]} expected {np.asarray(ref)[tuple(bad[0])]}"


def check_metadata(what, cells, src, seg, k, rows):
    """Pass-through metadata of cells [columns, rows] with the oracle's source_firing: from the firing of THIS segment, or the cleared defaults."""
    has = src >= 0
    rowidx = np.broadcast_to(np.arange(rows), src.shape)
    s = src[has].astype(np.uint64)
    eq(what + " row_index", cells["row_index"], np.where(has, rowidx, -1))
    eq(what + " firing_index", cells["firing_index"], np.where(has, src, 0).astype(np.uint64))
    eq(what + " stamp", cells["stamp"], np.where(has, 1000000 + 45 * src, 0).astype(np.uint64))
    uidx = np.full(src.shape, 2 ** 64 - 1, dtype=np.uint64)
    uidx[has] = (np.uint64(k) << np.uint64(48)) | (s << np.uint64(16)) | rowidx[has].astype(np.uint64)
    eq(what + " globally_unique_point_index", cells["globally_unique_point_index"], uidx)
    inten = np.zeros(src.shape, dtype=np.uint8)
    inten[has] = seg.intensity[src[has], rowidx[has]]
    eq(what + " intensity", cells["intensity"], inten)


def check_published(name, k, seg, got, complete):
    rows, ring = seg.rows, 10 * seg.num_columns
    if not got.published or all(to < frm for frm, to, *_ in got.published):
        assert not complete or seg.published is None
        return
    lo, hi = seg.published_range
    cols = np.concatenate([np.arange(frm, to + 1) for frm, to, *_ in got.published])
    if complete:
        eq("published columns", cols, np.arange(lo, hi + 1))
    else:
        eq("published columns", cols, np.arange(lo, lo + len(cols)))
    n = len(cols)
    cells = np.concatenate([c for _, _, c, _, _ in got.published])
    ref = {f: a[:n] for f, a in seg.published.items()}
    for f in ("id", "ground_point_label", "debug_ground_point_label", "is_ignored", "global_column_index", "tree_num_points", "cluster_width",
              "number_of_visited_neighbors", "belongs_to_finished_cluster"):
        eq(f, cells[f], ref[f])
    eq("n_child_points", cells["n_child_points"], ref["number_of_child_points"])
    for j, f in enumerate("xyz"):
        util.assert_float_equal(f, cells["xyz"][..., j].copy(), ref[f])
    for f in ("distance", "inclination_angle", "continuous_azimuth_angle", "finished_at_continuous_azimuth_angle"):
        util.assert_float_equal(f, cells[f].copy(), ref[f])
    eq("local_column_index", cells["local_column_index"], np.broadcast_to((cols % ring)[:, None], cells.shape))
    rootc, rootr = ref["tree_root_global_column"], ref["tree_root_row"]
    has_root = rootc >= 0
    eq("tree_root_.column_index", cells["tree_root_column"], np.where(has_root, rootc % ring, -1))
    eq("tree_root_.row_index", cells["tree_root_row"], np.where(has_root, rootr, 0))
    eq("tree_id", cells["tree_id"], np.where(has_root, rootc * rows + rootr, 0).astype(np.uint64))
    src = ref["source_firing"]
    check_metadata("published", cells, src, seg, k, rows)
    util.assert_float_equal("azimuth_angle", cells["azimuth_angle"].copy(), expected_azimuth(name, k)[:n])

    # child_points: the cells whose tree_parent_* name the point, in column-then-row order (cc.cpp:663), as (row, local column). The last published
    # columns may hold points of trees that are still open, with children in columns that were never published: the oracle's record has their number
    # (number_of_child_points, above) but not the cells, so entries behind the last published column are only held to their place at the list's end.
    parc, parr = ref["tree_parent_global_column"], ref["tree_parent_row"]
    child = np.argwhere((parc >= lo) & (parc < lo + n))                     # in column-then-row order
    key = (parc[child[:, 0], child[:, 1]] - lo) * rows + parr[child[:, 0], child[:, 1]]
    order = np.argsort(key, kind="stable")
    children = np.concatenate([c for *_, c, _ in got.published])
    owner = np.repeat(np.arange(n * rows), cells["n_child_points"].reshape(-1))
    owner_g = cols[owner // rows]
    child_g = owner_g + (children["column_index"] - owner_g % ring) % ring     # a child lies in its parent's column or behind it, within the ring
    same_owner = owner[1:] == owner[:-1]
    assert (np.diff(child_g)[same_owner] >= 0).all(), "a child list is not in column order"
    keep = child_g <= cols[-1]
    eq("published children per point", np.bincount(owner[keep], minlength=n * rows), np.bincount(key, minlength=n * rows))
    eq("child_points rows", children["row_index"][keep], child[order, 1])
    eq("child_points columns", child_g[keep], child[order, 0] + lo)
    assert (~keep).sum() <= 0.01 * max(1, len(keep)), "too many children in never-published columns for the check to mean much"

    # associated_trees (cc.cpp:693-694): only roots hold them; every entry is a root of the same cluster that names this root in turn; and the
    # roots of a cluster that lies in published columns are connected through them
    trees = np.concatenate([t for *_, t in got.published])
    n_assoc = cells["n_associated_trees"]
    start = np.concatenate([[0], np.cumsum(n_assoc.reshape(-1), dtype=np.int64)])
    is_root = has_root & (rootc == cols[:, None]) & (rootr == np.arange(rows)[None, :])
    assert not (n_assoc[~is_root] != 0).any(), "associated_trees in a point that is no tree root"
    links = {}
    for c, r in np.argwhere(n_assoc > 0):
        ent = trees[start[c * rows + r]:start[c * rows + r + 1]]
        assert list(zip(ent["row_index"].tolist(), ent["column_index"].tolist())) == sorted(zip(ent["row_index"].tolist(), ent["column_index"].tolist()))
        g = int(cols[c])
        # the linked root's global column: the one within half a ring of this root that maps to the entry's slot
        og = g + ((ent["column_index"] - g % ring + ring // 2) % ring) - ring // 2
        links[(g, int(r))] = set(zip(og.tolist(), ent["row_index"].tolist()))
    parent = {}

    def find(a):
        while parent.setdefault(a, a) != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, others in links.items():
        for b in others:
            if lo <= b[0] < lo + n:
                assert is_root[b[0] - lo, b[1]], f"associated tree {b} of root {a} is no root"
                assert ref["id"][b[0] - lo, b[1]] == ref["id"][a[0] - lo, a[1]], f"associated tree {b} of root {a} belongs to another cluster"
                assert a in links.get(b, ()), f"root {a} names {b}, but not the other way round"
            parent[find(a)] = find(b)
    ids = ref["id"][is_root]
    roots = list(zip(np.broadcast_to(cols[:, None], is_root.shape)[is_root].tolist(), np.broadcast_to(np.arange(rows), is_root.shape)[is_root].tolist()))
    first_of = {}
    multi = 0
    for cid, root in zip(ids.tolist(), roots):
        if cid == 0:
            continue
        if cid in first_of:
            multi += 1
            assert find(first_of[cid]) == find(root), f"cluster {cid}: roots {first_of[cid]} and {root} are not connected through associated_trees"
        else:
            first_of[cid] = root
    return multi


def check_ground_view(name, seg, got, k):
    if not got.ground or seg.published is None:
        return
    lo, hi = seg.published_range
    cols = np.array([c for c, _ in got.ground])
    keep = (cols >= lo) & (cols <= hi)
    cells = np.stack([c for _, c in got.ground])[keep]
    idx = cols[keep] - lo
    ref = {f: a[idx] for f, a in seg.published.items()}
    for f in ("ground_point_label", "debug_ground_point_label", "is_ignored", "global_column_index"):
        eq("ground view " + f, cells[f], ref[f])
    for j, f in enumerate("xyz"):
        util.assert_float_equal("ground view " + f, cells["xyz"][..., j].copy(), ref[f])
    for f in ("distance", "inclination_angle"):
        util.assert_float_equal("ground view " + f, cells[f].copy(), ref[f])
    check_metadata("ground view", cells, ref["source_firing"], seg, k, seg.rows)
    util.assert_float_equal("ground view azimuth_angle", cells["azimuth_angle"].copy(), expected_azimuth(name, k)[idx])


def check_clusters(seg, got, k):
    sel = (seg.events["type"] == capi.EV_CLUSTER) & (seg.events["d"] > 20)
    cb, flags = seg.events[sel], seg.use_last[sel]
    lo, hi = seg.published_range
    checked = 0
    for j, (stamp, members) in enumerate(got.clusters):
        cid, (og, orow) = int(cb[j]["c"]), seg.members[j]
        where = f"segment {k}, cluster callback {j} (id {cid})"
        assert np.array_equal(members["global_column_index"], og) and np.array_equal(members["row_index"], orow), where + ": members or their order differ"
        assert (members["id"] == cid).all(), where + ": a copy without the cluster id"
        assert stamp == ds.expected_cluster_stamp(members["stamp"], flags[j]), \
            where + f": stamp {stamp} under use_last_point_for_cluster_stamp = {int(flags[j])}, members' stamps {members['stamp'].min()} .. {members['stamp'].max()}"
        keep = (og >= lo) & (og <= hi)
        src = seg.published["source_firing"][og[keep] - lo, orow[keep]]
        assert (src >= 0).all()
        eq(where + " member stamps", members["stamp"][keep], (1000000 + 45 * src).astype(np.uint64))
        eq(where + " member globally_unique_point_index", members["globally_unique_point_index"][keep],
           (np.uint64(k) << np.uint64(48)) | (src.astype(np.uint64) << np.uint64(16)) | orow[keep].astype(np.uint64))
        checked += int(keep.sum())
    return checked


@pytest.mark.parametrize("name,batch", RUNS)
def test_dropin_class_follows_the_script(tmp_path, name, batch, oracle_lib):
    base = ds.script_ops(name)
    ops = ds.with_batch(base, batch)
    at = [i for i, op in enumerate(ops) if op[0] != "BATCH"]           # operation index of the script -> of this run
    assert [ops[i][0] for i in at] == [op[0] for op in base]
    segs, queries = ds.script_record(name)
    dump = run_harness(tmp_path, ops)
    assert len(dump.segments) == len(segs)
    mode_async = [not cfg.is_single_threaded for cfg in _config_at_reset(ops)]

    # exceptions: where the oracle stops, with its sentence
    errors = [(k, s.error) for k, s in enumerate(segs) if s.error is not None]
    assert len(dump.exceptions) == len(errors), dump.exceptions
    for (k, (op, firing, rc, text)), (gop, gfiring, what) in zip(errors, dump.exceptions):
        assert what == (text + ds.OVERRUN_TAIL if rc == capi.CC_ERR_RING_OVERRUN else text)
        if mode_async[k]:
            # rethrown by a later addFiring of the operation, or by the flush behind it
            assert (gop == at[op] and gfiring > firing) or (gop == at[op] + 1 and ops[gop][0] == "FLUSH" and gfiring == -1), (gop, gfiring, op, firing)
        else:
            # thrown by the addFiring that hands the firing to the engine: the one that fills its call of `batch` firings
            last = firing + (-(firing + 1)) % batch
            assert last < base[op][3] - base[op][2] and (gop, gfiring) == (at[op], last), (gop, gfiring, op, firing, last)

    multi = members = 0
    for k, (seg, got) in enumerate(zip(segs, dump.segments)):
        assert got.rows == seg.rows
        exp = expected_order(seg.events)
        if seg.error is not None and (mode_async[k] or batch != 1):
            # (the callbacks of the engine call that failed are not delivered: in the oracle, everything the firings in front of the stale column caused)
            assert got.order == exp[:len(got.order)], f"segment {k}: callbacks are no prefix of the oracle's events"
        else:
            first_bad = next((i for i, (a, b) in enumerate(zip(got.order, exp)) if a != b), min(len(got.order), len(exp)))
            assert got.order == exp, f"segment {k}: callback {first_bad}: class {got.order[first_bad:first_bad + 3]} oracle {exp[first_bad:first_bad + 3]}"
        multi += check_published(name, k, seg, got, complete=seg.error is None) or 0
        check_ground_view(name, seg, got, k)
        members += check_clusters(seg, got, k)
    assert dump.counts[2] == 0, "a ground-view callback saw clustering-stage values"
    assert dump.counts[0] == sum(len(g.ground) for g in dump.segments) and dump.counts[1] == sum(len(g.clusters) for g in dump.segments)
    if name == "long":
        assert multi > 100, "the script was chosen to contain clusters made of several linked trees"
    if name not in ds.ERROR_SCRIPTS:
        assert members > 1000

    # QUERY records
    assert sorted(dump.queries) == [at[i] for i in sorted(queries)]
    seg_of = np.cumsum([op[0] == "RESET" for op in base]) - 1
    for i, exp in queries.items():
        q = dump.queries[at[i]]
        exp = dict(exp)
        if exp.pop("failed"):
            # after an exception: the ring indices are those of the call that failed; in the asynchronous mode the only way on is reset()
            for f in ("ring_buffer_start_global_column_index", "ring_buffer_end_global_column_index"):
                exp.pop(f), q.pop(f)
            if mode_async[seg_of[i]]:
                exp["reset_required"] = 1
        assert q == exp, f"QUERY at operation {i}: class {q} expected {exp}"


def _config_at_reset(ops):
    cfg, out = None, []
    for op in ops:
        if op[0] == "CONFIG":
            cfg = op[1]
        elif op[0] == "RESET":
            out.append(cfg)
    return out
