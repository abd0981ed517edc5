"""What the device-to-device hand-over costs next to the step it follows, and next to the per-stream host reads it replaces.
For the record: no threshold.

    python tools/take_cost.py [--streams 256] [--steps 8] [--warmup 3] [--out f.json] [--clusters]

--streams streams of 64 rows x 2200 columns, one rotation per cc_engine_add_firings_device call, events off (the throughput configuration).
Every step, warm-up steps included, is
    add_firings_device + sync                                   -> step_ms
    take_points(CLUSTERED, ALL_RETURNS) into a reused tensor     -> take_ms      (what was published by the step, all streams, in HBM)
    read_columns over the SAME ranges, one call per stream       -> host_reads_ms (the only way before: one kernel, one copy, one
                                                                    synchronisation per stream, into reused host arrays; the seven
                                                                    fields a record carries, intensity has no host view)
all three between host timestamps (each ends synchronised). Prints one JSON line with the medians over --steps steps, the records and
bytes of a take, and the take's rate.

--clusters times the hand-over of the finished clusters instead, on the same set-up. Two engines are fed the same data, since
a cluster take consumes (the point take has cursors of its own and shares the first engine); after every step
    take_clusters(21) with points, into reused tensors           -> clusters_ms
    take_clusters(21) descriptors only                           -> descriptors_ms
    take_points(CLUSTERED, WITH_ID) + a stable torch.sort on the device by (stream, id), synchronised
                                                                 -> sort_baseline_ms (what a consumer does today for grouped points: it
                                                                    yields neither descriptors nor clusters ahead of publication)
and the line carries the medians over --steps steps with min and max.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import Engine, capi, synth, take  # noqa: E402

RECORD_FIELDS = ("x", "y", "z", "distance", "id", "ground_point_label", "source_firing")


def clusters_main(a):
    """--clusters: see the module's docstring"""
    import torch
    dev = torch.device("cuda", 0)
    S, R, F, NR = a.streams, 64, 2200, a.input_rotations
    cfg = capi.Config.kitti()
    sensor = synth.SensorModel.s64()
    distinct = min(a.distinct, S)
    xyz = torch.empty((NR, S, F, R, 3), dtype=torch.float32, device=dev)
    inten = torch.empty((NR, S, F, R), dtype=torch.uint8, device=dev)
    poses = torch.empty((NR, S, F, 12), dtype=torch.float64, device=dev)
    for d in range(distinct):
        st = synth.make_stream(F * NR, seed=20261018 + d, sensor=sensor, motion=synth.Motion.translate(10.0), xp=torch, device=dev, chunk=F)
        xyz[:, d::distinct] = st.xyz.view(NR, 1, F, R, 3)
        inten[:, d::distinct] = st.intensity.view(NR, 1, F, R)
        poses[:, d::distinct] = st.poses.view(NR, 1, F, 12)
    torch.cuda.synchronize()
    engines = [Engine(cfg, R, S) for _ in range(2)]
    for e in engines:
        e.record_events(False)
    records = torch.empty((S * F * R, 32), dtype=torch.uint8, device=dev)  # a rotation of every stream with a return in every cell
    descriptors = torch.empty((S * F * R // 6 + 1, 64), dtype=torch.uint8, device=dev)  # (a cluster with an id has at least six points)
    stream_ids = torch.arange(S, device=dev)
    ms = {"clusters_ms": [], "descriptors_ms": [], "sort_baseline_ms": []}
    n_cl, n_rec, n_sorted, lost = [], [], [], 0
    for b in range(a.warmup + a.steps):
        for e in engines:
            e.add_firings_device(F, xyz[b % NR], inten[b % NR], poses[b % NR])
            assert e.sync() == 0, e.last_error()
        t0 = time.perf_counter()
        cl, rec, table = engines[0].take_clusters(21, clusters=descriptors, records=records)
        t1 = time.perf_counter()
        cl_d, _, table_d = engines[1].take_clusters(21, descriptors_only=True, clusters=descriptors)
        t2 = time.perf_counter()
        got, tab = engines[0].take_points(take.TAKE_CLUSTERED, take.TAKE_WITH_ID, records=records)
        n = len(got)
        if n:
            # (stream, id) as one key: the stream of a record from the table's slices, the id from the record's bytes 16..19
            counts = torch.from_numpy(tab["n_records"].astype("int64")).to(dev)
            key = (torch.repeat_interleave(stream_ids, counts) << 32) | got[:, 16:20].contiguous().view(torch.int32).view(-1).to(torch.int64)
            order = torch.sort(key, stable=True).indices
            grouped = got[order]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert (table["error"] == 0).all() and len(cl) == len(cl_d)
        lost += int(table["lost_columns"].sum())
        if b >= a.warmup:
            ms["clusters_ms"].append((t1 - t0) * 1e3)
            ms["descriptors_ms"].append((t2 - t1) * 1e3)
            ms["sort_baseline_ms"].append((t3 - t2) * 1e3)
            n_cl.append(len(cl))
            n_rec.append(len(rec))
            n_sorted.append(n)
    med = statistics.median
    res = {"mode": "clusters", "streams": S, "rows": R, "columns": F, "firings_per_call": F, "steps": a.steps, "warmup": a.warmup, "min_points": 21}
    for k, v in ms.items():
        res[k] = round(med(v), 3)
        res[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    res.update({"clusters_per_take": int(med(n_cl)), "records_per_take": int(med(n_rec)), "sort_baseline_records_per_take": int(med(n_sorted)),
                "lost_columns": lost, "clusters_over_sort_baseline": round(med(ms["clusters_ms"]) / med(ms["sort_baseline_ms"]), 3)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in engines:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8, help="distinct scenes; stream s replays scene s mod this")
    ap.add_argument("--input-rotations", type=int, default=4, help="distinct rotations per scene, fed cyclically")
    ap.add_argument("--out", default=None)
    ap.add_argument("--clusters", action="store_true", help="time cc_engine_take_clusters and the take_points + sort it replaces (DESIGN.md §16)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the engine has no CPU variant")
    if a.clusters:
        return clusters_main(a)
    dev = torch.device("cuda", 0)
    S, R, F, NR = a.streams, 64, 2200, a.input_rotations
    cfg = capi.Config.kitti()
    sensor = synth.SensorModel.s64()
    distinct = min(a.distinct, S)
    xyz = torch.empty((NR, S, F, R, 3), dtype=torch.float32, device=dev)
    inten = torch.empty((NR, S, F, R), dtype=torch.uint8, device=dev)
    poses = torch.empty((NR, S, F, 12), dtype=torch.float64, device=dev)
    for d in range(distinct):
        st = synth.make_stream(F * NR, seed=20261018 + d, sensor=sensor, motion=synth.Motion.translate(10.0), xp=torch, device=dev, chunk=F)
        xyz[:, d::distinct] = st.xyz.view(NR, 1, F, R, 3)
        inten[:, d::distinct] = st.intensity.view(NR, 1, F, R)
        poses[:, d::distinct] = st.poses.view(NR, 1, F, 12)
    torch.cuda.synchronize()
    e = Engine(cfg, R, S)
    e.record_events(False)
    records = torch.empty((S * F * R, 32), dtype=torch.uint8, device=dev)  # a rotation of every stream with a return in every cell
    view, arrays = capi.make_column_view(2 * F, R, RECORD_FIELDS)
    step_ms, take_ms, reads_ms, n_rec, n_cols = [], [], [], [], []
    for b in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        e.add_firings_device(F, xyz[b % NR], inten[b % NR], poses[b % NR])
        assert e.sync() == 0, e.last_error()
        t1 = time.perf_counter()
        got, table = e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS, records=records)
        t2 = time.perf_counter()
        assert (table["error"] == 0).all() and (table["lost_columns"] == 0).all(), table
        t3 = time.perf_counter()
        for s in range(S):
            lo, hi = int(table[s]["col_from"]), int(table[s]["col_to"]) - 1
            if hi >= lo:
                assert hi - lo < 2 * F
                e._check(e.L.cc_engine_read_columns(e.h, s, lo, hi, C.byref(view)))
        t4 = time.perf_counter()
        if b >= a.warmup:
            step_ms.append((t1 - t0) * 1e3)
            take_ms.append((t2 - t1) * 1e3)
            reads_ms.append((t4 - t3) * 1e3)
            n_rec.append(len(got))
            n_cols.append(int((table["col_to"] - table["col_from"]).sum()))
    med = statistics.median
    res = {"streams": S, "rows": R, "columns": F, "firings_per_call": F, "steps": a.steps, "warmup": a.warmup,
           "step_ms": round(med(step_ms), 3), "take_ms": round(med(take_ms), 3), "host_reads_ms": round(med(reads_ms), 3),
           "take_ms_min_max": [round(min(take_ms), 3), round(max(take_ms), 3)],
           "host_reads_ms_min_max": [round(min(reads_ms), 3), round(max(reads_ms), 3)],
           "records_per_take": int(med(n_rec)), "columns_per_take": int(med(n_cols)), "record_bytes_per_take": int(med(n_rec)) * 32,
           "take_over_step": round(med(take_ms) / med(step_ms), 4), "host_reads_over_take": round(med(reads_ms) / med(take_ms), 2),
           "take_gb_per_s_written": round(med(n_rec) * 32 / med(take_ms) / 1e6, 1), "host_read_fields": list(RECORD_FIELDS)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
