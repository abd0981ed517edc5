"""What the time stamps of a take cost when they are resolved in device memory, next to the host round trip they replace.
For the record: no threshold.

    python tools/stamp_cost.py [--streams 256] [--steps 8] [--warmup 3] [--out f.json]

--streams streams of 64 rows x 2200 columns, one rotation per cc_engine_add_firings_device call, events off (the throughput configuration,
the set-up of tools/take_cost.py). One engine, one FiringStamps log of 32768 firings per stream on a HIP stream of its own. Every step,
warm-up steps included, is add_firings_device + sync, push of the rotation's stamps (device memory), take_clusters(21) and take_points
into reused tensors, and then, each between host timestamps and each ending synchronised:
    of_clusters (cluster stamps + every member's stamp)          -> of_clusters_ms
    of_points (stamps + time_sec / time_nsec)                    -> of_points_ms
    of_columns (column stamps + stream stamps)                   -> of_columns_ms
    the alternative for the clusters: a D2H copy of the cluster records' source_firing, stamps[stream][source_firing] in numpy against
    the caller's own host log, min / max per cluster with reduceat and the midpoint                       -> host_clusters_ms
    the alternative for the points: the same copy and look-up for the point records, then the minimum per column with reduceat
    (zeros are not filtered: it does less than of_columns)                                                -> host_points_ms
Prints one JSON line with the medians over --steps steps, min and max, and the records, clusters and columns of a take.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import Engine, capi, stamps, synth, take  # noqa: E402

BASE = 1_700_000_000_000_000_000


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8, help="distinct scenes; stream s replays scene s mod this")
    ap.add_argument("--input-rotations", type=int, default=4, help="distinct rotations per scene, fed cyclically")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the engine has no CPU variant")
    dev = torch.device("cuda", 0)
    S, R, F, NR, NB = a.streams, 64, 2200, a.input_rotations, a.warmup + a.steps
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
    # 10 Hz rotations: firing i of stream s at BASE + i * 45454 ns + s; the host keeps the whole log, as a caller without the side-car must
    host_log = (BASE + np.arange(NB * F, dtype=np.uint64)[None, :] * np.uint64(45454) + np.arange(S, dtype=np.uint64)[:, None])
    d_log = torch.from_numpy(host_log.view(np.int64).reshape(S, NB, F).transpose(1, 0, 2).copy()).to(dev)   # [NB][S][F]
    e = Engine(cfg, R, S)
    e.record_events(False)
    fs = stamps.FiringStamps(S, 32768)
    records = torch.empty((S * F * R, 32), dtype=torch.uint8, device=dev)
    cl_records = torch.empty((S * F * R, 32), dtype=torch.uint8, device=dev)
    descriptors = torch.empty((S * F * R // 6 + 1, 64), dtype=torch.uint8, device=dev)
    d_ptable = torch.zeros(S * 48, dtype=torch.uint8, device=dev)
    out_cl = torch.empty((descriptors.shape[0], 32), dtype=torch.uint8, device=dev)
    out_cl_points = torch.empty(S * F * R, dtype=torch.int64, device=dev)
    out_points = torch.empty(S * F * R, dtype=torch.int64, device=dev)
    out_sec_nsec = torch.empty((S * F * R, 2), dtype=torch.int32, device=dev)
    out_columns = torch.empty(S * 2 * F, dtype=torch.int64, device=dev)
    out_streams = torch.empty(S, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ms = {k: [] for k in ("of_clusters_ms", "of_points_ms", "of_columns_ms", "host_clusters_ms", "host_points_ms")}
    n_cl, n_clrec, n_rec, n_cols, agree = [], [], [], [], True
    for b in range(NB):
        e.add_firings_device(F, xyz[b % NR], inten[b % NR], poses[b % NR])
        assert e.sync() == 0, e.last_error()
        fs.push(F, d_log[b])
        cl, crec, ctable = e.take_clusters(21, clusters=descriptors, records=cl_records)
        got, ptable = e.take_points(take.TAKE_CLUSTERED, take.TAKE_ALL_RETURNS, records=records, d_table=d_ptable)
        assert (ptable["error"] == 0).all() and (ctable["error"] == 0).all()
        assert int((ptable["col_to"] - ptable["col_from"]).sum()) <= out_columns.shape[0]
        fs.sync()
        t0 = time.perf_counter()
        fs.of_clusters(cl, crec, False, out=out_cl, point_stamps=out_cl_points)
        fs.sync()
        t1 = time.perf_counter()
        fs.of_points(got, d_ptable, stamps=out_points, sec_nsec=out_sec_nsec)
        fs.sync()
        t2 = time.perf_counter()
        cols, _ = fs.of_columns(got, d_ptable, ptable, column_stamps=out_columns, stream_stamps=out_streams)
        fs.sync()
        t3 = time.perf_counter()
        # the host round trip for the clusters
        sf = crec[:, 20:24].contiguous().cpu().numpy().view(np.uint32).reshape(-1)
        d = cl.cpu().numpy().reshape(-1).view(take.TAKE_CLUSTER_DTYPE)
        host_cl = None
        if len(d):
            pt = host_log[np.repeat(d["stream"], d["n_points"]), sf]
            first = d["first_record"].astype(np.int64)
            lo, hi = np.minimum.reduceat(pt, first), np.maximum.reduceat(pt, first)
            host_cl = lo + (hi - lo) // np.uint64(2)
        t4 = time.perf_counter()
        # ... and for the points
        sf = got[:, 20:24].contiguous().cpu().numpy().view(np.uint32).reshape(-1)
        col = got[:, 28:32].contiguous().cpu().numpy().view(np.uint32).reshape(-1)
        host_cols = None
        if len(sf):
            of_stream = np.repeat(np.arange(S), ptable["n_records"])
            pt = host_log[of_stream, sf]
            key = of_stream.astype(np.int64) * (1 << 32) + col
            host_cols = np.minimum.reduceat(pt, np.concatenate([[0], np.flatnonzero(np.diff(key)) + 1]))
        t5 = time.perf_counter()
        if host_cl is not None:
            agree = agree and np.array_equal(out_cl[:len(d)].cpu().numpy().reshape(-1).view(stamps.CLUSTER_STAMP_DTYPE)["stamp"], host_cl)
        if host_cols is not None:
            dev_cols = cols.cpu().numpy().view(np.uint64)
            agree = agree and np.array_equal(dev_cols[dev_cols != 0], host_cols)
        if b >= a.warmup:
            for k, v in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                ms[k].append(v * 1e3)
            n_cl.append(len(d))
            n_clrec.append(len(crec))
            n_rec.append(len(got))
            n_cols.append(len(cols))
    med = statistics.median
    res = {"streams": S, "rows": R, "columns": F, "firings_per_call": F, "steps": a.steps, "warmup": a.warmup, "log_capacity": fs.capacity}
    for k, v in ms.items():
        res[k] = round(med(v), 3)
        res[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    res.update({"clusters_per_take": int(med(n_cl)), "cluster_records_per_take": int(med(n_clrec)), "point_records_per_take": int(med(n_rec)),
                "columns_per_take": int(med(n_cols)), "missing": sum(fs.counters(s)[1] for s in range(S)), "device_equals_host": bool(agree),
                "host_clusters_over_of_clusters": round(med(ms["host_clusters_ms"]) / med(ms["of_clusters_ms"]), 1),
                "host_points_over_of_points_and_columns": round(med(ms["host_points_ms"]) / (med(ms["of_points_ms"]) + med(ms["of_columns_ms"])), 1)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    fs.close()
    e.close()


if __name__ == "__main__":
    main()
