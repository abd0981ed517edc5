"""What the per-firing poses of one replay step cost on the host path and on the device path. For the record: no threshold.

    python tools/pose_cost.py [--streams 11 256] [--steps 8] [--warmup 3] [--out f.json]

Per stream count, streams x 2200 firings per step over synthetic pose tracks (kitti.synthetic_poses, a different yaw rate per stream),
the pose part of a step of replay.replay alone, every step, warm-up steps included:
    host    kitti.firing_stamps_and_poses per stream into h_pose, torch.from_numpy(h_pose).to(device), torch.cuda.synchronize
                                                                    -> host_ms (host_interpolate_ms of it before the upload)
    twin    the same with poses.host_sweep                           -> twin_ms
    device  one PoseTracks.sweep into a persistent d_pose            -> device_enqueue_ms until the call returns (all that a replay step
                                                                       waits for), device_ms with a synchronisation behind it
all between host timestamps. Prints one JSON line per stream count with the medians over --steps steps and their min and max, and whether
the device poses equalled the twin's bit for bit on the last step.
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

from continuous_clustering_amd import kitti, poses  # noqa: E402


def measure(S: int, steps: int, warmup: int) -> dict:
    import torch
    dev = torch.device("cuda", 0)
    n_frames = steps + warmup
    seqs = []
    for s in range(S):
        rows, times = kitti.synthetic_poses(n_frames, motion=(6.0 + 0.01 * s, 0.1, 0.0, 0.05 + 0.002 * s))
        stamps = np.array([1_700_000_000_000_000_000 + int(t * 1000000000) for t in times], dtype=np.uint64)
        track = np.stack([kitti.pose_from_line(r, kitti.CALIB_TR) for r in rows])
        seqs.append((stamps, track, *kitti.start_end_stamps(stamps)))
    tracks = poses.PoseTracks(S, n_frames)
    for s, (stamps, track, _, _) in enumerate(seqs):
        tracks.set(s, stamps, track)
    h_pose = np.zeros((S, kitti.COLS, 12), dtype=np.float64)
    d_pose = torch.empty((S, kitti.COLS, 12), dtype=torch.float64, device=dev)
    start, end = np.zeros(S, dtype=np.uint64), np.zeros(S, dtype=np.uint64)
    ms = {k: [] for k in ("host_ms", "host_interpolate_ms", "twin_ms", "device_enqueue_ms", "device_ms")}
    equal = False
    for f in range(n_frames):
        t0 = time.perf_counter()
        for s, (stamps, track, st, en) in enumerate(seqs):
            h_pose[s] = kitti.firing_stamps_and_poses(stamps, track, st[f], en[f])[1]
        t1 = time.perf_counter()
        d_host = torch.from_numpy(h_pose).to(dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        for s, (stamps, track, st, en) in enumerate(seqs):
            h_pose[s] = poses.host_sweep(stamps, track, kitti.COLS, st[f], en[f])[1]
        d_twin = torch.from_numpy(h_pose).to(dev)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        for s, (_, _, st, en) in enumerate(seqs):
            start[s], end[s] = st[f], en[f]
        tracks.sweep(kitti.COLS, start, end, d_pose)
        t4 = time.perf_counter()
        tracks.sync()
        t5 = time.perf_counter()
        if f >= warmup:
            for k, v in zip(ms, (t2 - t0, t1 - t0, t3 - t2, t4 - t3, t5 - t3)):
                ms[k].append(v * 1e3)
        equal = bool(torch.equal(d_pose.view(torch.int64), d_twin.view(torch.int64)))
    tracks.close()
    med = statistics.median
    res = {"streams": S, "firings": kitti.COLS, "steps": steps, "warmup": warmup, "pose_bytes": S * kitti.COLS * 96}
    for k, v in ms.items():
        res[k] = round(med(v), 4)
        res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    res["host_over_device"] = round(med(ms["host_ms"]) / med(ms["device_ms"]), 1)
    res["device_gb_per_s_written"] = round(S * kitti.COLS * 96 / med(ms["device_ms"]) / 1e6, 1)
    res["device_equals_twin"] = equal
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[11, 256])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the device path has no CPU variant")
    lines = [json.dumps(measure(S, a.steps, a.warmup)) for S in a.streams]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
