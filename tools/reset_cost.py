"""What resetting single streams costs next to the whole reset and next to the step it interrupts. For the record: no threshold.

    python tools/reset_cost.py [--streams 256] [--steps 8] [--warmup 3] [--out f.json]

--streams streams of 64 rows x 2200 columns, one rotation per cc_engine_add_firings_device call, events off (the throughput configuration).
Every step, warm-up steps included, is
    add_firings_device + sync                        -> step_ms
    reset_streams of 1 stream                        -> reset_1_ms
    reset_streams of 16 streams                      -> reset_16_ms
    reset_streams of all --streams streams           -> reset_all_ms
    reset (cc_engine_reset, same shape)              -> reset_whole_ms
each between host timestamps and each behind a synchronised step of its own, so that a reset never pays for draining the pipeline: what is
timed is the call on an idle engine (it returns synchronised). The robot transform is set again behind every reset, outside the timing. The
listed streams are spread over the engine (a stride, not a prefix). Prints one JSON line with the medians over --steps steps, min and max,
and the bytes a reset of one stream fills.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import Engine, IDENTITY_TF, capi, synth  # noqa: E402


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
    S, R, F, NR = a.streams, 64, 2200, a.input_rotations
    cfg = capi.Config.kitti()
    sensor = synth.SensorModel.s64()
    distinct = min(a.distinct, S)
    xyz = torch.empty((NR, S, F, R, 3), dtype=torch.float32, device=dev)
    inten = torch.empty((NR, S, F, R), dtype=torch.uint8, device=dev)
    poses = torch.empty((NR, S, F, 12), dtype=torch.float64, device=dev)
    for d in range(distinct):
        st = synth.make_stream(F * NR, seed=20261019 + d, sensor=sensor, motion=synth.Motion.translate(10.0), xp=torch, device=dev, chunk=F)
        xyz[:, d::distinct] = st.xyz.view(NR, 1, F, R, 3)
        inten[:, d::distinct] = st.intensity.view(NR, 1, F, R)
        poses[:, d::distinct] = st.poses.view(NR, 1, F, 12)
    torch.cuda.synchronize()
    e = Engine(cfg, R, S)
    e.record_events(False)
    lists = {"reset_1_ms": [S // 2], "reset_16_ms": [(i * S) // 16 for i in range(min(16, S))], "reset_all_ms": list(range(S))}
    ms = {"step_ms": [], "reset_1_ms": [], "reset_16_ms": [], "reset_all_ms": [], "reset_whole_ms": []}
    feeds = [0]

    def step():
        b = feeds[0]
        feeds[0] += 1
        t0 = time.perf_counter()
        e.add_firings_device(F, xyz[b % NR], inten[b % NR], poses[b % NR])
        assert e.sync() == 0, e.last_error()
        return (time.perf_counter() - t0) * 1e3

    for it in range(a.warmup + a.steps):
        got = {"step_ms": step()}
        for name, listed in lists.items():
            step()
            t0 = time.perf_counter()
            e.reset_streams(listed)
            got[name] = (time.perf_counter() - t0) * 1e3
            for s in set(listed):
                e.set_robot_from_sensor(IDENTITY_TF, stream=s)
        step()
        t0 = time.perf_counter()
        e.reset()
        got["reset_whole_ms"] = (time.perf_counter() - t0) * 1e3
        e.set_robot_from_sensor(IDENTITY_TF)
        if it >= a.warmup:
            for k, v in got.items():
                ms[k].append(v)
    med = statistics.median
    cells = F * 10 * R
    tab_tiles = F * 10 // 64 + 2
    bytes_one = cells * (4 + 4 + 2 + 4 + 1 + 1 + 1 + 4) + tab_tiles * R * 8 + 16  # the ten planes' slices (the state and cursors are < 1 KB)
    res = {"streams": S, "rows": R, "columns": F, "firings_per_call": F, "steps": a.steps, "warmup": a.warmup, "fill_bytes_per_stream": bytes_one}
    for k, v in ms.items():
        res[k] = round(med(v), 3)
        res[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    res["reset_1_gb_per_s"] = round(bytes_one / med(ms["reset_1_ms"]) / 1e6, 1)
    res["reset_all_gb_per_s"] = round(bytes_one * S / med(ms["reset_all_ms"]) / 1e6, 1)
    res["reset_whole_gb_per_s"] = round(bytes_one * S / med(ms["reset_whole_ms"]) / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
