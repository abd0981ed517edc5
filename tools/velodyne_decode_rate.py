"""The Velodyne VLS-128 decoder alone, timed with HIP events: bytes moved / kernel time, for the record (no threshold).

    python tools/velodyne_decode_rate.py [--streams 256] [--packets <one rotation at 600 rpm>] [--stride 1206] [--repeats 21] [--out f.json]

--streams x --packets payloads resident in HBM (4 distinct synthetic streams tiled over --streams, static sensor), one warm-up decode, then
--repeats decodes, each between two events on the decoder's HIP stream. Prints one JSON line: the bytes one decode moves (packets, packet
poses and skip flags read; xyz, intensity, poses and block azimuths written — the accounting of cc_velodyne.hip's header), the event
times, their median and the rate at the median. --stride 1206 is the bare payload (u16 staging), 1208 the dword path, 1216 the 16-byte path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import synth, velodyne  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--packets", type=int, default=velodyne.rotation_packets())
    ap.add_argument("--stride", type=int, default=velodyne.PACKET_BYTES)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the decoder has no CPU variant")
    dev = torch.device("cuda", 0)
    S, P, distinct = a.streams, a.packets, 4
    cal = velodyne.synthetic_calibration(0)
    per = [velodyne.synthetic_packets(cal, P, seed=900 + i, motion=synth.Motion.static(), stride=a.stride) for i in range(distinct)]
    d_packets = torch.from_numpy(np.stack([per[s % distinct]["packets"] for s in range(S)])).to(dev)
    d_pposes = torch.from_numpy(np.stack([per[s % distinct]["packet_poses"] for s in range(S)])).to(dev)
    d_skip = torch.zeros((S, P), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dec = velodyne.VelodyneDecoder(S, max_packets=P)
    dec.set_calibration(cal)
    stream = torch.cuda.ExternalStream(dec.hip_stream(), device=dev)
    out = dec.decode(d_packets, d_pposes, d_skip)                                  # warm-up
    dec.sync()
    times = []
    for _ in range(a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        dec.decode(d_packets, d_pposes, d_skip, out=out)
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    staged = {16: 1216, 4: 1208}.get(16 if a.stride % 16 == 0 else 4 if a.stride % 4 == 0 else 2, 1206)
    read = S * P * (staged + 96 + 1)
    written = S * P * 3 * (128 * 13 + 96 + 4)
    med = statistics.median(times)
    res = {"streams": S, "packets_per_stream": P, "stride": a.stride, "points": S * P * 384, "bytes_read": read, "bytes_written": written,
           "bytes_per_decode": read + written, "event_ms": [round(t, 4) for t in times], "median_ms": round(med, 4),
           "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "tb_per_s_at_median": round((read + written) / med / 1e9, 3),
           "gpoints_per_s_at_median": round(S * P * 384 / med / 1e6, 2)}
    dec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
