"""The generic PointCloud2 decoder alone, timed with HIP events: bytes moved / kernel time, for the record (no threshold).

    python tools/points_decode_time.py [--streams 256] [--repeats 21] [--out f.json]

Three layouts at --streams streams, message bytes resident in HBM, three warm-up decodes, then --repeats decodes each between two events
on the decoder's HIP stream:
  raw_firing          the reference's 37-byte raw-firing message, H = 128, C = 1, 64 messages per call (messages back to back: odd addresses)
  organised_aligned   a row-major organised xyzi cloud, 16-byte points, H = 64, C = 512, one message per call, 16-byte-aligned base
  organised_offset_1  the same cloud with the message base 1 byte off
and, as the yardstick on the same device, the Velodyne VLS-128 decoder at a similar input byte volume. Prints one JSON line with, per
leg, the bytes one decode reads (message bytes, message poses, skip flags) and writes (xyz, intensity, poses), the median event time and
GB/s of input plus output at the median.
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

from continuous_clustering_amd import points, synth, velodyne  # noqa: E402

WARMUP = 3


def time_calls(torch, stream, call, repeats):
    for _ in range(WARMUP):
        call()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        call()
        t1.record(stream)
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return times


def leg_result(read, written, times):
    med = statistics.median(times)
    return {"bytes_read": int(read), "bytes_written": int(written), "median_ms": round(med, 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4), "gb_per_s_at_median": round((read + written) / med / 1e6, 1)}


def points_leg(torch, dev, S, layout, M, base, repeats, distinct=4):
    rng = np.random.default_rng(layout.rows + base)
    n = M * layout.columns
    xyz = rng.normal(0, 20, (distinct, n, layout.rows, 3)).astype(np.float32)
    inten = rng.integers(0, 256, (distinct, n, layout.rows), dtype=np.uint8)
    msg = points.write_messages(xyz, inten, layout, fill=rng)                      # [distinct][M][message_bytes]
    stride = msg.shape[-1]
    buf = torch.empty(base + S * M * stride, dtype=torch.uint8, device=dev)
    d_small = torch.from_numpy(msg).to(dev)
    buf[base:].copy_(d_small[torch.arange(S, device=dev) % distinct].reshape(-1))
    d_poses = torch.from_numpy(rng.normal(size=(S, M, 12))).to(dev)
    d_skip = torch.zeros((S, M), dtype=torch.uint8, device=dev)
    dec = points.PointsDecoder(S, layout, max_messages=M)
    out = dict(xyz=torch.empty((S, n, layout.rows, 3), dtype=torch.float32, device=dev),
               intensity=torch.empty((S, n, layout.rows), dtype=torch.uint8, device=dev),
               poses=torch.empty((S, n, 12), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(dec.hip_stream(), device=dev)
    times = time_calls(torch, stream, lambda: dec.decode(buf[base:], d_poses, d_skip, out=out, n_messages=M, message_stride=stride), repeats)
    dec.sync()
    same = bool((out["xyz"][:distinct].cpu() == torch.from_numpy(xyz)).all()) and bool((out["intensity"][:distinct].cpu() == torch.from_numpy(inten)).all())
    dec.close()
    res = leg_result(S * M * (stride + 96 + 1), S * n * (layout.rows * 13 + 96), times)
    res.update(rows=layout.rows, columns=layout.columns, messages_per_call=M, message_bytes=stride, base_offset=base,
               kernel_path=points.kernel_path(layout), firings_per_workgroup=points.column_tile(layout), output_equals_input=same)
    return res


def velodyne_leg(torch, dev, S, P, repeats, distinct=4):
    cal = velodyne.synthetic_calibration(0)
    per = [velodyne.synthetic_packets(cal, P, seed=900 + i, motion=synth.Motion.static(), stride=1216) for i in range(distinct)]
    d_packets = torch.from_numpy(np.stack([per[s % distinct]["packets"] for s in range(S)])).to(dev)
    d_pposes = torch.from_numpy(np.stack([per[s % distinct]["packet_poses"] for s in range(S)])).to(dev)
    d_skip = torch.zeros((S, P), dtype=torch.uint8, device=dev)
    dec = velodyne.VelodyneDecoder(S, max_packets=P)
    dec.set_calibration(cal)
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(dec.hip_stream(), device=dev)
    out = dec.decode(d_packets, d_pposes, d_skip)
    times = time_calls(torch, stream, lambda: dec.decode(d_packets, d_pposes, d_skip, out=out), repeats)
    dec.close()
    res = leg_result(S * P * (1216 + 96 + 1), S * P * 3 * (128 * 13 + 96 + 4), times)
    res.update(packets_per_call=P, stride=1216)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the decoder has no CPU variant")
    dev = torch.device("cuda", 0)
    S = a.streams
    raw = points.raw_firing_layout(128)
    F32 = points.FLOAT32
    cloud = points.layout_from_pointcloud2(64, 512, 16, 512 * 16, [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 12, F32, 1)],
                                           intensity_mode=points.INTENSITY_F32_255)
    res = {"streams": S, "repeats": a.repeats, "warmup": WARMUP}
    res["raw_firing"] = points_leg(torch, dev, S, raw, 64, 0, a.repeats)
    res["organised_aligned"] = points_leg(torch, dev, S, cloud, 1, 0, a.repeats)
    res["organised_offset_1"] = points_leg(torch, dev, S, cloud, 1, 1, a.repeats)
    # the yardstick: packets whose bytes add up to about the raw-firing leg's input (64 x 4736 B = 249 payloads of 1216 B)
    res["velodyne_similar_raw_firing"] = velodyne_leg(torch, dev, S, 249, a.repeats)
    # and to about the organised cloud's input (524 288 B = 431 payloads)
    res["velodyne_similar_organised"] = velodyne_leg(torch, dev, S, 431, a.repeats)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
