"""Ouster packets -> GPU decoder -> engine, against firings -> engine, on the shape of a 256-stream 64 x 2048 LEGACY fleet.

    python tools/ouster_feed.py [--streams 256] [--steps 6] [--repeats 3] [--out profiles/ouster_feed.json]
    python tools/ouster_feed.py --decode-only --iters 20        # the decoder alone (run under rocprofv3 --kernel-trace --stats)

One step = one rotation of every stream (128 packets of 16 columns = 2048 firings per stream). Legs, alternated in one process, median of
--repeats:
  device_packets   packets resident in HBM -> cc_ouster_decode on cc_engine_hip_stream(e) -> cc_engine_add_firings_device
  device_firings   the same firings resident in HBM -> cc_engine_add_firings_device
  pcie_packets     pinned host packets -> H2D on a copy stream -> decode -> engine
  pcie_firings     pinned host firings (xyz, intensity, poses) -> H2D on a copy stream -> engine
The scene is synth's (static sensor, 8 distinct streams tiled over --streams), every rotation the same packets.
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

from continuous_clustering_amd import Engine, capi, ouster, synth  # noqa: E402


def make_inputs(meta, S, distinct=8):
    P = ouster.rotation_packets(meta)
    per = [ouster.synthetic_packets(meta, P, seed=900 + i, motion=synth.Motion.static()) for i in range(distinct)]
    packets = np.stack([per[s % distinct]["packets"] for s in range(S)])
    poses = np.stack([per[s % distinct]["packet_poses"] for s in range(S)])
    return packets, poses


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--columns", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch
    dev = torch.device("cuda", 0)
    meta = ouster.synthetic_metadata(a.rows, a.columns, 16)
    S, H, Cc, P = a.streams, a.rows, 16, ouster.rotation_packets(meta)
    F = P * Cc
    lut = ouster.make_lut(meta, "reference")
    h_packets, h_pposes = make_inputs(meta, S)
    d_packets = torch.from_numpy(h_packets).to(dev)
    d_pposes = torch.from_numpy(h_pposes).to(dev)
    torch.cuda.synchronize()
    pkt_bytes = h_packets.nbytes
    fire_bytes = S * F * (H * 12 + H + 96)
    decode_bytes = pkt_bytes + h_pposes.nbytes + fire_bytes        # read packets + packet poses, write xyz + intensity + poses

    if a.decode_only:
        dec = ouster.OusterDecoder(S, H, Cc, max_packets=P)
        dec.set_lut(*lut)
        out = dec.decode(d_packets, d_pposes)
        dec.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            dec.decode(d_packets, d_pposes, out=out)
        dec.sync()
        el = (time.perf_counter() - t0) / a.iters
        print(json.dumps({"decode_only": True, "streams": S, "packets_per_stream": P, "bytes_per_rotation": decode_bytes,
                          "wall_ms_per_rotation": el * 1e3, "wall_TBs": decode_bytes / el / 1e12}))
        return

    cfg = capi.Config.default()
    cfg.num_columns = a.columns
    nb = a.warmup + a.steps

    def engine():
        e = Engine(cfg, H, S)
        e.record_events(False)
        e.set_option("input_on_engine_stream", 1)
        return e

    # the firing-fed legs' inputs: exactly what the decoder makes of the packets
    e_ref = engine()
    dec_ref = ouster.OusterDecoder(S, H, Cc, max_packets=P, hip_stream=e_ref.hip_stream())
    dec_ref.set_lut(*lut)
    firings = dec_ref.decode(d_packets, d_pposes)
    dec_ref.sync()
    firings = {k: firings[k] for k in ("xyz", "intensity", "poses")}
    dec_ref.close()
    e_ref.close()

    def run_device(kind):
        e = engine()
        if kind == "packets":
            dec = ouster.OusterDecoder(S, H, Cc, max_packets=P, hip_stream=e.hip_stream())
            dec.check_engine(e)
            dec.set_lut(*lut)
            bufs = [{k: torch.empty_like(v) for k, v in firings.items()} for _ in range(nb)]
            torch.cuda.synchronize()
        t0 = None
        for b in range(nb):
            if b == a.warmup:
                if e.sync() != 0:
                    raise SystemExit(e.last_error())
                before = e.totals()["cells_published"]
                t0 = time.perf_counter()
            if kind == "packets":
                o = dec.decode(d_packets, d_pposes, out=bufs[b])
                e.add_firings_device(F, o["xyz"], o["intensity"], o["poses"])
            else:
                e.add_firings_device(F, firings["xyz"], firings["intensity"], firings["poses"])
        if e.sync() != 0:
            raise SystemExit(e.last_error())
        el = time.perf_counter() - t0
        cells = e.totals()["cells_published"] - before
        if kind == "packets":
            dec.close()          # before the engine whose HIP stream it uses
        e.close()
        return dict(ms_per_step=el / a.steps * 1e3, Mpoints_per_s=S * F * H * a.steps / el / 1e6, cells_published=int(cells))

    h_firings = {k: v.cpu().pin_memory() for k, v in firings.items()}
    h_packets_pinned = torch.from_numpy(h_packets).pin_memory()
    h_pposes_pinned = torch.from_numpy(h_pposes).pin_memory()

    def run_pcie(kind):
        e = engine()
        copy_stream = torch.cuda.Stream(device=dev)
        if kind == "packets":
            dec = ouster.OusterDecoder(S, H, Cc, max_packets=P, hip_stream=e.hip_stream())
            dec.set_lut(*lut)
            host = (h_packets_pinned, h_pposes_pinned)
            devb = [(torch.empty_like(d_packets), torch.empty_like(d_pposes)) for _ in range(nb)]
            outs = [{k: torch.empty_like(v) for k, v in firings.items()} for _ in range(nb)]
        else:
            host = (h_firings["xyz"], h_firings["intensity"], h_firings["poses"])
            devb = [tuple(torch.empty_like(firings[k]) for k in ("xyz", "intensity", "poses")) for _ in range(nb)]
        h2d = sum(int(t.numel() * t.element_size()) for t in host)
        evs = [torch.cuda.Event() for _ in range(nb)]
        torch.cuda.synchronize()

        def start_copy(b):
            with torch.cuda.stream(copy_stream):
                for d, h in zip(devb[b], host):
                    d.copy_(h, non_blocking=True)
                evs[b].record(copy_stream)

        def feed(b):
            evs[b].synchronize()
            if b + 1 < nb:
                start_copy(b + 1)
            if kind == "packets":
                o = dec.decode(devb[b][0], devb[b][1], out=outs[b])
                e.add_firings_device(F, o["xyz"], o["intensity"], o["poses"])
            else:
                e.add_firings_device(F, *devb[b])

        start_copy(0)
        for b in range(a.warmup):
            feed(b)
        if e.sync() != 0:
            raise SystemExit(e.last_error())
        before = e.totals()["cells_published"]
        t0 = time.perf_counter()
        for b in range(a.warmup, nb):
            feed(b)
        if e.sync() != 0:
            raise SystemExit(e.last_error())
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        cells = e.totals()["cells_published"] - before
        if kind == "packets":
            dec.close()
        e.close()
        return dict(ms_per_step=el / a.steps * 1e3, Mpoints_per_s=S * F * H * a.steps / el / 1e6, h2d_bytes_per_step=h2d,
                    pcie_GBs=h2d * a.steps / el / 1e9, cells_published=int(cells))

    legs = {"device_packets": lambda: run_device("packets"), "device_firings": lambda: run_device("firings"),
            "pcie_packets": lambda: run_pcie("packets"), "pcie_firings": lambda: run_pcie("firings")}
    runs = {k: [] for k in legs}
    for r in range(a.repeats):
        order = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in order:
            runs[k].append(legs[k]())
    res = {"shape": f"{S} streams x {H} x {a.columns} LEGACY, {P} packets of {Cc} columns per rotation, config num_columns {a.columns}",
           "steps": a.steps, "repeats": a.repeats, "packet_bytes_per_step": pkt_bytes, "firing_bytes_per_step": fire_bytes,
           "decode_bytes_per_rotation": decode_bytes}
    for k, v in runs.items():
        med = statistics.median(x["ms_per_step"] for x in v)
        res[k] = dict(ms_per_step_median=med, ms_per_step_all=[round(x["ms_per_step"], 3) for x in v],
                      Mpoints_per_s_median=S * F * H / (med / 1e3) / 1e6, cells_published=[x["cells_published"] for x in v],
                      **({"pcie_GBs_median": statistics.median(x["pcie_GBs"] for x in v), "h2d_bytes_per_step": v[0]["h2d_bytes_per_step"]}
                         if "pcie" in k else {}))
    res["device_packets_over_firings"] = res["device_packets"]["ms_per_step_median"] / res["device_firings"]["ms_per_step_median"]
    res["pcie_packets_over_firings_rate"] = res["pcie_packets"]["Mpoints_per_s_median"] / res["pcie_firings"]["Mpoints_per_s_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
