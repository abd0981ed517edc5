"""The Ouster decoder alone, once per UDP profile, for a kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/ouster_decode_profiles.py [--streams 256] [--packets 64]
        [--rows 64] [--repeats 3] [--profiles LEGACY,RNG19_RFL8_SIG16_NIR16,RNG19_RFL8_SIG16_NIR16_DUAL]

Per profile, in the order given: one warm-up decode, then --repeats decodes of --streams x --packets packets of --rows x 16 resident in HBM,
each followed by a synchronise. The k_ouster_decode rows of the kernel trace are in that order (1 + repeats per profile). Prints one JSON
line with the dispatch order, the bytes one decode moves and the host wall time of each repeat (launch and synchronise included: the kernel
time is the trace's). The scene is synth's (static sensor, 8 distinct streams tiled over --streams).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import ouster, synth  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--packets", type=int, default=64)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profiles", default=",".join(ouster.PROFILE_NAMES))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the decoder has no CPU variant")
    dev = torch.device("cuda", 0)
    S, P, H, Cc, distinct = a.streams, a.packets, a.rows, 16, 8
    res = {"streams": S, "packets_per_stream": P, "rows": H, "columns_per_packet": Cc, "warmup": 1, "repeats": a.repeats, "profiles": []}
    for name in a.profiles.split(","):
        meta = ouster.synthetic_metadata(H, P * Cc, Cc, udp_profile_lidar=name)
        per = [ouster.synthetic_packets(meta, P, seed=900 + i, motion=synth.Motion.static()) for i in range(distinct)]
        d_packets = torch.from_numpy(np.stack([per[s % distinct]["packets"] for s in range(S)])).to(dev)
        d_pposes = torch.from_numpy(np.stack([per[s % distinct]["packet_poses"] for s in range(S)])).to(dev)
        torch.cuda.synchronize()
        dec = ouster.OusterDecoder(S, H, Cc, max_packets=P, profile=name)
        dec.set_lut(*ouster.make_lut(meta, "reference"))
        out = dec.decode(d_packets, d_pposes)                                     # warm-up
        dec.sync()
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            dec.decode(d_packets, d_pposes, out=out)
            dec.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
        moved = d_packets.numel() + d_pposes.numel() * 8 + S * P * Cc * (H * 13 + 96)   # read packets + poses, write xyz + intensity + poses
        res["profiles"].append({"profile": name, "packet_bytes": dec.packet_bytes, "bytes_per_decode": int(moved),
                                "wall_ms": [round(w, 4) for w in wall]})
        dec.close()
        del d_packets, d_pposes, out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
