"""What the scatter and evaluation bookkeeping of a replay step costs, per stream and per frame on the host (evaluation.DeviceFrameScatter)
and as one device call for all streams (evaluation.BatchedFrameScatter, cc_replay_eval_step). For the record: no threshold.

    python tools/replay_eval_cost.py [--streams 11 64] [--steps 8] [--warmup 3] [--distinct 4] [--cols-per-row 2083] [--out f.json]

Synthetic KITTI-format sequences (kitti.write_synthetic_sequence; --distinct of them on disk, stream s replays sequence s mod --distinct),
one frame per step through replay.replay, which takes host timestamps around its publish block — the scatter of what the step published and
the evaluation of the frames that completed, ending synchronised. Both scatterers run in this process, one after the other per stream count,
on the same files. The last step of a run (it also evaluates the final frames) is left out: the sequences are one frame longer than
--warmup + --steps. Prints one JSON line per stream count with the medians over --steps steps, min and max, and the batched path's counters."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from continuous_clustering_amd import kitti, replay  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[11, 64])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--cols-per-row", type=int, default=2083)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the engine has no CPU variant")
    n_frames = a.warmup + a.steps + 1
    lines = []
    with tempfile.TemporaryDirectory() as root:
        for d in range(a.distinct):
            kitti.write_synthetic_sequence(root, d, n_frames, seed=900 + 20 * d, motion=(6.0 + d, 0.05 * d, 0.0, 0.1), cols_per_row=a.cols_per_row)
        for S in a.streams:
            seqs = [s % a.distinct for s in range(S)]
            res = {"streams": S, "frames_per_step": S, "steps": a.steps, "warmup": a.warmup, "cols_per_row": a.cols_per_row}
            records = {}
            for kind in ("device", "batched"):
                timing = {"sync_publish": True}
                records[kind], totals = replay.replay(root, seqs, max_frames=n_frames, timing=timing, scatter=kind)
                ms = timing["publish_ms"][a.warmup:a.warmup + a.steps]
                res[kind + "_publish_ms"] = round(statistics.median(ms), 3)
                res[kind + "_publish_ms_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
                res[kind + "_step_ms"] = round(timing["device_s"] / n_frames * 1e3, 3)   # convert + engine + publish, mean over all steps
                if kind == "batched":
                    c = timing["counters"]
                    res["batched_counters"] = c
                    res["batched_launches_per_step"] = round(c["kernel_launches"] / c["steps"], 2)
                    res["batched_syncs_per_step"] = round(c["host_syncs"] / c["steps"], 2)
            res["records_equal"] = sorted(records["device"]) == sorted(records["batched"])
            res["records"] = len(records["batched"])
            res["device_over_batched"] = round(res["device_publish_ms"] / res["batched_publish_ms"], 2)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
