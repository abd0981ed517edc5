"""GPU: bench.py --dump-outputs writes what the timed path computed in its last step (stream states of every stream, the newest published
rotation of a seeded sample of streams) as float32 / float64 .npy files within 64 MB, and the same arguments give the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, STREAMS = 3, 2, 12


def run_dump(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(STREAMS), "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}


@pytest.mark.gpu
def test_dump_outputs_of_the_last_step_are_complete_and_repeatable(tmp_path):
    out, a = run_dump(tmp_path / "a")
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["ms_per_step"] > 0 and out["value"] > 0
    assert abs(out["value"] - out["cells_published"] / (out["ms_per_step"] * STEPS / 1e3) / 1e6) < 1e-6 * out["value"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    for name, v in a.items():
        assert np.isfinite(v).all(), name
    # cells without a return: NaN in the engine's view, 0 in the dump and marked in the class file
    assert (a["columns_distance_class"] == 1).any() and (a["columns_distance_class"] == 0).any()
    assert set(np.unique(a["columns_distance_class"])) <= {0.0, 1.0, 2.0, 3.0}
    assert (a["columns_distance"][a["columns_distance_class"] != 0] == 0).all()
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    assert a["state"].shape == (STREAMS, 10) and (a["state"][:, 7] > 0).all()  # cells_published of every stream
    meta = a["columns_meta"]
    k, n_cols = meta.shape[0], int(meta[0, 2] - meta[0, 1] + 1)
    assert 1 <= k <= STREAMS and n_cols == 2200
    for name, v in a.items():
        if name.startswith("columns_") and name != "columns_meta":
            assert v.shape == (k, n_cols, 64), (name, v.shape)
    # the newest rotation of each sampled stream ends at its last published column (state: first_unpublished - 1)
    assert np.array_equal(meta[:, 2], a["state"][meta[:, 0].astype(int), 4] - 1)
    assert np.array_equal(a["columns_global_column_index"][:, :, 0], meta[:, 1:2] + np.arange(n_cols)[None, :])
    assert (a["columns_ground_point_label"] != 0).any() and (a["columns_id"] != 0).any()
    _, b = run_dump(tmp_path / "b")
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_inputs_fed_cyclically_stay_equal_to_the_oracle():
    """A leg longer than --input-rotations feeds the generated rotations again (the pose steps back at each wrap, the columns continue):
    the oracle replays exactly the batches as fed and the engine must still equal it, stream state and published columns."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", "8", "--steps", "9", "--warmup", "2", "--input-rotations", "4",
           "--full", "--repeats", "1", "--verify-streams", "2", "--no-s128", "--no-cpu-baseline", "--no-latency", "--no-few-streams", "--no-host-fed",
           "--no-cluttered", "--no-strong-split"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 9 and out["verified_streams"] == 2
    assert out["cells_published"] > 0
