"""Randomised parity sweep (GPU box): many small scenes with lots of short-lived trees, odd chunkings, both sensors, both
association kernels. Engine vs oracle through tests/util.run_and_compare. Usage: python tools/stress_parity.py [--thresholds] [--returns] [--reconfigure] [n_cases] [seed0]
--thresholds: every case also takes three entries of the threshold sweep (tests/cases.py: SEGMENTATION_SWEEP, ASSOCIATION_SWEEP), drawn from a
generator of their own, so that the scenes, chunkings and options of a seed are the same with and without the switch.
--returns: every case also gets three classes of degenerate returns (tests/return_streams.py: MIXED_CLASSES — zeros, column edges, scaled, infinite,
partly NaN, duplicates, lone returns, gaps) planted at about 2 % of its returns behind the first rotation, drawn from a generator of their own as well;
the oracle's error text (a dropped NaN azimuth) must be the engine's.
--reconfigure: every case changes its configuration twice in mid-stream and its robot transform once (tests/reconfigure_streams.py: CONFIG_TABLE,
TRANSFORM_TABLE; the firings and the entries drawn from a generator of their own): set_config / set_robot_from_sensor between two calls, the oracle
under the same schedule (tests/util.run_schedule_and_compare)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import util, cases
from continuous_clustering_amd import synth
from continuous_clustering_amd.synth import Motion, SceneModel
from oracle import pyoracle
pyoracle.build()

args = [a for a in sys.argv[1:] if a not in ("--thresholds", "--returns", "--reconfigure")]
thresholds = "--thresholds" in sys.argv[1:]
returns = "--returns" in sys.argv[1:]
reconfigure = "--reconfigure" in sys.argv[1:]
n_cases = int(args[0]) if len(args) > 0 else 12
seed0 = int(args[1]) if len(args) > 1 else 1000
# (read only with the switch: without it the tool needs nothing of tests/cases.py beyond the sensors and configurations it always used)
SWEPT = {**cases.SEGMENTATION_SWEEP, **cases.ASSOCIATION_SWEEP} if thresholds else {}
if returns:  # (likewise: tests/return_streams.py is read only with its switch)
    import return_streams
if reconfigure:  # (likewise)
    import reconfigure_streams
bad = 0
for i in range(n_cases):
    rng = np.random.default_rng(seed0 + i)
    s128 = (i % 4) == 3
    cols = int(rng.choice([240, 360, 480, 720]))
    sensor = cases._s128(cols) if s128 else cases._s64(cols)
    scene = SceneModel(n_objects=int(rng.integers(0, 200)), object_range=(2.0, float(rng.uniform(8, 30))),
                       object_radius=(0.05, float(rng.uniform(0.15, 1.0))), wall_radius=float(rng.choice([0.0, 10.0, 25.0, 45.0])),
                       wall_gaps_deg=() if rng.random() < 0.3 else ((20.0, 32.0), (140.0, 155.0)),
                       range_noise=float(rng.choice([0.01, 0.05, 0.2])), dropout=float(rng.choice([0.02, 0.1, 0.3])))
    motion = [Motion.static(), Motion.translate(float(rng.uniform(1, 20))), Motion.turn(8.0, float(rng.uniform(-1, 1)))][int(rng.integers(0, 3))]
    n = cols * int(rng.integers(2, 4)) + int(rng.integers(0, cols))
    stream = synth.make_stream(n, seed=seed0 + 17 * i, sensor=sensor, scene=scene, motion=motion)
    planted = []
    if returns:
        rrng = np.random.default_rng([seed0 + i, 11])
        # (the edge classes aim whole firings at a column boundary: not with per-laser azimuth offsets)
        table = [c for c in return_streams.MIXED_CLASSES if not (s128 and c in return_streams.EDGE_CLASSES)]
        planted = [str(k) for k in rrng.choice(table, size=3, replace=False)]
        stream = return_streams.plant_mixed(stream, seed0 + i, classes=tuple(planted))[0]
    over = {}
    if rng.random() < 0.3:
        over["max_distance"] = float(rng.choice([0.4, 0.7, 1.2]))
    if rng.random() < 0.2:
        over["stop_after_association_enabled"] = 0
    swept = []
    if thresholds:
        trng = np.random.default_rng([seed0 + i, 7])
        swept = [str(k) for k in trng.choice(sorted(SWEPT), size=3, replace=False)]
        for k in swept:
            over.update(SWEPT[k])
    cfg = (cases._vls if s128 else cases._kitti)(cols, **over)
    chunks = [int(c) for c in rng.choice([1, 3, 17, 64, 97, 250, cols, 2 * cols], size=4)]
    waves = [0, 4, 3, 1][i % 4]  # default (k_assoc3 + links wavefront), pinned four / three waves, k_assoc_lds
    batch = 0 if i % 7 == 6 else 1  # the batch-parallel kernel in front (default) or not
    rounds = [0, 2, 1, 3][i % 4]
    box = {}
    setup = lambda e: (e.set_option("assoc_waves", waves), e.set_option("assoc_batch", batch), e.set_option("assoc_rounds", rounds), box.setdefault("e", e))
    changed = []
    try:
        if reconfigure:
            crng = np.random.default_rng([seed0 + i, 13])
            at = sorted(int(a) for a in crng.choice(np.arange(cols // 2, n - 1), size=2, replace=False))
            entries = [str(k) for k in crng.choice(sorted(reconfigure_streams.CONFIG_TABLE), size=2, replace=False)]
            tf_name = str(crng.choice(sorted(reconfigure_streams.TRANSFORM_TABLE)))
            maker = cases._vls if s128 else cases._kitti
            cfgs = [maker(cols, **{**over, **reconfigure_streams.CONFIG_TABLE[k]}) for k in entries]
            schedule = reconfigure_streams.cut(n, at, [(cfg, None), (cfgs[0], None), (cfgs[1], reconfigure_streams.TRANSFORM_TABLE[tf_name])])
            changed = list(zip(at, entries, (None, tf_name)))
            record = util.schedule_oracle_record(stream, schedule)
            summ = util.run_schedule_and_compare(stream, schedule, chunks, engine_setup=setup, oracle=record)
            otext = record[0].last_error()
        else:
            summ = util.run_and_compare(stream, cfg, chunks=chunks, robot_tf=None, engine_setup=setup)
            otext = util.run_oracle(stream, cfg)[0].last_error() if returns else None
        es = summ["engine_state"]
        if returns:
            assert box["e"].last_error() == otext, f"error text: oracle {otext!r} engine {box['e'].last_error()!r}"
        bc = box["e"].batch_counters()
        print(f"case {i:3d} ok: rows {sensor.num_rows} cols {cols} firings {n} objects {scene.n_objects} chunks {chunks} waves {waves} "
              f"clusters {summ['clusters']} serial columns {es['error_b']} batch {batch} rounds {rounds} columns {bc['batch_columns']} "
              f"bails {bc['batch_bails']} {bc['bail_reasons'][1:7]}" + (f" thresholds {swept}" if thresholds else "") +
              (f" returns {planted}" if returns else "") + (f" reconfigured {changed}" if reconfigure else ""), flush=True)
    except AssertionError as ex:
        bad += 1
        print(f"case {i:3d} FAILED (seed {seed0 + i}{', thresholds ' + str(swept) if thresholds else ''}{', returns ' + str(planted) if returns else ''}"
              f"{', reconfigured ' + str(changed) if reconfigure else ''}): {str(ex)[:300]}", flush=True)
print("failures:", bad)
sys.exit(1 if bad else 0)
