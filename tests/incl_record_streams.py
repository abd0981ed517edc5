"""Streams for the tests of the single copy of a cell's inclination (Planes::sc_rec.w; tests/test_incl_record_cpu.py,
tests/test_gpu_incl_record.py). Smallest shapes at which a stale record can show: 8 and 12 rows, 64 columns per rotation (a ring of 640
columns), 13 passes over the ring.

A cell's record is not cleared when its column is released, so the cell of ring slot (lc, row) still holds what pass p wrote when pass p + 1
comes by. The stale row makes that visible: it has a return in every column of the even passes and none in the odd ones, so behind every one
of its cells without a return lies a record with a valid inclination of the pass before."""
import numpy as np

from continuous_clustering_amd import capi, synth

COLS = 64
RING = 10 * COLS     # cc.cpp:17
PASSES = 13
EDGE = 8             # firings at either end of an odd pass in which the row below the stale row stays as it is (stale_stream)
OFFSETS = (-6.4, -2.7, 0.9, 4.5)   # per-laser azimuth offsets (degrees) of the multi-column firing shape: a firing spans three columns of 5.6 degrees


def stale_row(rows):
    return rows - 2   # looks at the ground 5 m ahead (a return in every firing), with a row below it (the supplement's source) and one above


def sensor(rows, multi_column=False):
    return synth.SensorModel(num_rows=rows, num_columns=COLS, azimuth_offsets_deg=OFFSETS if multi_column else ())


def config(supplement=True):
    cfg = capi.Config.kitti()
    cfg.num_columns = COLS
    cfg.supplement_inclination_angle_for_nan_cells = 1 if supplement else 0
    return cfg


def _base(rows, n, seed, multi_column=False):
    scene = synth.SceneModel(n_objects=12, object_range=(6.0, 20.0), wall_radius=25.0, dropout=0.05)
    st = synth.make_stream(n, seed=seed, sensor=sensor(rows, multi_column), scene=scene, motion=synth.Motion.translate(3.0))
    return synth.Stream(xyz=st.xyz.copy(), intensity=st.intensity.copy(), poses=st.poses.copy(), sensor=st.sensor)


def in_odd_pass(n):
    return (np.arange(n) // RING) % 2 == 1


def stale_stream(rows, seed=1, multi_column=False, passes=PASSES):
    """The stale row has a return in every firing of the even passes over the ring (firing f fills column f, or f + its laser's offset)
    and none in the odd passes."""
    n = RING * passes + 37
    st = _base(rows, n, seed, multi_column)
    r = stale_row(rows)
    odd = in_odd_pass(n)
    # (the scene's drop-outs in the stale row of the even passes: the return of the nearest firing that has one, turned by the pose difference —
    # any finite point in the same column would do)
    missing = np.isnan(st.xyz[:, r, 0]) & ~odd
    have = np.nonzero(~np.isnan(st.xyz[:, r, 0]))[0]
    for f in np.nonzero(missing)[0]:
        g = have[np.argmin(np.abs(have - f))]
        # direction of the row's ray in this firing = the direction of firing g's return turned about z by the firings' azimuth difference
        d_az = -(f - g) * 2 * np.pi / COLS
        c, s = np.cos(d_az), np.sin(d_az)
        x, y, z = st.xyz[g, r]
        st.xyz[f, r] = (c * x - s * y, s * x + c * y, z)
    st.xyz[odd, r] = np.nan
    # A laser's inclination is the same in every firing, so the supplemented inclination of a cell (that of the row below plus the table's last
    # step between the two rows, cc.cpp:364-369) would come out as what the previous tenant had, often to the bit. In the odd passes the row
    # below therefore looks 20 % less steeply down (x and y, and with them the column, stay) — but for EDGE firings at either end of the pass:
    # with per-laser azimuth offsets a column at the boundary would hold the stale row's last return next to an altered one of the row below,
    # and the table would keep that step for the whole pass.
    inner = odd & (np.arange(n) % RING >= EDGE) & (np.arange(n) % RING < RING - EDGE)
    st.xyz[inner, r + 1, 2] *= np.float32(0.8)
    return st


def nan_range_stream(rows, seed=2):
    """stale_stream with returns whose z is NaN (a NaN range, cc_device.h: NAN_RANGE_BITS: x and y keep the return in its column) in every
    pass: in the stale row where it has returns, in the rows around it, and in whole firings."""
    st = stale_stream(rows, seed)
    n = st.n_firings
    rng = np.random.default_rng(seed)
    r = stale_row(rows)
    for f in rng.choice(np.arange(COLS, n - COLS), 60, replace=False):
        for row in (r, r - 1, r + 1, int(rng.integers(0, rows))):
            if not np.isnan(st.xyz[f, row, 0]):
                st.xyz[f, row, 2] = np.nan
    for f in rng.choice(np.arange(COLS, n - COLS), 6, replace=False):
        st.xyz[f, :, 2] = np.nan
    return st


def rollback_firings(n):
    """Firings of rollback_stream that leave the single-column shape: in the middle of calls of 128 and of 97 firings that alternate, and of calls of 128
    firings alone; in odd and even passes."""
    return [f for f in (RING + 301, 2 * RING + 17, 5 * RING + 444, 7 * RING + 95, 8 * RING + 600) if f + 1 < n]


def rollback_stream(rows, seed=3):
    """stale_stream in which a few firings straddle two columns (every other row carries the NEXT firing's return): the block-parallel insertion
    has written the firings behind such a firing when it finds it, and takes them back (par_take_back: the cells return to the cleared state,
    their records stay)."""
    st = stale_stream(rows, seed)
    for f in rollback_firings(st.n_firings):
        st.xyz[f, ::2] = st.xyz[f + 1, ::2]
    return st


def overrun_config(supplement=True):
    """No finished-cluster check for more than ten rotations: nothing is published or cleared (cc.cpp:841-842) and the eleventh rotation runs
    into its own tail (tests/test_gpu_ringwrap.py: test_deliberate_ring_overrun)."""
    cfg = config(supplement)
    cfg.cluster_point_trees_every_nth_column = 100000
    return cfg


def overrun_streams(rows, seed=4):
    """(the stream that overruns the ring, the stream behind the reset). Behind the reset the stale row has no return at all: the table entry
    of that row and of the row above it (sc_inclination_angles_between_lasers_, which reset keeps: cc.cpp:46) stays what the failing call left,
    and the supplemented inclinations of the stale row show it."""
    a = _base(rows, RING + 3 * COLS, seed)
    b = _base(rows, 5 * COLS, seed + 100)
    b.xyz[:, stale_row(rows)] = np.nan
    return a, b
