"""Named parity cases shared by the CPU (oracle / golden) and GPU (engine vs oracle) tests.

Every case is (stream, config, robot_from_sensor or None). Streams are small (seconds for the CPU oracle)."""
from __future__ import annotations

import zlib

import numpy as np

import pose_streams
import profile_streams
import return_streams
from continuous_clustering_amd import capi, synth
from continuous_clustering_amd.synth import Motion, SceneModel, SensorModel


def _kitti(num_columns=2200, **over):
    c = capi.Config.kitti()
    c.num_columns = num_columns
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _vls(num_columns=1700, **over):
    c = capi.Config.vls128()
    c.num_columns = num_columns
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _s64(cols):
    return SensorModel(num_rows=64, num_columns=cols)


def _s128(cols, offsets=True):
    s = SensorModel.s128(offsets)
    s.num_columns = cols
    return s


def jitter_azimuth(stream, seed, amp_columns=0.8):
    """Rotate every firing about the sensor's z axis by a random fraction of a column: firings then repeat columns (cell collisions,
    the shift-to-the-next-column rule cc.cpp:188-202, refusals cc.cpp:204-206), skip columns (empty columns) and step backwards
    (returns behind the first unfinished column, cc.cpp:209-219) — what the evenly stepping synthetic sensor never does."""
    rng = np.random.default_rng(seed)
    w = 2 * np.pi / stream.sensor.num_columns
    a = rng.uniform(-amp_columns, amp_columns, stream.n_firings) * w
    ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
    x, y = stream.xyz[..., 0].astype(np.float64), stream.xyz[..., 1].astype(np.float64)
    xyz = stream.xyz.copy()
    xyz[..., 0] = (ca * x - sa * y).astype(np.float32)
    xyz[..., 1] = (sa * x + ca * y).astype(np.float32)
    return synth.Stream(xyz=xyz, intensity=stream.intensity, poses=stream.poses, sensor=stream.sensor, hit=stream.hit)


ROBOT_TF_TILTED = np.array([0.9961946980917455, 0.0, 0.08715574274765817, 1.2,
                            0.0, 1.0, 0.0, 0.1,
                            -0.08715574274765817, 0.0, 0.9961946980917455, 0.3], dtype=np.float64)


# ---- slope-controlled columns (profile_streams.py): name -> (rows, columns, top / bottom inclination in degrees, config, seed).
# 2 rotations + a quarter: a full rotation, the ring start and several 64-column tiles with a partial last one.
PROFILE_SENSORS = {
    "p_s64_profiles": (64, 360, 2.0, -24.8, _kitti, 301),
    "p_s128_profiles": (128, 340, 15.0, -25.0, _vls, 302),
    "p_s40_profiles": (40, 360, 7.0, -18.0, _kitti, 303),   # rows: a multiple of 8, not of 16
    "p_s50_profiles": (50, 360, 3.0, -25.0, _kitti, 304),   # rows: no multiple of 8
    "p_s16_profiles": (16, 360, 1.0, -29.0, _kitti, 305),
}


def profile_sensor(name):
    rows, cols, top, bottom, _, _ = PROFILE_SENSORS[name]
    return SensorModel(num_rows=rows, num_columns=cols, incl_top_deg=top, incl_bottom_deg=bottom)


def profile_stream(name, seed=None, moving=False):
    """The stream of a p_* case; with another seed: another stream of the same sensor (multi-stream tests); moving: the same returns under a
    pose sequence that drives, yaws, rolls and pitches (the ego-box cases)."""
    rows, cols, _, _, _, seed0 = PROFILE_SENSORS[name]
    n = 2 * cols + cols // 4
    poses = profile_streams.moving_poses(n, 900 + seed0) if moving else None
    return profile_streams.make_profile_stream(profile_sensor(name), n, seed0 if seed is None else seed, poses=poses)


def profile_config(name, **over):
    return PROFILE_SENSORS[name][4](PROFILE_SENSORS[name][1], **over)


# One field or pair per entry, against the base configuration of the case. tests/test_profile_cases_cpu.py shows on the oracle that every entry
# changes at least 100 cells (or the events) of p_s64_profiles; tests/test_gpu_segmentation_sweep.py runs the engine under each of them.
FOG = dict(fog_filtering_enabled=1, fog_filtering_intensity_below=128, fog_filtering_distance_below=12.0, fog_filtering_inclination_above=-0.25)
SEGMENTATION_SWEEP = {
    "use_terrain": dict(use_terrain=1),
    "max_slope_0.05": dict(max_slope=0.05),
    "max_slope_0.21": dict(max_slope=0.21),
    "max_slope_1.0": dict(max_slope=1.0),
    "first_ring_max_0.1": dict(first_ring_as_ground_max_allowed_z_diff=0.1),
    "first_ring_min_-0.1": dict(first_ring_as_ground_min_allowed_z_diff=-0.1),
    "last_ground_slope_0.1": dict(last_ground_point_slope_higher_than=0.1),
    "last_ground_slope_-10": dict(last_ground_point_slope_higher_than=-10.0),
    "last_ground_distance_0.5": dict(last_ground_point_distance_smaller_than=0.5),
    "close_to_ground_z_0.05": dict(ground_because_close_to_last_certain_ground_max_z_diff=0.05),
    "close_to_ground_dist_0.3": dict(ground_because_close_to_last_certain_ground_max_dist_diff=0.3),
    "next_obstacle_dist_0": dict(obstacle_because_next_certain_obstacle_max_dist_diff=0.0),
    "next_obstacle_dist_3.0": dict(obstacle_because_next_certain_obstacle_max_dist_diff=3.0),
    "no_supplement": dict(supplement_inclination_angle_for_nan_cells=0),
    "no_inclination_ignore": dict(ignore_points_with_too_big_inclination_angle_diff=0),
    "chessboard": dict(ignore_points_in_chessboard_pattern=1),
    "max_distance_0.05": dict(max_distance=0.05),
    "max_distance_3.0": dict(max_distance=3.0),
    "fog": FOG,
}
ASSOCIATION_SWEEP = {
    "max_steps_in_column_1": dict(max_steps_in_column=1),
    "max_steps_in_column_3": dict(max_steps_in_column=3),
    "max_steps_in_row_1": dict(max_steps_in_row=1),
    "max_steps_in_row_4": dict(max_steps_in_row=4),
    "min_steps_5": dict(stop_after_association_min_steps=5),
}
# a value from each row of the two tables at once (use_terrain = 1 switches the YELLOW / YELLOWGREEN rules off, so the second entry keeps them)
EVERYTHING = dict(use_terrain=1, max_slope=0.21, first_ring_as_ground_max_allowed_z_diff=0.1, first_ring_as_ground_min_allowed_z_diff=-0.1,
                  last_ground_point_slope_higher_than=0.1, last_ground_point_distance_smaller_than=0.5,
                  ground_because_close_to_last_certain_ground_max_z_diff=0.05, ground_because_close_to_last_certain_ground_max_dist_diff=0.3,
                  obstacle_because_next_certain_obstacle_max_dist_diff=3.0, supplement_inclination_angle_for_nan_cells=0,
                  ignore_points_with_too_big_inclination_angle_diff=0, ignore_points_in_chessboard_pattern=1, max_distance=3.0,
                  max_steps_in_column=3, max_steps_in_row=4, stop_after_association_min_steps=5, **FOG)
EVERYTHING_NO_TERRAIN = dict(EVERYTHING, use_terrain=0)
SWEEP_BASE_CASE = "p_s64_profiles"


def sweep_overrides(entry):
    if entry == "base":
        return {}
    if entry == "everything":
        return EVERYTHING
    if entry == "everything_no_terrain":
        return EVERYTHING_NO_TERRAIN
    return SEGMENTATION_SWEEP[entry] if entry in SEGMENTATION_SWEEP else ASSOCIATION_SWEEP[entry]


# ---- ego box: robot_from_sensor and box settings for p_s64_profiles under the moving pose sequence. (name -> (robot_from_sensor, overrides))
ROBOT_TF_AHEAD_ABOVE = np.array([1.0, 0.0, 0.0, 6.0,
                                 0.0, 1.0, 0.0, 0.0,
                                 0.0, 0.0, 1.0, 2.0], dtype=np.float64)
ROBOT_TF_1M_UP = np.array([1.0, 0.0, 0.0, 0.0,
                           0.0, 1.0, 0.0, 0.0,
                           0.0, 0.0, 1.0, 1.0], dtype=np.float64)
EGO_SETTINGS = {
    "tilted_tf": (ROBOT_TF_TILTED, {}),
    "sensor_ahead_above": (ROBOT_TF_AHEAD_ABOVE, dict(height_ref_to_ground_=0.3, height_ref_to_maximum_=2.5, length_ref_to_front_end_=9.0)),
    "asymmetric_box": (None, dict(length_ref_to_front_end_=12.0, length_ref_to_rear_end_=-0.5, width_ref_to_left_mirror_=0.3, width_ref_to_right_mirror_=-4.0)),
    "box_without_sensor": (None, dict(length_ref_to_front_end_=9.0, length_ref_to_rear_end_=1.5, width_ref_to_left_mirror_=5.0, width_ref_to_right_mirror_=0.5)),
    "empty_box": (None, dict(length_ref_to_front_end_=-1.0, length_ref_to_rear_end_=1.0)),
    "huge_box": (None, dict(length_ref_to_front_end_=200.0, length_ref_to_rear_end_=-200.0, width_ref_to_left_mirror_=200.0,
                            width_ref_to_right_mirror_=-200.0, height_ref_to_maximum_=200.0, height_ref_to_ground_=-200.0)),
    # returns above the box exist only where the sensor sits low in it: mounted 1 m above the robot's origin the plain box ends 0.5 m below the
    # sensor (walls next to the sensor rise above that), the box with height_ref_to_maximum_ = 5 takes them in
    "sensor_1m_up": (ROBOT_TF_1M_UP, dict(height_ref_to_ground_=-0.7)),
    "height_max_5": (ROBOT_TF_1M_UP, dict(height_ref_to_ground_=-0.7, height_ref_to_maximum_=5.0)),
}


def ego_case(setting):
    tf, over = EGO_SETTINGS[setting]
    return profile_stream(SWEEP_BASE_CASE, moving=True), profile_config(SWEEP_BASE_CASE, **over), tf


def build_case(name: str):
    if name.startswith("o_"):
        return pose_case(name)
    if name.startswith("r_"):
        return return_case(name)[:3]
    if name in PROFILE_SENSORS:
        return profile_stream(name), profile_config(name), None
    if name == "p_s64_profiles_moving":
        return profile_stream(SWEEP_BASE_CASE, moving=True), profile_config(SWEEP_BASE_CASE), None
    if name == "p_s64_alternating":
        # ground / obstacle changes on every second valid row: the input on which k_seg_small's fixed point over the labels needs many rounds.
        # The risers are 3 - 10 cm apart from the treads below them, so the two distance rules that would merge them are tightened: an obstacle only
        # pulls ground within 2 cm with it, and "close to the last certain ground" reaches 5 cm.
        cfg = _kitti(360, obstacle_because_next_certain_obstacle_max_dist_diff=0.02, ground_because_close_to_last_certain_ground_max_dist_diff=0.05)
        return profile_streams.make_alternating_stream(_s64(360), 120, 311), cfg, None
    if name == "p_s64_terrain_gaps":
        # use_terrain = 1 on smooth ground with many missing rows: the rule that a ground point more than 5 m beyond the previous one is an obstacle
        # (cc.cpp: the terrain branch of "flat w.r.t. the previous point") decides the first obstacle of most columns
        mix = profile_streams.Mixture(flat=0.55, edge=0.0, mild=0.05, steep=0.0, wall=0.0, step=0.0, missing=0.40, near_start=0.0,
                                      first_weights=(0.3, 0.3, 0.0, 0.0, 0.2, 0.2))
        return profile_streams.make_profile_stream(_s64(360), 810, 313, mix=mix), _kitti(360, use_terrain=1), None
    if name == "p_s64_label_chains":
        # one-row walls and flat rows in turn, thresholds from the sweep table: the labels form a dependency chain over the whole column, so that an
        # iteration over the labels (k_seg_small) needs about rows / 2 rounds (tests/test_profile_cases_cpu.py counts them)
        sen = SensorModel(num_rows=64, num_columns=360, incl_top_deg=-12.0, incl_bottom_deg=-30.0)
        cfg = _kitti(360, max_slope=1.0, ground_because_close_to_last_certain_ground_max_z_diff=0.03)
        return profile_streams.make_chain_stream(sen, 120, 312), cfg, None
    if name == "s64_static":
        return synth.make_stream(720 * 3, seed=1234, sensor=_s64(720)), _kitti(720), None
    if name == "s64_translate":
        return synth.make_stream(720 * 3, seed=7, sensor=_s64(720), motion=Motion.translate()), _kitti(720), None
    if name == "s64_turn":
        return synth.make_stream(720 * 3, seed=8, sensor=_s64(720), motion=Motion.turn(10.0, 0.6)), _kitti(720), None
    if name == "s64_full_2200":
        return synth.make_stream(2200 * 2 + 300, seed=21, motion=Motion.translate()), _kitti(2200), None
    if name == "s64_forced_finish_ring":
        # unbroken wall ring: clusters exceed one rotation -> tree-width refusals, finished-root refusals, forced finish
        sc = SceneModel(n_objects=0, wall_radius=12.0, wall_gaps_deg=())
        return synth.make_stream(360 * 4, seed=5, sensor=_s64(360), scene=sc), _kitti(360), None
    if name == "s64_ring_with_objects":
        sc = SceneModel(n_objects=25, wall_radius=14.0, wall_gaps_deg=(), object_range=(3.0, 11.0))
        return synth.make_stream(360 * 4, seed=6, sensor=_s64(360), scene=sc, motion=Motion.translate(3.0)), _kitti(360), None
    if name == "s64_fog_and_ego":
        sc = SceneModel(n_objects=40, object_range=(1.5, 12.0), object_radius=(0.2, 0.6))
        cfg = _kitti(720, fog_filtering_enabled=1, fog_filtering_intensity_below=40, fog_filtering_distance_below=18.0,
                     fog_filtering_inclination_above=-0.2)
        return synth.make_stream(720 * 2 + 50, seed=9, sensor=_s64(720), scene=sc), cfg, None
    if name == "s64_counterclockwise":
        sen = _s64(720)
        sen.clockwise = False
        return synth.make_stream(720 * 2 + 50, seed=10, sensor=sen), _kitti(720, sensor_is_clockwise=0), None
    if name == "s64_every_2nd_column":
        return synth.make_stream(720 * 2 + 50, seed=11, sensor=_s64(720)), _kitti(720, cluster_point_trees_every_nth_column=2), None
    if name == "s64_no_early_stop":
        # stop_after_association disabled: many links per point -> exercises the exact serial association path
        return synth.make_stream(360 * 2 + 50, seed=12, sensor=_s64(360)), _kitti(360, stop_after_association_enabled=0), None
    if name == "s64_wide_window_global_kernel":
        # max_steps_in_row beyond the LDS window of k_assoc_lds: every stream runs the global-memory association kernel
        return synth.make_stream(720 * 2 + 50, seed=22, sensor=_s64(720)), _kitti(720, max_steps_in_row=31), None
    if name == "s64_min_steps_3":
        return synth.make_stream(720 * 2 + 50, seed=13, sensor=_s64(720)), _kitti(720, stop_after_association_min_steps=3), None
    if name == "s64_dropouts":
        sc = SceneModel(dropout=0.35, max_range=40.0)
        return synth.make_stream(720 * 2 + 50, seed=14, sensor=_s64(720), scene=sc, motion=Motion.translate()), _kitti(720), None
    if name == "s64_no_supplement_no_incl_ignore":
        cfg = _kitti(720, supplement_inclination_angle_for_nan_cells=0, ignore_points_with_too_big_inclination_angle_diff=0)
        return synth.make_stream(720 * 2 + 50, seed=15, sensor=_s64(720), scene=SceneModel(dropout=0.2)), cfg, None
    if name == "s64_robot_tf_tilted":
        cfg = _kitti(720)
        return synth.make_stream(720 * 2 + 50, seed=16, sensor=_s64(720), motion=Motion.turn(8.0, 0.3)), cfg, ROBOT_TF_TILTED
    if name == "s64_deep_lookback":
        # everything "flat" and every ground cell below a new obstacle "close": the downward fix-up of cc.cpp:513-535 relabels runs of up to
        # 62 rows, far beyond the 16 rows k_seg_scan keeps in LDS (it reads the rest from the staging plane)
        cfg = _kitti(360, max_slope=5.0, obstacle_because_next_certain_obstacle_max_dist_diff=1.0e6)
        sc = SceneModel(n_objects=30, object_range=(3.0, 15.0))
        return synth.make_stream(360 * 2 + 50, seed=31, sensor=_s64(360), scene=sc), cfg, None
    if name == "s128_offsets":
        return synth.make_stream(680 * 3, seed=17, sensor=_s128(680), start_column=20), _vls(680), None
    if name == "s128_no_offsets_translate":
        return synth.make_stream(680 * 3, seed=18, sensor=_s128(680, False), motion=Motion.translate()), _vls(680), None
    if name == "s128_full_1700":
        return synth.make_stream(1700 * 2 + 200, seed=19, sensor=SensorModel.s128(), start_column=40,
                                 motion=Motion.translate()), _vls(1700), None
    if name == "s96_offsets":
        # 96 rows: two rows per lane with a half-filled second register (lanes 32 - 63 own no second row), per-laser azimuth offsets
        sen = SensorModel(num_rows=96, num_columns=600, incl_top_deg=12.0, incl_bottom_deg=-25.0, azimuth_offsets_deg=(-3.1, -1.0, 1.0, 3.1))
        return synth.make_stream(600 * 3 + 40, seed=23, sensor=sen, start_column=15, motion=Motion.translate()), _vls(600), None
    if name == "s32_small_sensor":
        sen = SensorModel(num_rows=32, num_columns=512, incl_top_deg=10.0, incl_bottom_deg=-30.0)
        return synth.make_stream(512 * 3, seed=20, sensor=sen), _vls(512, max_distance=0.5), None
    # ---- jittered firing azimuths: collisions, shifts, refusals, skipped and revisited columns in the insertion
    if name == "j_s64_jitter":
        st = synth.make_stream(720 * 2 + 50, seed=51, sensor=_s64(720), motion=Motion.translate())
        return jitter_azimuth(st, 151, 0.8), _kitti(720), None
    if name == "j_s64_jitter_wide":
        st = synth.make_stream(360 * 3, seed=52, sensor=_s64(360), motion=Motion.turn(8.0, 0.4), scene=SceneModel(dropout=0.15))
        return jitter_azimuth(st, 152, 2.5), _kitti(360), ROBOT_TF_TILTED
    if name == "j_s128_offsets_jitter":
        st = synth.make_stream(680 * 2, seed=53, sensor=_s128(680), start_column=20, motion=Motion.translate())
        return jitter_azimuth(st, 153, 1.2), _vls(680), None
    # ---- ring-wrap cases: >= 12 rotations through the 10-rotation ring (cc.cpp:17), small columns-per-rotation so the oracle stays fast
    if name == "w_s64_240x13":
        sc = SceneModel(n_objects=40, object_range=(4.0, 30.0))
        return synth.make_stream(240 * 13, seed=41, sensor=_s64(240), scene=sc, motion=Motion.translate()), _kitti(240), None
    if name == "w_s64_360x12_turn":
        return synth.make_stream(360 * 12 + 100, seed=42, sensor=_s64(360), motion=Motion.turn(8.0, 0.5)), _kitti(360), ROBOT_TF_TILTED
    if name == "w_s64_ring_wall_240x12":
        # unbroken wall ring + objects: forced finishes (cluster wider than a rotation) on every rotation, across the ring wrap
        sc = SceneModel(n_objects=25, wall_radius=14.0, wall_gaps_deg=(), object_range=(3.0, 11.0))
        return synth.make_stream(240 * 12 + 60, seed=43, sensor=_s64(240), scene=sc, motion=Motion.translate(3.0)), _kitti(240), None
    if name == "w_s128_offsets_340x12":
        return synth.make_stream(340 * 12 + 80, seed=44, sensor=_s128(340), start_column=12, motion=Motion.translate()), _vls(340), None
    if name == "w_s32_256x12":
        sen = SensorModel(num_rows=32, num_columns=256, incl_top_deg=10.0, incl_bottom_deg=-30.0)
        return synth.make_stream(256 * 12 + 40, seed=45, sensor=sen, motion=Motion.translate()), _vls(256, max_distance=0.5), None
    # ---- gaps in slanted surfaces: a tree that has gone quiet for about as many columns as its points' max angle difference reaches is met
    # again by a later, nearer point (large cylinders seen off-centre: the range changes quickly with the azimuth; every few dozen columns the
    # obstacle returns of 4 - 15 consecutive firings are dropped). The reference then refuses attaches to trees whose cluster finished meanwhile
    # (cc.cpp:658) or keeps a cluster alive through a link: the exceptions the batch-parallel association kernel has to detect
    if name in ("x_s64_slanted_gaps", "x_s64_slanted_gaps_far"):
        far = name.endswith("far")
        sc = SceneModel(n_objects=14, object_range=(14.0, 40.0) if far else (7.0, 24.0), object_radius=(3.0, 11.0), object_top_z=2.5,
                        wall_radius=30.0 if far else 0.0, wall_gaps_deg=((10.0, 50.0), (200.0, 260.0)), dropout=0.05)
        st = synth.make_stream(720 * 3, seed=61 if far else 62, sensor=_s64(720), scene=sc, motion=Motion.translate(6.0))
        xyz = st.xyz.copy()
        rng = np.random.default_rng(161)
        k = 0
        while k < st.n_firings:
            k += int(rng.integers(9, 40))
            g = int(rng.integers(3, 16))
            sel = st.hit[k:k + g] > 1  # obstacle returns only: the ground keeps the columns (and the insertion) regular
            xyz[k:k + g][sel] = np.nan
            k += g
        return synth.Stream(xyz=xyz, intensity=st.intensity, poses=st.poses, sensor=st.sensor, hit=st.hit), _kitti(720), None
    if name == "x_s64_refused_attach":
        # Hand-made: the attach the reference REFUSES because the candidate's tree belongs to a finished cluster (cc.cpp:658). A tree lives until a
        # column's smallest AZIMUTH passes its largest (azimuth + max angle difference); a later point accepts a candidate when their 3-D distance is
        # below max_distance. For steep lasers the 3-D angle is smaller than the azimuth difference (cos(inclination) < 1), so a post seen by the rows
        # at -21..-23 degrees at 3 m is still within 0.5 m of an equal post 20 columns later although its tree was finished a column earlier — provided
        # the first post sits at the very start of its column and the second one too. 720 columns, static sensor, unbroken wall (every row returns).
        sen = _s64(720)
        sc = SceneModel(n_objects=0, wall_radius=40.0, wall_gaps_deg=(), range_noise=0.0, dropout=0.0)
        st = synth.make_stream(720 * 2 + 100, seed=81, sensor=sen, scene=sc)
        xyz = st.xyz.astype(np.float64)
        w = 2 * np.pi / 720
        incl = np.deg2rad(np.linspace(sen.incl_top_deg, sen.incl_bottom_deg, 64))
        frac = np.full(st.n_firings, 0.5)
        posts = []
        k = 60
        gaps = [20, 20, 19, 20, 18, 20, 20, 17, 20, 20, 20, 16, 20, 20]
        i = 0
        while k + 25 < st.n_firings:
            gap = gaps[i % len(gaps)]
            posts.append((k, k + gap))
            frac[k] = 0.02
            frac[k + 1:k + gap] = 0.5
            frac[k + gap] = 0.01
            k += gap + 31 + (i % 5)
            i += 1
        # rotate every firing about z so that it sits at (k + frac) * w instead of (k + 0.5) * w (clockwise sensor: azimuth = pi - that)
        rot = -(frac - 0.5) * w
        ca, sa = np.cos(rot)[:, None], np.sin(rot)[:, None]
        x, y = xyz[..., 0].copy(), xyz[..., 1].copy()
        xyz[..., 0] = ca * x - sa * y
        xyz[..., 1] = sa * x + ca * y
        rows = np.arange(54, 59)
        for a, b in posts:
            for kk in (a, b):
                az = np.pi - (kk + frac[kk]) * w
                rng_ = 3.0
                xyz[kk, rows, 0] = rng_ * np.cos(incl[rows]) * np.cos(az)
                xyz[kk, rows, 1] = rng_ * np.cos(incl[rows]) * np.sin(az)
                xyz[kk, rows, 2] = rng_ * np.sin(incl[rows])
        return synth.Stream(xyz=xyz.astype(np.float32), intensity=st.intensity, poses=st.poses, sensor=sen, hit=st.hit), _kitti(720), None
    if name.startswith("x_s64_near_jitter_gaps"):
        # The same close to the sensor with jittered firing azimuths: a point reaches back ceil(max angle difference / column width) columns, a
        # tree lives until a column's smallest azimuth passes its largest azimuth + max angle difference — with every firing at its own fraction
        # of a column and a nearer point looking back at a farther one the two can disagree by a column (only below ~6 m at 720 columns).
        seed = int(name.rsplit("_", 1)[1]) if name[-1].isdigit() else 0
        sc = SceneModel(n_objects=26, object_range=(2.2, 6.5), object_radius=(0.4, 3.0), object_top_z=1.5, wall_radius=0.0, dropout=0.04)
        st = synth.make_stream(720 * 3, seed=70 + seed, sensor=_s64(720), scene=sc, motion=Motion.translate(4.0))
        xyz = st.xyz.copy()
        rng = np.random.default_rng(170 + seed)
        k = 0
        while k < st.n_firings:
            k += int(rng.integers(6, 30))
            g = int(rng.integers(2, 19))
            sel = st.hit[k:k + g] > 1
            xyz[k:k + g][sel] = np.nan
            k += g
        st = synth.Stream(xyz=xyz, intensity=st.intensity, poses=st.poses, sensor=st.sensor, hit=st.hit)
        return jitter_azimuth(st, 270 + seed, 0.9), _kitti(720), None
    # ---- vegetation-like scenes: what leaves the batch-parallel association's fast path on natural data --------------------------------
    if name == "c_s64_sparse_clutter":
        # isolated returns at 3 .. 30 m all around: more unfinished trees side by side than the kernel has lanes for (AB_BAIL_TREES)
        return synth.make_stream(2200 * 2 + 300, seed=77, sensor=_s64(2200), scene=SceneModel.sparse_clutter(0.1), motion=Motion.translate()), _kitti(2200), None
    if name == "c_s64_near_clutter":
        # a shell of returns at 2 .. 8 m all around: a tree that may reach the one-rotation limits (AB_BAIL_ROTATION)
        return synth.make_stream(2200 * 2 + 300, seed=77, sensor=_s64(2200), scene=SceneModel.near_clutter(0.1), motion=Motion.translate()), _kitti(2200), None
    if name == "c_s64_mixed_clutter":
        return synth.make_stream(2200 * 2 + 300, seed=78, sensor=_s64(2200), scene=SceneModel.cluttered(0.1), motion=Motion.turn(8.0, 0.15)), _kitti(2200), None
    if name == "c_s128_sparse_clutter":
        return synth.make_stream(1700 + 600, seed=79, sensor=_s128(1700), scene=SceneModel.sparse_clutter(0.08), motion=Motion.translate()), _vls(1700), None
    # ---- small variants kept as committed golden fixtures -------------------------------------------------------
    if name == "g_s64_translate":
        return synth.make_stream(800, seed=31, sensor=_s64(360), motion=Motion.translate()), _kitti(360), None
    if name == "g_s64_forced_finish_ring":
        sc = SceneModel(n_objects=0, wall_radius=12.0, wall_gaps_deg=())
        return synth.make_stream(240 * 4, seed=32, sensor=_s64(240), scene=sc), _kitti(240), None
    if name == "g_s128_offsets":
        return synth.make_stream(816, seed=33, sensor=_s128(340), start_column=12, motion=Motion.turn(6.0, 0.4)), _vls(340), None
    if name == "g_s64_fog_and_ego":
        sc = SceneModel(n_objects=40, object_range=(1.5, 12.0), object_radius=(0.2, 0.6), dropout=0.1)
        cfg = _kitti(360, fog_filtering_enabled=1, fog_filtering_intensity_below=40, fog_filtering_distance_below=18.0,
                     fog_filtering_inclination_above=-0.2)
        return synth.make_stream(800, seed=34, sensor=_s64(360), scene=sc), cfg, ROBOT_TF_TILTED
    raise KeyError(name)


ALL_CASES = ["s64_static", "s64_translate", "s64_turn", "s64_full_2200", "s64_forced_finish_ring", "s64_ring_with_objects",
             "s64_fog_and_ego", "s64_counterclockwise", "s64_every_2nd_column", "s64_no_early_stop", "s64_min_steps_3",
             "s64_wide_window_global_kernel", "s64_dropouts", "s64_no_supplement_no_incl_ignore", "s64_robot_tf_tilted", "s128_offsets",
             "s128_no_offsets_translate", "s128_full_1700", "s96_offsets", "s32_small_sensor", "j_s64_jitter", "j_s64_jitter_wide", "j_s128_offsets_jitter"]

EXCEPTION_CASES = ["x_s64_slanted_gaps", "x_s64_slanted_gaps_far", "x_s64_near_jitter_gaps_3", "x_s64_refused_attach"]

CLUTTER_CASES = ["c_s64_sparse_clutter", "c_s64_near_clutter", "c_s64_mixed_clutter", "c_s128_sparse_clutter"]

RING_WRAP_CASES = ["w_s64_240x13", "w_s64_360x12_turn", "w_s64_ring_wall_240x12", "w_s128_offsets_340x12", "w_s32_256x12"]

PROFILE_CASES = list(PROFILE_SENSORS)
FIXED_POINT_CASES = ["p_s64_alternating", "p_s64_label_chains"]

# cases stored as golden fixtures under tests/golden/ (inputs + expected outputs)
GOLDEN_CASES = ["g_s64_translate", "g_s64_forced_finish_ring", "g_s128_offsets", "g_s64_fog_and_ego"]


# ---- odometry poses far from the origin, not rigid, not finite (pose_streams.py): o_<what>__<parent or variant>[__<box>] ------------------------
# tests/test_pose_cases_cpu.py measures on the oracle what each of them does; tests/test_gpu_pose_parity.py runs the engine on them.
FAR_PARENTS = ["p_s64_profiles_moving", "p_s128_profiles_moving", "p_s40_profiles", "s64_turn"]                      # under every FAR_OFFSETS entry
# ... and under one offset. Two of them are not the cases of the same name under the UTM offset (tests/test_pose_cases_cpu.py has the figures):
# p_s64_alternating's 120 firings look along -x, where UTM coordinates are quantised to 3 cm only, and keep their (x, y) apart (6 identical pairs),
# so it takes the 2^24 offset (1 m); x_s64_refused_attach's wall has no range noise and stands exactly upright, so 14890 vertical pairs share
# (x, y) before any offset — its wall returns get 0.2 permille of range noise first (x_s64_refused_attach_rough_wall; the posts stay as they are).
FAR_SINGLE = {"p_s64_alternating": "2p24", "p_s64_label_chains": "utm", "s64_forced_finish_ring": "utm", "x_s64_refused_attach_rough_wall": "utm"}
FAR_FIXED_POINT_CASES = ["o_2p24__p_s64_alternating", "o_utm__p_s64_label_chains"]
FAR_CASES = [f"o_{off}__{parent}" for parent in FAR_PARENTS for off in pose_streams.FAR_OFFSETS] + [f"o_{off}__{parent}" for parent, off in FAR_SINGLE.items()]

CORNER_BOXES = ["default", "sensor_ahead_above", "tilted_tf", "asymmetric_box"]
CORNER_CASES = [f"o_corner__{variant}__{box}" for variant in pose_streams.POSE_VARIANTS for box in CORNER_BOXES]

NON_FINITE_PARENTS = ["s64_turn", "p_s64_profiles_moving"]
NON_FINITE_CASES = [f"o_{value}_{place}__{parent}" for parent in NON_FINITE_PARENTS for value in ("nan", "inf") for place in pose_streams.NON_FINITE_PLACES]


def pose_parent(name):
    """The case an o_* case was made from."""
    if name == "p_s128_profiles_moving":
        return profile_stream("p_s128_profiles", moving=True), profile_config("p_s128_profiles"), None
    if name == "x_s64_refused_attach_rough_wall":
        stream, cfg, tf = build_case("x_s64_refused_attach")
        xyz = stream.xyz.astype(np.float64)
        wall = np.sqrt((xyz ** 2).sum(-1)) > 30.0
        factor = 1.0 + np.random.default_rng(481).uniform(-2e-4, 2e-4, wall.shape)
        xyz[wall] *= factor[wall][:, None]
        return synth.Stream(xyz=xyz.astype(np.float32), intensity=stream.intensity, poses=stream.poses, sensor=stream.sensor, hit=stream.hit), cfg, tf
    return build_case(name)


def corner_case(variant, box, eps=None, seed=331):
    """(stream, config, robot_from_sensor, planted): three rotations of 64 x 360 profile columns under the constant pose POSE_VARIANTS[variant], with
    48 returns planted just inside and just outside the corners of the ego box `box` (pose_streams.plant_box_corners). The margin is 2 permille of the
    box's half extents; 3 percent for the asymmetric box at UTM coordinates, where with 2 permille the float32 rounding (0.5 m in y) happens to throw
    every corner of the utm and utm_f32_rotation poses out of the box and the case would hold no EGO return at all."""
    if eps is None:
        eps = 3e-2 if box == "asymmetric_box" and variant in pose_streams.UTM_VARIANTS else 2e-3
    tf, over = (None, {}) if box == "default" else EGO_SETTINGS[box]
    cfg = profile_config(SWEEP_BASE_CASE, **over)
    base = profile_streams.make_profile_stream(profile_sensor(SWEEP_BASE_CASE), 3 * 360, seed)
    stream, planted = pose_streams.plant_box_corners(base, pose_streams.POSE_VARIANTS[variant], tf, cfg, eps)
    return stream, cfg, tf, planted


def pose_case(name):
    what, _, rest = name[2:].partition("__")
    if what == "corner":
        variant, _, box = rest.partition("__")
        return corner_case(variant, box)[:3]
    stream, cfg, tf = pose_parent(rest)
    if what in pose_streams.FAR_OFFSETS:
        return pose_streams.with_offset(stream, pose_streams.FAR_OFFSETS[what]), cfg, tf
    value, _, place = what.partition("_")
    return pose_streams.with_non_finite(stream, {"nan": np.nan, "inf": np.inf}[value], place), cfg, tf


# ---- degenerate and extreme returns (return_streams.py): r_<class>__<parent> ---------------------------------------------------------------------
# tests/test_return_cases_cpu.py measures on the oracle what each of them does; tests/test_gpu_return_parity.py runs the engine on them.
RETURN_BASE_CASE = "p_s64_profiles"
RETURN_MIXED_PARENT = "w_s64_240x13"
RETURN_S64_CASES = [f"r_{cls}__{RETURN_BASE_CASE}" for cls in return_streams.ALL_CLASSES]
RETURN_CCW_CASES = [f"r_{cls}__{RETURN_BASE_CASE}_ccw" for cls in return_streams.ZERO_CLASSES]       # the zeros under the other sensor direction
# a thinner set on two rows per lane and on rows off the chunk size: one class of every group
RETURN_THIN_CLASSES = ["zero", "yneg0_xneg", "edge_hi_exact", "edge_straddle", "scaled_1e-42", "scaled_1e36", "all_inf", "z_nan", "y_nan", "dup_firings",
                       "gap_half_plus", "one_mid"]
RETURN_S128_CASES = [f"r_{cls}__p_s128_profiles" for cls in RETURN_THIN_CLASSES]
RETURN_S40_CASES = [f"r_{cls}__p_s40_profiles" for cls in RETURN_THIN_CLASSES]
RETURN_RING_CASES = [f"r_{cls}__s64_forced_finish_ring" for cls in return_streams.CLUSTER_CLASSES + ("z_nan",)]
# the infinities under the moving pose: no entry of its rotation block is zero, so inf stays inf (0 * inf = NaN under the static identity pose)
RETURN_MOVING_CASES = [f"r_{cls}__p_s64_profiles_moving" for cls in return_streams.INF_CLASSES]
RETURN_MIXED_CASE = f"r_mixed__{RETURN_MIXED_PARENT}"
RETURN_CASES = (RETURN_S64_CASES + RETURN_CCW_CASES + RETURN_S128_CASES + RETURN_S40_CASES + RETURN_RING_CASES + RETURN_MOVING_CASES +
                [RETURN_MIXED_CASE])


def return_parent(name):
    """The case an r_* case was made from."""
    if name == RETURN_BASE_CASE + "_ccw":
        rows, cols, top, bottom, _, seed = PROFILE_SENSORS[RETURN_BASE_CASE]
        sen = SensorModel(num_rows=rows, num_columns=cols, incl_top_deg=top, incl_bottom_deg=bottom, clockwise=False)
        return profile_streams.make_profile_stream(sen, 2 * cols + cols // 4, seed), profile_config(RETURN_BASE_CASE, sensor_is_clockwise=0), None
    return build_case(name)


def return_seed(name):
    return zlib.crc32(name.encode()) % 100000


def return_case(name):
    """(stream, config, robot_from_sensor, planted mask [firings, rows]) of an r_* case."""
    cls, _, parent = name[2:].partition("__")
    stream, cfg, tf = return_parent(parent)
    if cls == "mixed":
        stream, mask, _ = return_streams.plant_mixed(stream, return_seed(name))
    else:
        stream, mask = return_streams.plant(stream, cls, return_seed(name))
    return stream, cfg, tf, mask
