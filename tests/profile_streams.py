"""Slope-controlled columns: seeded streams whose every firing is a terrain PROFILE walked from the bottom laser to the top one.

The flat-ground scenes of continuous_clustering_amd/synth.py leave most rules of the ground segmentation (cc.cpp:294-624) idle: a column there is
ground, at most one object, ground again. Here every return lies on its laser's ray (inclinations linspace(top, bottom, rows), azimuth
pi - (k + 0.5) * width for firing k of a clockwise sensor), and the surface the rays hit is drawn row by row: with the previous surface point
(rho_p, z_p) in the firing's azimuth plane and a slope s the ray of inclination a meets the line through that point at the range
    t = (z_p - s * rho_p) / (sin a - s * cos a);
a t outside (0.6 m, 150 m) is no return. The slopes come from a mixture whose parts sit where the segmentation's thresholds are: flat, just
either side of max_slope, mild, steep faces, near-vertical walls, downward steps, missing returns. The bottom row starts on ground whose height
above the reference plane straddles the first-ring thresholds (or, in a minority of profiles, on something near the sensor: the ego box). A
profile persists over a run of 1 .. 30 firings with a little slope noise per firing, so that obstacles form clusters.

Everything is numpy and deterministic per seed."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from continuous_clustering_amd import synth

T_MIN, T_MAX = 0.6, 150.0

# kinds of a row's slope draw
FLAT, EDGE, MILD, STEEP, WALL, STEP, MISSING = range(7)


@dataclass
class Mixture:
    """Probabilities of the row kinds (normalised) and what the bottom row starts on."""
    flat: float = 0.30
    edge: float = 0.22
    mild: float = 0.14
    steep: float = 0.09
    wall: float = 0.08
    step: float = 0.07
    missing: float = 0.10
    max_slope: float = 0.2                                   # the EDGE kind sits at +-(max_slope +- 0.02)
    ground_height: float = -1.7                              # height_ref_to_ground_ below a sensor mounted at the robot's origin
    first_heights: tuple = (0.38, -0.38, 0.42, -0.42, 0.05, -0.05)  # of the bottom row above ground_height: either side of +-0.4, and inside
    first_weights: tuple = (0.15, 0.15, 0.25, 0.25, 0.1, 0.1)        # half of the first rings ground, half obstacle
    near_start: float = 0.08                                 # share of profiles whose bottom row returns from 0.8 .. 3 m instead (ego box, ORANGE)
    run: tuple = (1, 30)                                     # firings a drawn profile persists
    slope_noise: float = 0.004                               # per firing, on every slope of the run's profile

    def probabilities(self):
        p = np.array([self.flat, self.edge, self.mild, self.steep, self.wall, self.step, self.missing], dtype=np.float64)
        return p / p.sum()


def inclinations(sensor) -> np.ndarray:
    return np.deg2rad(np.linspace(sensor.incl_top_deg, sensor.incl_bottom_deg, sensor.num_rows))


def firing_azimuths(sensor, n_firings: int) -> np.ndarray:
    w = 2 * math.pi / sensor.num_columns
    k = np.arange(n_firings, dtype=np.float64)
    return (math.pi - (k + 0.5) * w) if sensor.clockwise else (-math.pi + (k + 0.5) * w)


def _draw_profile(rng, rows: int, mix: Mixture):
    kind = rng.choice(7, size=rows, p=mix.probabilities())
    s = np.zeros(rows)
    drop = np.zeros(rows)
    n = rows
    s = np.where(kind == FLAT, rng.normal(0.0, 0.03, n), s)
    edge = rng.choice([-1.0, 1.0], n) * (mix.max_slope + rng.choice([-1.0, 1.0], n) * rng.uniform(0.002, 0.02, n))
    s = np.where(kind == EDGE, edge, s)
    s = np.where(kind == MILD, rng.normal(0.0, 0.15, n), s)
    s = np.where(kind == STEEP, rng.choice([-1.0, 1.0], n, p=[0.25, 0.75]) * rng.uniform(0.4, 2.5, n), s)
    s = np.where(kind == WALL, rng.uniform(6.0, 60.0, n), s)
    s = np.where(kind == STEP, rng.normal(0.0, 0.03, n), s)
    drop = np.where(kind == STEP, rng.uniform(0.15, 1.2, n), 0.0)
    if rng.random() < mix.near_start:
        start = ("range", float(rng.uniform(0.8, 3.0)))
    else:
        start = ("height", float(rng.choice(mix.first_heights, p=mix.first_weights)) + float(rng.normal(0.0, 0.004)))
    return kind, s, drop, start


def walk_profile(incl: np.ndarray, kind, slope, drop, start, mix: Mixture) -> np.ndarray:
    """Ranges [rows] (NaN = no return) of one firing: bottom row (last index) to top row."""
    rows = incl.shape[0]
    t = np.full(rows, np.nan)
    rho_p = z_p = None
    for r in range(rows - 1, -1, -1):
        a = incl[r]
        sa, ca = math.sin(a), math.cos(a)
        if rho_p is None:
            if start[0] == "range":
                tr = start[1]
            else:
                z0 = mix.ground_height + start[1]
                tr = z0 / sa if sa < 0 else math.inf
        elif kind[r] == MISSING:
            continue
        else:
            den = sa - slope[r] * ca
            tr = ((z_p - drop[r]) - slope[r] * rho_p) / den if den != 0.0 else math.inf
        if not (T_MIN < tr < T_MAX):
            if rho_p is None:
                return t  # (a sensor whose bottom laser does not reach the ground: nothing to walk from)
            continue
        t[r] = tr
        rho_p, z_p = tr * ca, tr * sa
    return t


def points_on_rays(incl: np.ndarray, az: np.ndarray, t: np.ndarray) -> np.ndarray:
    """xyz [F, rows, 3] (float64) of the ranges t [F, rows] along the rays (inclination per row, azimuth per firing)."""
    ce, se = np.cos(incl)[None, :], np.sin(incl)[None, :]
    return np.stack([t * ce * np.cos(az)[:, None], t * ce * np.sin(az)[:, None], t * se], -1)


def moving_poses(n_firings: int, seed: int) -> np.ndarray:
    """odom_from_sensor of a vehicle that drives, yaws and sways: yaw rate ~0.5 rad/s at 10 m/s, roll and pitch of a few degrees."""
    rng = np.random.default_rng(seed)
    tsec = np.arange(n_firings, dtype=np.float64) / 8000.0  # (a few hundred columns per rotation: a slow sensor, so that the pose moves per column)
    yaw = 0.5 * tsec + 0.05 * np.sin(7.0 * tsec)
    roll = np.deg2rad(3.0) * np.sin(5.0 * tsec + rng.uniform(0, 6.28))
    pitch = np.deg2rad(2.5) * np.sin(3.0 * tsec + rng.uniform(0, 6.28))
    px = 10.0 * np.sin(0.5 * tsec) / 0.5
    py = 10.0 * (1.0 - np.cos(0.5 * tsec)) / 0.5
    pz = 0.03 * np.sin(9.0 * tsec)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    # R = Rz(yaw) Ry(pitch) Rx(roll)
    return np.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, px,
                     sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, py,
                     -sp, cp * sr, cp * cr, pz], -1)


def static_poses(n_firings: int) -> np.ndarray:
    return np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64), (n_firings, 1))


def make_profile_stream(sensor, n_firings: int, seed: int, mix: Mixture | None = None, poses: np.ndarray | None = None) -> synth.Stream:
    mix = mix or Mixture()
    rng = np.random.default_rng(seed)
    incl = inclinations(sensor)
    rows = sensor.num_rows
    t = np.full((n_firings, rows), np.nan)
    k = 0
    while k < n_firings:
        kind, s, drop, start = _draw_profile(rng, rows, mix)
        run = int(rng.integers(mix.run[0], mix.run[1] + 1))
        for kk in range(k, min(n_firings, k + run)):
            t[kk] = walk_profile(incl, kind, s + rng.normal(0.0, mix.slope_noise, rows), drop, start, mix)
        k += run
    xyz = points_on_rays(incl, firing_azimuths(sensor, n_firings), t).astype(np.float32)
    inten = rng.integers(0, 256, (n_firings, rows), dtype=np.uint8)
    hit = np.where(np.isnan(t), 0, 1).astype(np.uint16)
    return synth.Stream(xyz=xyz, intensity=inten, poses=static_poses(n_firings) if poses is None else poses, sensor=sensor, hit=hit)


def make_alternating_stream(sensor, n_firings: int, seed: int, mix: Mixture | None = None) -> synth.Stream:
    """Columns that change between ground and obstacle on every second valid row (a staircase of short risers): two rows that rise at 0.3 - 0.45
    (steeper than max_slope: obstacle), two rows at a slope near zero (flat to the row below and, over the whole period, flat to the last certain
    ground point: ground) — with the phase, the slopes and a few missing rows drawn per run of firings."""
    mix = mix or Mixture()
    rng = np.random.default_rng(seed)
    incl = inclinations(sensor)
    rows = sensor.num_rows
    t = np.full((n_firings, rows), np.nan)
    k, next_gap = 0, 22
    while k < n_firings:
        phase = int(rng.integers(0, 4))
        idx = (np.arange(rows)[::-1] + phase) % 4          # counted from the bottom row
        riser = idx >= 2
        s = np.where(riser, rng.uniform(0.30, 0.45, rows), rng.normal(-0.06, 0.01, rows))
        kind = np.where(rng.random(rows) < 0.04, MISSING, FLAT)
        start = ("height", float(rng.choice([0.05, -0.05, 0.1])))
        run = int(rng.integers(1, 9))
        for kk in range(k, min(n_firings, k + run)):
            t[kk] = walk_profile(incl, kind, s + rng.normal(0.0, 0.002, rows), np.zeros(rows), start, mix)
        k += run
        if k >= next_gap:
            # nine firings of plain ground (more than max_distance spans at the bottom row's range): the staircases on either side become
            # clusters of their own and finish, so that columns are published
            for kk in range(k, min(n_firings, k + 9)):
                t[kk] = walk_profile(incl, np.full(rows, FLAT), rng.normal(0.0, 0.01, rows), np.zeros(rows), ("height", 0.0), mix)
            k += 9
            next_gap = k + 22
    xyz = points_on_rays(incl, firing_azimuths(sensor, n_firings), t).astype(np.float32)
    inten = rng.integers(0, 256, (n_firings, rows), dtype=np.uint8)
    return synth.Stream(xyz=xyz, intensity=inten, poses=static_poses(n_firings), sensor=sensor, hit=np.where(np.isnan(t), 0, 1).astype(np.uint16))


def make_chain_stream(sensor, n_firings: int, seed: int, mix: Mixture | None = None) -> synth.Stream:
    """Columns on which a fixed-point iteration over the labels needs about rows / 2 rounds: a wall of one row (not flat to the row below) and one
    flat row, over and over. With max_slope = 1 and "close to the last certain ground" reaching a little more than one riser's height the walls are
    YELLOW, RED, YELLOW, RED ...: the first one above the last certain ground point is close to it, the flat row above a YELLOW one may not move
    that point (cc.cpp:546-548), so the next wall is two risers above it and an obstacle, and the flat row above an obstacle moves the point again.
    Every label depends on where the last ground point is, which depends on the labels of the four rows below: the period of four rows settles
    every two rounds. Phase, start height and a few missing rows are drawn per run of firings; plain ground in between lets clusters finish."""
    mix = mix or Mixture()
    rng = np.random.default_rng(seed)
    incl = inclinations(sensor)
    rows = sensor.num_rows
    t = np.full((n_firings, rows), np.nan)
    k, next_gap = 0, 22
    while k < n_firings:
        phase = int(rng.integers(0, 2))
        riser = ((np.arange(rows)[::-1] + phase) % 2) == 1
        s = np.where(riser, rng.uniform(40.0, 60.0, rows), rng.normal(0.0, 0.004, rows))
        kind = np.where(rng.random(rows) < 0.02, MISSING, FLAT)
        start = ("height", float(rng.choice([0.05, -0.05, 0.1])))
        run = int(rng.integers(1, 9))
        for kk in range(k, min(n_firings, k + run)):
            t[kk] = walk_profile(incl, kind, s, np.zeros(rows), start, mix)
        k += run
        if k >= next_gap:
            for kk in range(k, min(n_firings, k + 9)):
                t[kk] = walk_profile(incl, np.full(rows, FLAT), rng.normal(0.0, 0.01, rows), np.zeros(rows), ("height", 0.0), mix)
            k += 9
            next_gap = k + 22
    xyz = points_on_rays(incl, firing_azimuths(sensor, n_firings), t).astype(np.float32)
    inten = rng.integers(0, 256, (n_firings, rows), dtype=np.uint8)
    return synth.Stream(xyz=xyz, intensity=inten, poses=static_poses(n_firings), sensor=sensor, hit=np.where(np.isnan(t), 0, 1).astype(np.uint16))
