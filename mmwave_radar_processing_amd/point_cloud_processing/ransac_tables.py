"""Host-made tables of the batched ego-velocity kernel (``mmw_ego_velocity_ransac``).

Everything random or transcendental in scikit-learn's RANSAC loop is a function of the point count N alone, so it is evaluated
here once per N (and kept for the life of the process) and the kernel only looks it up:

* ``subset_table(N)``: the 20 x 10 indices ``RANSACRegressor(random_state=42, min_samples=10, max_trials=20).fit`` draws for N
  samples -- a fresh ``RandomState(42)`` per fit, one ``sample_without_replacement(N, 10)`` per trial, skipped or not;
* ``trials_table(N)``: ``min(20, _dynamic_max_trials(k, N, 10, 0.99))`` for k = 0 .. N inliers.

``vehicle_draws`` / ``vehicle_tables`` do the same for ``VehicleVelEstimator``'s own loop (``mmw_vehicle_velocity_ransac``,
DESIGN.md 4.25): the heads of ``default_rng(seed).permutation(N)``, NumPy only.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from .._lazy import lazy_import

MIN_SAMPLES = 10
MAX_TRIALS = 20
STOP_PROBABILITY = 0.99
SEED = 42
_EPSILON = np.spacing(1)

_subsets: Dict[int, np.ndarray] = {}
_trials: Dict[int, np.ndarray] = {}


def subset_table(n: int) -> np.ndarray:
    n = int(n)
    tab = _subsets.get(n)
    if tab is None:
        if n < MIN_SAMPLES:
            raise ValueError(f"no {MIN_SAMPLES}-point subset of {n} points")
        draw = lazy_import("sklearn.utils.random").sample_without_replacement
        rs = np.random.RandomState(SEED)
        tab = np.array([draw(n, MIN_SAMPLES, random_state=rs) for _ in range(MAX_TRIALS)], dtype=np.int32)
        tab.setflags(write=False)
        _subsets[n] = tab
    return tab


def dynamic_max_trials(n_inliers, n_samples: int) -> float:
    """scikit-learn 1.7.2 ``_dynamic_max_trials(n_inliers, n_samples, 10, 0.99)``: the same NumPy scalar expression."""
    inlier_ratio = n_inliers / float(n_samples)
    nom = max(_EPSILON, 1 - STOP_PROBABILITY)
    denom = max(_EPSILON, 1 - inlier_ratio ** MIN_SAMPLES)
    if nom == 1:
        return 0
    if denom == 1:
        return float("inf")
    return abs(float(np.ceil(np.log(nom) / np.log(denom))))


def trials_table(n: int) -> np.ndarray:
    """int32 ``[n + 1]``.  Evaluated from k = n downwards; the value grows as k falls, and once eight consecutive k have
    reached the cap of 20 the rest is 20 (``trials_table_full`` evaluates every k; the tests compare the two)."""
    n = int(n)
    tab = _trials.get(n)
    if tab is None:
        tab = np.full(n + 1, MAX_TRIALS, dtype=np.int32)
        run = 0
        for k in range(n, -1, -1):
            v = min(float(MAX_TRIALS), dynamic_max_trials(np.int64(k), n))
            tab[k] = int(v)
            run = run + 1 if v >= MAX_TRIALS else 0
            if run >= 8:
                break
        tab.setflags(write=False)
        _trials[n] = tab
    return tab


def trials_table_full(n: int) -> np.ndarray:
    return np.array([int(min(float(MAX_TRIALS), dynamic_max_trials(np.int64(k), n))) for k in range(int(n) + 1)], dtype=np.int32)


def seed_tables(n: int, subsets: np.ndarray, trials: np.ndarray) -> None:
    """Install recorded tables for N = n (a host without scikit-learn driving the kernel from stored draws)."""
    subsets = np.ascontiguousarray(subsets, dtype=np.int32)
    trials = np.ascontiguousarray(trials, dtype=np.int32)
    if subsets.shape != (MAX_TRIALS, MIN_SAMPLES) or trials.shape != (int(n) + 1,) or subsets.min() < 0 or subsets.max() >= n:
        raise ValueError(f"tables do not fit N = {n}")
    _subsets[int(n)], _trials[int(n)] = subsets, trials


def frame_tables(counts: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The four table arguments of ``mmw_ego_velocity_ransac`` for a batch with these point counts:
    ``subsets [R, 20, 10]``, ``subset_row [F]`` (-1 below 10 points), ``trials_tab``, ``trials_off [R]``."""
    counts = np.asarray(counts, dtype=np.int64)
    sizes = np.unique(counts[counts >= MIN_SAMPLES])
    row = np.full(counts.shape, -1, dtype=np.int32)
    subsets = np.zeros((max(len(sizes), 1), MAX_TRIALS, MIN_SAMPLES), dtype=np.int32)
    offs = np.zeros(max(len(sizes), 1), dtype=np.int32)
    tabs, off = [], 0
    for r, n in enumerate(sizes.tolist()):
        subsets[r] = subset_table(n)
        t = trials_table(n)
        offs[r] = off
        tabs.append(t)
        off += len(t)
        row[counts == n] = r
    tab = np.concatenate(tabs) if tabs else np.zeros(1, dtype=np.int32)
    return subsets[:len(sizes)] if len(sizes) else subsets[:0], row, tab, offs[:len(sizes)]


_dopaz: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}


def dopaz_tables(n_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """The two table arguments of ``mmw_doppler_azimuth_ransac`` for peak lists of up to ``n_rows`` pairs, made once per
    ``n_rows`` and kept: ``subsets`` int32 ``[n_tab, 20, 10]`` with row N - 10 the draws for N pairs, and ``trials``, the
    ``trials_table_full(N)`` rows (N + 1 entries each) one behind the other, for N = 10 .. n_rows.  The kernel indexes both by
    the N it counted.  Below 10 rows no fit is possible: ``n_tab`` is 0 and both arrays hold one unused entry."""
    n_rows = int(n_rows)
    tabs = _dopaz.get(n_rows)
    if tabs is None:
        sizes = range(MIN_SAMPLES, n_rows + 1)
        subsets = np.zeros((max(len(sizes), 1), MAX_TRIALS, MIN_SAMPLES), dtype=np.int32)
        trials = [np.zeros(1, dtype=np.int32)] if not len(sizes) else []
        for row, n in enumerate(sizes):
            subsets[row] = subset_table(n)
            t = trials_table(n)
            trials.append(t)
        tabs = (subsets, np.ascontiguousarray(np.concatenate(trials), dtype=np.int32))
        for t in tabs:
            t.setflags(write=False)
        _dopaz[n_rows] = tabs
    return tabs


_vehicle: Dict[Tuple[int, int, int, int], np.ndarray] = {}
VEHICLE_CACHE_TABLES = 4096      # draw tables kept (an unseeded estimator's batch calls bring a new seed each): emptied beyond that


def vehicle_draws(seed, n: int, max_iters: int, points_per_fit: int) -> np.ndarray:
    """The draws of one ``VehicleVelEstimator.estimate_ego_vel`` call on ``n`` points: int32 ``[max_iters, points_per_fit]``, row i
    the first ``points_per_fit`` entries of the i-th ``rng.permutation(n)`` of a fresh ``np.random.default_rng(seed)`` (the rest of
    a permutation only orders the class's sums).  Kept per ``(seed, n, max_iters, points_per_fit)``, at most ``VEHICLE_CACHE_TABLES`` of them; ``seed=None`` draws from OS
    entropy and keeps nothing.  The host class and ``mmw_vehicle_velocity_ransac``'s tables both come from here."""
    n, max_iters, points_per_fit = int(n), int(max_iters), int(points_per_fit)
    if n < points_per_fit:
        raise ValueError(f"no {points_per_fit}-point draw from {n} points")
    key = None if seed is None else (int(seed), n, max_iters, points_per_fit)
    tab = _vehicle.get(key) if key is not None else None
    if tab is None:
        rng = np.random.default_rng(seed)
        tab = np.array([rng.permutation(n)[:points_per_fit] for _ in range(max_iters)], dtype=np.int32).reshape(max_iters, points_per_fit)
        tab.setflags(write=False)
        if key is not None:
            if len(_vehicle) >= VEHICLE_CACHE_TABLES:
                _vehicle.clear()
            _vehicle[key] = tab
    return tab


def vehicle_tables(seed, sizes, n_max: int, max_iters: int, points_per_fit: int) -> np.ndarray:
    """The ``d_draws`` argument of ``mmw_vehicle_velocity_ransac``: int32 ``[n_tab, max_iters, points_per_fit]`` with row
    ``N - points_per_fit`` the draws for N points, ``n_tab = n_max - points_per_fit + 1`` (one unused row when that is below 1).
    Only the point counts in ``sizes`` are drawn; every other row holds -1, which the kernel reports instead of reading."""
    n_tab = max(int(n_max) - int(points_per_fit) + 1, 1)
    tab = np.full((n_tab, int(max_iters), int(points_per_fit)), -1, dtype=np.int32)
    for n in sorted({int(n) for n in sizes}):
        if points_per_fit <= n <= n_max:
            tab[n - points_per_fit] = vehicle_draws(seed, n, max_iters, points_per_fit)
    return tab
