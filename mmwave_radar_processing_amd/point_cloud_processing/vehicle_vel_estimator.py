"""Ego velocity of a vehicle from one frame's point cloud, by a RANSAC loop of its own.

A static scene seen from a platform moving with velocity u shows every point p at the radial speed v = -(p / |p|) . u, so the
least-squares solution c of H c = v with H = p / |p| is the velocity of the *environment* and -c the vehicle's.  Each of
``max_iters`` iterations fits ``points_per_fit`` drawn points, collects every other point whose squared residual is below
``fit_thresh``, and -- with more than ``num_close_pts`` members -- refits on all of them; the refit with the smallest mean
squared error wins.  A previous estimate, when given, first removes the points it does not explain (movers).

Mirrors the public surface and behaviour of the reference's ``point_cloud_processing/vehicle_vel_estimator.py``.  This
single-frame path is plain NumPy on the host: it is the drop-in, and the fallback of ``FramePipeline.vehicle_fits`` (the batched
device path) for the frames its kernel does not decide.  The draws come from ``ransac_tables.vehicle_draws``:
unseeded on every call by default, as in the reference; with ``seed`` set, every call starts from ``default_rng(seed)``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import ransac_tables as T

_NONE = np.empty(shape=0)


def bearings(detections: np.ndarray, dim: int) -> np.ndarray:
    """``[N, dim]`` unit vectors towards the detections' first ``dim`` coordinates."""
    P = detections[:, 0:dim]
    return np.divide(P, np.linalg.norm(P, axis=1).reshape(-1, 1))


def normal_equation_fit(H: np.ndarray, y: np.ndarray) -> np.ndarray:
    return np.linalg.inv(H.T @ H) @ H.T @ y


class VehicleVelEstimator:
    def __init__(self, points_per_fit: int = 7, max_iters: int = 100, fit_thresh: float = 0.05, num_close_pts: int = 10,
                 static_vel_thresh: float = 0.2, seed: Optional[int] = None) -> None:
        if num_close_pts < points_per_fit:
            raise ValueError(f"num_close_pts ({num_close_pts}) must not be below points_per_fit ({points_per_fit}): a frame "
                             "that passes the point-count check must hold a whole draw")
        self.best_fit, self.best_error = None, np.inf
        self.points_per_fit, self.max_iters = points_per_fit, max_iters
        self.fit_thresh, self.num_close_pts = fit_thresh, num_close_pts
        self.static_vel_thresh = static_vel_thresh
        self.seed = seed

    # least squares ----------------------------------------------------------
    def lsq_fit_2D(self, detections: np.ndarray, only_2D: bool = True) -> np.ndarray:
        """The environment's [x, y] (or [x, y, z]) velocity that best explains the detections' radial speeds."""
        return normal_equation_fit(bearings(detections, 2 if only_2D else 3), detections[:, 3])

    def lsq_predict(self, detections: np.ndarray, v: np.ndarray) -> np.ndarray:
        """Radial speed of every detection in an environment moving with ``v`` (three components: 3-D bearings, else 2-D)."""
        return bearings(detections, 3 if v.shape[0] == 3 else 2) @ v

    # losses -----------------------------------------------------------------
    def square_error_loss(self, v_true: np.ndarray, v_pred: np.ndarray) -> np.ndarray:
        return (v_true - v_pred) ** 2

    def mean_square_error(self, v_true: np.ndarray, v_pred: np.ndarray) -> float:
        return np.sum(self.square_error_loss(v_true, v_pred)) / v_true.shape[0]

    # movers -----------------------------------------------------------------
    def get_static_detections(self, detections: np.ndarray, ego_vel: np.ndarray) -> np.ndarray:
        """The detections whose speed a vehicle moving with ``ego_vel`` explains to within ``static_vel_thresh`` (squared)."""
        loss = self.square_error_loss(detections[:, 3], self.lsq_predict(detections, -1 * ego_vel))
        return detections[loss < self.static_vel_thresh, :]

    # RANSAC -----------------------------------------------------------------
    def ransac(self, detections: np.ndarray, initial_ego_vel_est: np.ndarray = _NONE, only_2D: bool = True,
               seed=None) -> Tuple[bool, int]:
        """One frame: (found, points behind the static filter).  ``best_fit`` / ``best_error`` are left as
        ``estimate_ego_vel`` leaves them: untouched below ``num_close_pts`` points, the error reset to inf from there on, both
        replaced by every strictly better consensus refit.  ``seed``: the draws' seed in place of ``self.seed``."""
        pts = np.asarray(detections)
        if pts.shape[0] >= self.num_close_pts and np.shape(initial_ego_vel_est)[0] > 0:
            pts = self.get_static_detections(pts, np.asarray(initial_ego_vel_est))
        n = pts.shape[0]
        if n < self.num_close_pts:
            return False, n
        self.best_error = np.inf
        H, y = bearings(pts, 2 if only_2D else 3), pts[:, 3]
        draws = T.vehicle_draws(self.seed if seed is None else seed, n, self.max_iters, self.points_per_fit)
        for drawn in draws:
            model = normal_equation_fit(H[drawn], y[drawn])
            close = self.square_error_loss(y, H @ model) < self.fit_thresh
            close[drawn] = False                       # the drawn points are members whatever their residual
            members = np.concatenate((drawn, np.flatnonzero(close)))
            if members.shape[0] > self.num_close_pts:
                model = normal_equation_fit(H[members], y[members])
                error = self.mean_square_error(y[members], H[members] @ model)
                if error < self.best_error:
                    self.best_error, self.best_fit = error, model
        return bool(self.best_error != np.inf), n

    def estimate_ego_vel(self, detections: np.ndarray, initial_ego_vel_est: np.ndarray = _NONE,
                         only_2D: bool = True) -> np.ndarray:
        """The vehicle's [x, y] (or [x, y, z]) velocity, or an empty array: fewer than ``num_close_pts`` points (before or
        after the static filter an initial estimate asks for), or no iteration with a consensus."""
        found, _ = self.ransac(detections, initial_ego_vel_est, only_2D)
        return self.get_vehicle_vel_est() if found else np.empty(shape=0)

    def get_vehicle_vel_est(self) -> np.ndarray:
        return self.best_fit * -1
