"""Ego velocity from one frame's point cloud: a robust no-intercept line fit of the Doppler speeds on the bearings.

A static scene seen from a platform moving with velocity u shows every point p at the radial speed v = -(p / |p|) . u, so
the regression of y = -v on H = p / |p| has u as its coefficients; scikit-learn's RANSAC (10-point subsets, 0.15 m/s residual
threshold, at most 20 trials, seed 42) keeps movers and clutter out of the fit.  ``standard`` arrays resolve azimuth only
(u = (vx, vy, 0)), ``ods`` arrays all three components.  A proposed estimate replaces the current one only when the fit's
R^2 on its inliers and its inlier share both reach their thresholds.

Mirrors the public behaviour of the reference's ``point_cloud_processing/vel_estimator.py`` (constructor, attributes,
histories, ``process(points=...)``), including that a failed 3-D fit returns a 2-vector of zeros.  The per-frame fit runs
scikit-learn on the host: it is the drop-in and the fallback of ``FramePipeline.ego_velocities`` (the batched device path).
"""
from __future__ import annotations

import numpy as np

from .._lazy import lazy_import
from ..processors._processor import _Processor
from . import ransac_tables as T

RESIDUAL_THRESHOLD = 0.15


def ransac_fit(points: np.ndarray, dim: int, return_mask: bool = False):
    """(coefficients, R^2 on the inliers, inlier share) of one frame; zeros (a 2-vector, whatever ``dim``) when RANSAC finds
    no consensus set or there are fewer than 10 points."""
    lm = lazy_import("sklearn.linear_model")
    y = -1 * points[:, 3]
    H = points[:, 0:dim] / np.linalg.norm(points[:, 0:dim], axis=1, keepdims=True)
    model = lm.RANSACRegressor(estimator=lm.LinearRegression(fit_intercept=False), residual_threshold=RESIDUAL_THRESHOLD,
                               random_state=T.SEED, max_trials=T.MAX_TRIALS, min_samples=T.MIN_SAMPLES)
    try:
        model.fit(H, y)
    except ValueError:
        failed = (np.array([0.0, 0.0]), 0.0, 0.0)
        return failed + (np.zeros(len(y), dtype=bool),) if return_mask else failed
    inliers = model.inlier_mask_
    count = inliers.sum()
    r2 = model.score(H[inliers], y[inliers]) if count > 3 else 0.0
    out = (model.estimator_.coef_, r2, count / len(inliers))
    return out + (inliers,) if return_mask else out


GEOMETRY_DIM = {"standard": 2, "ods": 3}      # regression columns per array geometry


class VelocityEstimator(_Processor):
    def __init__(self, config_manager, min_R2_threshold: float = 0.6, min_inlier_percent: float = 0.75, **kwargs) -> None:
        super().__init__(config_manager=config_manager)
        self.min_R2_threshold, self.min_inlier_percent = min_R2_threshold, min_inlier_percent
        self.estimated_R2 = self.inlier_percent = 0.0
        self.proposed_velocity_estimate = np.empty(shape=0)
        self.current_velocity_estimate = np.zeros(3)
        self.history_R2_statistics, self.history_inlier_statistics = [], []

    def reset(self):
        self.history_R2_statistics, self.history_inlier_statistics = [], []
        return super().reset()

    def update_history(self, estimated: np.ndarray = np.empty(0), ground_truth: np.ndarray = np.empty(0)) -> None:
        for log, value in ((self.history_R2_statistics, self.estimated_R2), (self.history_inlier_statistics, self.inlier_percent)):
            log.append(value)
        return super().update_history(estimated=estimated, ground_truth=ground_truth)

    # one frame's fit ------------------------------------------------------
    def lsq_fit_ego_vel_ransac_points_2D(self, points: np.ndarray = np.empty(shape=0)):
        """(vx, vy), R^2, inlier share; no points: the bare zero vector (what the reference returns; process() never asks)."""
        return ransac_fit(points, 2) if len(points) else np.zeros(2)

    def lsq_fit_ego_vel_ransac_points_3D(self, points: np.ndarray = np.empty(shape=0)):
        return ransac_fit(points, 3) if len(points) else (np.zeros(3), 0.0, 0.0)

    def take_fit(self, dim: int, fit) -> None:
        """A frame's (coefficients, R^2, inlier share) become the statistics and the proposal: [vx, vy, 0] from a 2-D fit, the
        fit's own vector (two zeros when it failed) from a 3-D one."""
        vel, self.estimated_R2, self.inlier_percent = fit
        self.proposed_velocity_estimate = vel if dim == 3 else np.array([vel[0], vel[1], 0.0])

    def estimate_ego_velocity_points(self, points: np.ndarray = np.empty(shape=0)):
        dim = GEOMETRY_DIM.get(self.config_manager.array_geometry)
        if dim is not None:                     # any other geometry: nothing is estimated
            fit = self.lsq_fit_ego_vel_ransac_points_3D if dim == 3 else self.lsq_fit_ego_vel_ransac_points_2D
            self.take_fit(dim, fit(points=points))

    def update_and_check_current_vel_measurements(self):
        """The proposal is adopted when the statistics it came with reach both thresholds."""
        if self.estimated_R2 >= self.min_R2_threshold and self.inlier_percent >= self.min_inlier_percent:
            self.current_velocity_estimate = self.proposed_velocity_estimate

    def process(self, points: np.ndarray = np.empty(shape=0), **kwargs) -> np.ndarray:
        """One frame's ``(N, 4)`` (x, y, z, v) points -> the current [vx, vy, vz].  An empty frame estimates nothing: the
        statistics and the proposal of the last non-empty frame are checked again."""
        points = np.asarray(points)
        if len(points):
            self.estimate_ego_velocity_points(points=points)
        self.update_and_check_current_vel_measurements()
        return self.current_velocity_estimate
