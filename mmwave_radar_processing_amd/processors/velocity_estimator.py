"""Ego velocity from the Doppler-azimuth response of one frame's ADC cube (reference module path:
mmwave_radar_processing/processors/velocity_estimator.py; not the point-cloud class of the same name in
``point_cloud_processing.vel_estimator`` -- the two are told apart by module, as in the reference).

A static scene seen from a platform moving with (vx, vy) shows a scatterer at azimuth theta at the Doppler velocity
vd = -(vx cos(theta) + vy sin(theta)).  One frame is worked off in three stages:

1. Doppler-azimuth maps (``DopplerAzimuthProcessor.process``) of the range bins around the altitude: one antenna set on a
   ``standard`` array, the mean of two sets per direction (azimuth, elevation) on an ``ods`` array;
2. peaks: the strongest peak down the zero-azimuth column gives vx = -vd(0) (the mean of both directions where both exist);
   one peak per velocity row gives the (theta, vd) pairs of the regression;
3. a RANSAC line fit without intercept of those pairs: for vx >= 0.1 of y = -vd - vx cos(theta) on sin(theta), whose slope
   is vy; for a small vx of theta on (vd - vx), whose slope a gives vy = -1 / a.  R^2 on the inliers and the inlier share
   gate what the current estimate takes from the proposal.

With ``enable_precise_responses`` stages 1 and 2 are repeated on zoomed maps centred on -vx before stage 3.  The batched form
of all of this over resident frames is ``FramePipeline.doppler_azimuth_velocities``; this class is its
per-frame drop-in, its source of parameters and the host refit of the pairs the device flags.
"""
from __future__ import annotations

import numpy as np

from .._lazy import lazy_import
from ..point_cloud_processing import ransac_tables as T
from ..point_cloud_processing.vel_estimator import ransac_fit
from .doppler_azimuth_resp import DopplerAzimuthProcessor

VX_BRANCH = 0.1                   # below this vx the regression is turned round (theta on vd - vx)
THRESHOLD_STANDARD = 0.15         # residual thresholds of the two regressions
THRESHOLD_SMALL_VX = 0.20
NO_PEAK = np.empty(shape=0)

# antenna sets by (geometry, virtual antennas): per direction one set, or two whose maps are averaged; shift_angle per direction
AZIMUTH_SETS = {("standard", True): [list(range(8))], ("standard", False): [list(range(4))],
                ("ods", True): [[0, 3, 4, 7], [1, 2, 5, 6]], ("ods", False): [[0, 3], [1, 2]]}
ELEVATION_SETS = {("ods", True): [[10, 11, 6, 7], [9, 8, 5, 4]], ("ods", False): [[1, 0], [3, 4]]}


def antenna_plan(config_manager):
    """``(rx_sets, groups, shift_angle)`` of ``FramePipeline.doppler_azimuth_peaks`` for this array: the azimuth group first,
    then (ods) the elevation group, whose maps are taken without the angle shift."""
    key = (config_manager.array_geometry, bool(config_manager.virtual_antennas_enabled))
    if key not in AZIMUTH_SETS:
        raise ValueError(f"no antenna sets for array geometry {config_manager.array_geometry!r}")
    az, el = AZIMUTH_SETS[key], ELEVATION_SETS.get(key, [])
    sets = az + el
    groups = [tuple(range(len(az)))] + ([tuple(range(len(az), len(sets)))] if el else [])
    return sets, groups, [True] * len(az) + [False] * len(el)


def _ransac_line(H: np.ndarray, y: np.ndarray, threshold: float):
    """The fitted model of the one-column regression, or None where RANSAC raises (fewer than 10 pairs, no consensus set)."""
    lm = lazy_import("sklearn.linear_model")
    model = lm.RANSACRegressor(estimator=lm.LinearRegression(fit_intercept=False), residual_threshold=threshold,
                               random_state=T.SEED, max_trials=T.MAX_TRIALS, min_samples=T.MIN_SAMPLES)
    try:
        return model.fit(H.reshape(-1, 1), y)
    except ValueError:
        return None


class VelocityEstimator(DopplerAzimuthProcessor):
    def __init__(self, config_manager, lower_range_bound: float, upper_range_bound: float, precise_vel_bound: float = 0.25,
                 valid_angle_range: np.ndarray = np.array([np.deg2rad(-70), np.deg2rad(70)]), peak_threshold_dB: float = 30.0,
                 x_measurement_only: bool = False, min_R2_threshold: float = 0.6, min_inlier_percent: float = 0.75,
                 **kwargs) -> None:
        super().__init__(config_manager=config_manager, num_angle_bins=64, valid_angle_range=np.asarray(valid_angle_range))
        self.lower_range_bound, self.upper_range_bound = lower_range_bound, upper_range_bound
        self.precise_vel_bound = precise_vel_bound
        self.peak_threshold_dB = peak_threshold_dB
        self.x_measurement_only = x_measurement_only
        self.min_R2_threshold, self.min_inlier_percent = min_R2_threshold, min_inlier_percent
        # the latest maps and peaks
        self.azimuth_response_mag = self.elevation_response_mag = NO_PEAK
        self.precise_azimuth_response_mag = self.precise_elevation_response_mag = NO_PEAK
        self.az_resps_mag, self.el_resps_mag = [], []
        self.azimuth_peaks = self.azimuth_peak_zero_az = NO_PEAK
        self.elevation_peaks = self.elevation_peak_zero_az = NO_PEAK
        # the estimates; vx < 0 marks "no ADC-cube estimate yet" for the gate of the points path
        self.ego_vx_estimate = -1.0
        self.azimuth_ego_vy_estimate = self.azimuth_estimate_R2 = self.azimuth_inlier_percent = 0.0
        self.elevation_ego_vy_estimate = self.elevation_estimate_R2 = self.elevation_inlier_percent = 0.0
        self.proposed_velocity_estimate = np.empty(shape=0)
        self.current_velocity_estimate = np.array([0.0, 0.0, 0.0])
        self.history_R2_statistics, self.history_inlier_statistics = [], []

    def reset(self):
        self.history_R2_statistics, self.history_inlier_statistics = [], []
        return super().reset()

    def update_history(self, estimated: np.ndarray = np.empty(0), ground_truth: np.ndarray = np.empty(0)) -> None:
        self.history_R2_statistics.append(np.array([self.azimuth_estimate_R2, self.elevation_estimate_R2]))
        self.history_inlier_statistics.append(np.array([self.azimuth_inlier_percent, self.elevation_inlier_percent]))
        return super().update_history(estimated=estimated, ground_truth=ground_truth)

    # stage 1: maps ------------------------------------------------------------------------------------------------------
    def get_range_window(self, altitude: float = 0.0, sensing_direction: str = "down") -> np.ndarray:
        """[min, max] range in metres: around the altitude when looking down, everything past 1 m when looking out."""
        far = self.config_manager.range_max_m
        if sensing_direction == "down":
            return np.array([max(0, altitude - self.lower_range_bound), min(far, altitude + self.upper_range_bound)])
        if sensing_direction == "out":
            return np.array([1.0, far])
        return None

    def _direction_response(self, sets, shift_angle, adc_cube, range_window, use_precise_fft, centre):
        vel_range = np.array([centre - self.precise_vel_bound, centre + self.precise_vel_bound])
        maps = [super(VelocityEstimator, self).process(adc_cube=adc_cube, rx_antennas=np.array(s), range_window=range_window,
                                                       shift_angle=shift_angle, use_precise_fft=use_precise_fft,
                                                       precise_vel_range=vel_range) for s in sets]
        return maps, (maps[0] if len(maps) == 1 else (maps[0] + maps[1]) / 2)

    def _sets(self, table, what: str):
        cm = self.config_manager
        key = (cm.array_geometry, bool(cm.virtual_antennas_enabled))
        if key not in table:
            raise NotImplementedError(f"no {what.lower()} antenna sets for a {cm.array_geometry!r} array")
        return table[key]

    def compute_azimuth_response(self, adc_cube: np.ndarray, range_window: np.ndarray, use_precise_fft: bool = False,
                                 precise_fft_center_vel: float = 0.0):
        maps, mean = self._direction_response(self._sets(AZIMUTH_SETS, "Azimuth"), True, adc_cube, range_window, use_precise_fft,
                                              precise_fft_center_vel)
        if len(maps) == 2:
            self.az_resps_mag = maps
        if use_precise_fft:
            self.precise_azimuth_response_mag = mean
        else:
            self.azimuth_response_mag = mean

    def compute_elevation_response(self, adc_cube: np.ndarray, range_window: np.ndarray, use_precise_fft: bool = False,
                                   precise_fft_center_vel: float = 0.0):
        maps, mean = self._direction_response(self._sets(ELEVATION_SETS, "Elevation"), False, adc_cube, range_window,
                                              use_precise_fft, precise_fft_center_vel)
        self.el_resps_mag = maps
        if use_precise_fft:
            self.precise_elevation_response_mag = mean
        else:
            self.elevation_response_mag = mean

    # stage 2: peaks -----------------------------------------------------------------------------------------------------
    def _maps_and_bins(self, use_precise_response: bool):
        if use_precise_response:
            return self.precise_azimuth_response_mag, self.precise_elevation_response_mag, self.zoomed_vel_bins
        return self.azimuth_response_mag, self.elevation_response_mag, self.vel_bins

    def detect_vel_row_peaks(self, use_precise_response: bool = False):
        """One (angle, velocity) peak per velocity row of each direction that has a map; the others keep their last peaks."""
        az, el, bins = self._maps_and_bins(use_precise_response)
        if az.shape[0] > 0:
            self.azimuth_peaks = self.detect_peaks_rows(az, bins, self.peak_threshold_dB)
        if el.shape[0] > 0:
            self.elevation_peaks = self.detect_peaks_rows(el, bins, self.peak_threshold_dB)

    def detect_vel_zero_az_peaks(self, use_precise_response: bool = False):
        az, el, bins = self._maps_and_bins(use_precise_response)
        if az.shape[0] > 0:
            self.azimuth_peak_zero_az = self.detect_peak_zero_az(az, bins, self.peak_threshold_dB)
        if el.shape[0] > 0:
            self.elevation_peak_zero_az = self.detect_peak_zero_az(el, bins, self.peak_threshold_dB)

    def estimate_ego_vx_velocity(self):
        """vx from the zero-azimuth peaks: minus their mean, minus the one that exists, or 0."""
        az, el = self.azimuth_peak_zero_az, self.elevation_peak_zero_az
        if az.shape[0] > 0 and el.shape[0] > 0:
            self.ego_vx_estimate = -1 * (az[1] + el[1]) / 2.0
        elif az.shape[0] > 0:
            self.ego_vx_estimate = -1 * az[1]
        elif el.shape[0] > 0:
            self.ego_vx_estimate = -1 * el[1]
        else:
            self.ego_vx_estimate = 0.0
        return self.ego_vx_estimate

    # stage 3: regression ------------------------------------------------------------------------------------------------
    def lsq_fit_ego_vy_ransac(self, peaks: np.ndarray):
        if self.ego_vx_estimate >= VX_BRANCH:
            return self.lsq_fit_ego_vy_ransac_standard(peaks=peaks)
        return self.lsq_fit_ego_vy_ransac_small_vx(peaks=peaks)

    def lsq_fit_ego_vel_ransac_points(self, points: np.ndarray = np.empty(shape=0)):
        """(vx, vy), R^2, inlier share from (x, y, z, v) points; no points: the bare zero vector."""
        return ransac_fit(points, 2) if points.shape[0] else np.array([0.0, 0.0])

    def lsq_fit_ego_vy_ransac_standard(self, peaks: np.ndarray):
        """vy, R^2 on the inliers (0 with at most 3), inlier share; a bare 0.0 without peaks."""
        if peaks is None or len(peaks) == 0:
            return 0.0
        y = -1 * peaks[:, 1] - self.ego_vx_estimate * np.cos(peaks[:, 0])
        H = np.sin(peaks[:, 0]).reshape(-1, 1)
        model = _ransac_line(H, y, THRESHOLD_STANDARD)
        if model is None:
            return 0.0, 0.0, 0.0
        inliers = model.inlier_mask_
        count = inliers.sum()
        r2 = model.score(H[inliers], y[inliers]) if count > 3 else 0.0
        return model.estimator_.coef_[0], r2, count / len(inliers)

    def lsq_fit_ego_vy_ransac_small_vx(self, peaks: np.ndarray):
        """The regression turned round, theta = a (vd - vx) with vy = -1 / a: near vx = 0 the peaks lie along the angle axis."""
        if peaks is None or len(peaks) == 0:
            return 0.0, 0.0
        y = peaks[:, 0]
        H = (peaks[:, 1] - self.ego_vx_estimate).reshape(-1, 1)
        model = _ransac_line(H, y, THRESHOLD_SMALL_VX)
        if model is None:
            return 0.0, 0.0, 0.0
        inliers = model.inlier_mask_
        a = model.estimator_.coef_[0]
        return (-1 / a if a != 0 else 0.0), model.score(H[inliers], y[inliers]), inliers.sum() / len(inliers)

    def lsq_fit_ego_vy(self, peaks: np.ndarray):
        """Plain least squares of the standard regression (no outlier rejection)."""
        if peaks is None or len(peaks) == 0:
            return 0.0
        y = -1 * peaks[:, 1] - (self.ego_vx_estimate * np.cos(peaks[:, 0]))
        H = np.sin(peaks[:, 0])[:, np.newaxis]
        return np.linalg.lstsq(H, y, rcond=None)[0][0]

    def lsq_predict_velocity_measurement(self, v: np.ndarray, angles_to_predict: np.ndarray = np.empty(shape=0)):
        """The Doppler velocity a static scene shows at each angle for the ego velocity v = [vx, vy]."""
        angles = self.valid_angle_bins if np.size(angles_to_predict) == 0 else angles_to_predict
        return -1 * np.dot(np.stack([np.cos(angles), np.sin(angles)], axis=-1), v)

    def compute_R2_statistics(self):
        """R^2 of the proposal's predicted Doppler velocities against all row peaks of each direction (inliers or not)."""
        geometry = self.config_manager.array_geometry
        vel = self.proposed_velocity_estimate

        def r2(peaks, v):
            rss = np.sum((peaks[:, 1] - self.lsq_predict_velocity_measurement(v=v, angles_to_predict=peaks[:, 0])) ** 2)
            tss = np.sum((peaks[:, 1] - np.mean(peaks[:, 1])) ** 2)
            return 1 - rss / tss if tss > 0 else 0

        if self.azimuth_peaks.shape[0] > 0 and geometry in ("ods", "standard"):
            v = np.array([vel[2], vel[0]]) if geometry == "ods" else np.array([vel[0], vel[1]])
            self.azimuth_estimate_R2 = r2(self.azimuth_peaks, v)
        if self.elevation_peaks.shape[0] > 0:
            if geometry != "ods":
                raise NotImplementedError(f"elevation peaks have no velocity components to be scored against on a {geometry!r} array")
            self.elevation_estimate_R2 = r2(self.elevation_peaks, np.array([vel[2], vel[1]]))

    def update_and_check_current_vel_measurements(self):
        """What the current estimate takes from the proposal.  ods: the boresight component always, each lateral component when
        its direction's R^2 and inlier share reach the thresholds (else 0).  standard, ADC cube: vx always, vy when the R^2 does;
        standard, points (vx still negative): the whole proposal or zeros by the R^2."""
        cur, new = self.current_velocity_estimate, self.proposed_velocity_estimate
        if self.x_measurement_only:
            cur[0] = new[0]
            return
        geometry = self.config_manager.array_geometry
        az_ok = self.azimuth_estimate_R2 >= self.min_R2_threshold
        if geometry == "ods":
            el_ok = self.elevation_estimate_R2 >= self.min_R2_threshold
            cur[0] = new[0] if az_ok and self.azimuth_inlier_percent >= self.min_inlier_percent else 0.0
            cur[1] = new[1] if el_ok and self.elevation_inlier_percent >= self.min_inlier_percent else 0.0
            cur[2] = new[2]
        elif geometry == "standard":
            if self.ego_vx_estimate < 0.0:
                self.current_velocity_estimate = new if az_ok else np.array([0.0, 0.0, 0.0])
            else:
                cur[1] = new[1] if az_ok else 0.0
                cur[0] = new[0]
                cur[2] = 0.0

    def take_fits(self, azimuth=None, elevation=None) -> None:
        """Install (vy, R^2, share) of a direction -- None keeps what the last frame left -- and form the proposal in the
        geometry's component order: ods [az vy, el vy, vx] (x is boresight), standard [vx, az vy, 0]."""
        if azimuth is not None:
            self.azimuth_ego_vy_estimate, self.azimuth_estimate_R2, self.azimuth_inlier_percent = azimuth
        if elevation is not None:
            self.elevation_ego_vy_estimate, self.elevation_estimate_R2, self.elevation_inlier_percent = elevation
        geometry = self.config_manager.array_geometry
        if self.x_measurement_only:
            self.proposed_velocity_estimate = np.array([self.ego_vx_estimate])
        elif geometry == "ods":
            self.proposed_velocity_estimate = np.array([self.azimuth_ego_vy_estimate, self.elevation_ego_vy_estimate,
                                                        self.ego_vx_estimate])
        elif geometry == "standard":
            self.proposed_velocity_estimate = np.array([self.ego_vx_estimate, self.azimuth_ego_vy_estimate, 0.0])

    def estimate_ego_velocity_adc_data(self):
        """The fits of the directions that have row peaks, then the proposal."""
        if self.x_measurement_only:
            return self.take_fits()
        fits = [self.lsq_fit_ego_vy_ransac(peaks=p) if p.shape[0] > 0 else None for p in (self.azimuth_peaks, self.elevation_peaks)]
        self.take_fits(*fits)

    def estimate_ego_velocity_points(self, points: np.ndarray = np.empty(shape=0)):
        geometry = self.config_manager.array_geometry
        if geometry == "ods":
            raise NotImplementedError("points= needs the two-column fit of a standard array; an ods array estimates from ADC cubes only")
        if geometry == "standard":
            vel, self.azimuth_estimate_R2, self.azimuth_inlier_percent = self.lsq_fit_ego_vel_ransac_points(points=points)
            self.proposed_velocity_estimate = np.array([vel[0]]) if self.x_measurement_only else np.array([vel[0], vel[1], 0.0])

    def process(self, adc_cube: np.ndarray = np.empty(shape=0), points: np.ndarray = np.empty(shape=0), altitude: float = 0.0,
                enable_precise_responses: bool = False, **kwargs) -> np.ndarray:
        """One frame -> the current [vx, vy, vz]: from the ADC cube ``[rx, sample, chirp]`` where one is given, else from
        ``points`` (x, y, z, v)."""
        points = np.asarray(points)
        adc_cube = np.asarray(adc_cube)
        cm = self.config_manager
        if adc_cube.shape[0] > 0:
            window = self.get_range_window(altitude=altitude, sensing_direction=cm.array_direction)
            with_elevation = cm.array_geometry == "ods"
            for precise in ((False, True) if enable_precise_responses else (False,)):
                centre = -1 * self.ego_vx_estimate if precise else 0.0
                self.compute_azimuth_response(adc_cube, window, use_precise_fft=precise, precise_fft_center_vel=centre)
                if with_elevation:
                    self.compute_elevation_response(adc_cube, window, use_precise_fft=precise, precise_fft_center_vel=centre)
                self.detect_vel_zero_az_peaks(use_precise_response=precise)
                self.estimate_ego_vx_velocity()
            if not self.x_measurement_only:
                self.detect_vel_row_peaks(use_precise_response=enable_precise_responses)
            self.estimate_ego_velocity_adc_data()
        elif points.shape[0] > 0:
            self.estimate_ego_velocity_points(points=points)
        self.update_and_check_current_vel_measurements()
        return self.current_velocity_estimate
