"""Synthetic-array (delay-and-sum) beamformer over an aperture synthesised from platform motion (reference:
mmwave_radar_processing/processors/simple_synthetic_array_beamformer_processor_multiFrame.py:175-246, 332-472, 818-872).

The processor keeps ``num_frames`` frames of every ``stride``-th chirp of one transmitter as seen by one receiver, and a velocity
history of the same length.  While the history says "steady straight flight" (the validity gate), the chirps of the window are the
elements of a synthetic array whose positions follow from integrating the velocities backwards from the newest chirp; the image
is ``FFT_S(hann(S) . X[S, E] W[E, T])`` with ``W`` the Hamming-tapered steering matrix -- ``SyntheticArrayBeamformerCore.contract``.

Host state here is two small scans (``gate`` and ``window_geometry``, both pure functions of a velocity history);
``batch.synthetic_array_geometry`` runs them for a whole sequence and ``FramePipeline.synthetic_array`` contracts every valid frame
of a resident batch in one ``mmw_synth_array`` call, reading the windows in place.

Calibration against targets of opportunity is ``SelfCalibratingSyntheticArrayProcessor`` (below; batched as
``FramePipeline.synthetic_array_calibrated`` on ``mmw_synth_array_calibrate``); the plain class keeps refusing
``enable_calibration=True``.  The beam pattern of a geometry -- the aperture the motion synthesised, with unit signals and no
taper -- is ``compute_synthetic_array_pattern`` (one direction on the host: ``compute_array_factor_at_angle``); for every valid
frame of a drive at once ``batch.synthetic_array_patterns`` / ``FramePipeline.synthetic_array_patterns`` on
``mmw_synth_array_pattern``.  Left out on purpose: the Cartesian ``griddata`` resampling of the image, which is presentation (and
raises upstream for more than one elevation bin).
"""
from __future__ import annotations

import numpy as np

from ._processor import _Processor
from .steering_beamformers import SyntheticArrayBeamformerCore

SPEED_OF_LIGHT_M_S = 299792458.0        # scipy.constants.c


def gate(history: np.ndarray, min_vel, max_vel, max_vel_stdev) -> bool:
    """The validity gate on a velocity history ``[H, 3]``: every |component| inside [min_vel, max_vel], the spread of each component
    at most max_vel_stdev, and every pair of directions within cos > 0.95 (the norm carries the reference's +1e-6)."""
    mag = np.abs(history)
    if not (np.all(mag >= min_vel) and np.all(mag <= max_vel)):
        return False
    if not np.all(np.std(history, axis=0) <= max_vel_stdev):
        return False
    unit = history / (np.linalg.norm(history, axis=1, keepdims=True) + 1e-6)
    return bool(np.all(np.dot(unit, unit.T) > 0.95))


def window_geometry(history: np.ndarray, chirp_start_times_us: np.ndarray, frame_period_ms: float) -> np.ndarray:
    """Element positions ``[H, 3, Cv]`` of the window whose velocity history is ``history [H, 3]`` (oldest first).  The newest
    frame ends at the origin; within a frame ``p = 2 t 1e-6 v + start`` (the factor 2: transmitter and receiver both move), and
    the frame before it starts ``2 v period`` further back."""
    H = len(history)
    out = np.empty((H, 3, len(chirp_start_times_us)))
    start = np.zeros(3)
    for f in range(H - 1, -1, -1):
        v = history[f]
        out[f] = (2 * chirp_start_times_us * 1e-6)[None, :] * v[:, None] + start[:, None]
        start = start + 2 * v * (-1 * frame_period_ms * 1e-3)
    return out


class SyntheticArrayBeamformerProcessor(_Processor):
    def __init__(self, config_manager, receiver_idx: int = 0, chirp_cfg_idx: int = 0, num_frames: int = 2, stride: int = 1,
                 az_angle_bins_rad=np.deg2rad(np.linspace(start=-30, stop=30, num=60)), el_angle_bins_rad=np.array([0]),
                 min_vel=np.array([0.17, 0.0, 0.0]), max_vel=np.array([0.25, 0.05, 0.05]),
                 max_vel_stdev=np.array([0.1, 0.1, 0.1]), enable_calibration: bool = False, **kwargs):
        if enable_calibration:
            raise NotImplementedError("SyntheticArrayBeamformerProcessor: array calibration is not part of this build")
        self.receiver_idx, self.chirp_cfg_idx = receiver_idx, chirp_cfg_idx
        self.num_frames, self.stride = num_frames, stride
        self.az_angle_bins_rad, self.el_angle_bins_rad = np.asarray(az_angle_bins_rad), np.asarray(el_angle_bins_rad)
        self.min_vel, self.max_vel, self.max_vel_stdev = np.asarray(min_vel), np.asarray(max_vel), np.asarray(max_vel_stdev)
        self.enable_calibration = False
        self.array_geometry = np.empty(shape=0)
        self.array_geometry_valid = False
        self.beamformed_resp = None
        self._core = None
        super().__init__(config_manager)

    def configure(self):
        cm = self.config_manager
        prof = cm.profile_cfgs[0]
        self.num_range_bins = cm.get_num_adc_samples(profile_idx=0)
        self.range_bins = np.linspace(start=0, stop=cm.range_max_m, num=self.num_range_bins)
        self.lambda_m = SPEED_OF_LIGHT_M_S / (float(prof["startFreq_GHz"]) * 1e9)
        cfgs = np.arange(cm.frameCfg_start_index, cm.frameCfg_end_index + 1)
        self.chirps_per_frame = cm.frameCfg_loops * len(cfgs)
        self.chirp_period_us = prof["idleTime_us"] + prof["rampEndTime_us"]
        self.frame_period_ms = cm.frameCfg_periodicity_ms
        self.chirp_cfg_idxs = np.tile(cfgs, cm.frameCfg_loops)
        # the chirps of this transmitter, every stride-th of them
        mask = np.zeros(self.chirps_per_frame, dtype=bool)
        mask[np.flatnonzero(self.chirp_cfg_idxs == self.chirp_cfg_idx)[::self.stride]] = True
        self.valid_chirps_mask = mask
        # the last chirp of a frame starts at 0, the ones before it earlier
        self.chirp_start_times_us = (np.arange(self.chirps_per_frame - 1, -1, -1) * -self.chirp_period_us)[mask]
        self._core = SyntheticArrayBeamformerCore(self.az_angle_bins_rad, self.el_angle_bins_rad, self.lambda_m, ctx=self._ctx)
        self.d = self._core.d
        self.reset()

    def reset(self):
        self.history_acd_cube_valid_chirps = np.zeros((self.num_frames, self.num_range_bins, int(self.valid_chirps_mask.sum())),
                                                      dtype=complex)
        self.history_avg_vel = np.zeros((self.num_frames, 3), dtype=float)
        self.array_geometry_valid = False
        super().reset()

    def _update_array_geometries(self, current_vel) -> bool:
        hist = self.history_avg_vel
        hist[:-1] = hist[1:].copy()
        hist[-1] = current_vel
        self.array_geometry_valid = gate(hist, self.min_vel, self.max_vel, self.max_vel_stdev)
        self.array_geometry = window_geometry(hist, self.chirp_start_times_us, self.frame_period_ms)
        return self.array_geometry_valid

    def compute_synthetic_response(self, array_geometry: np.ndarray) -> np.ndarray:
        """complex128 ``[S, n_az, n_el]`` of the stored window with element positions ``array_geometry [num_frames, 3, Cv]``."""
        return self._core.compute_synthetic_response(self.history_acd_cube_valid_chirps, array_geometry)

    def compute_array_factor_at_angle(self, array_geometry: np.ndarray, steering_vector: np.ndarray) -> complex:
        """The array factor of ``array_geometry [3, N]`` towards ``steering_vector [3]``: unit signals, no taper (host numpy)."""
        return self._core.compute_array_factor_at_angle(array_geometry, steering_vector)

    def compute_synthetic_array_pattern(self, array_geometry: np.ndarray) -> np.ndarray:
        """The beam pattern float32 ``[n_az, n_el]`` of ``array_geometry [num_frames, 3, Cv]``, normalised to its maximum."""
        return self._core.compute_synthetic_array_pattern(array_geometry)

    def process(self, adc_cube: np.ndarray, current_vel, **kwargs) -> np.ndarray:
        """``adc_cube``: the RAW cube ``[num_rx, S, chirps_per_frame]``.  The image, or ``np.empty(0)`` while the gate is shut."""
        cube = np.asarray(adc_cube)
        if cube.ndim != 3 or cube.shape[1:] != (self.num_range_bins, self.chirps_per_frame):
            raise ValueError(f"expected a raw cube [num_rx, {self.num_range_bins}, {self.chirps_per_frame}], got {cube.shape}")
        hist = self.history_acd_cube_valid_chirps
        hist[:-1] = hist[1:].copy()
        hist[-1] = cube[self.receiver_idx][:, self.valid_chirps_mask]
        if not self._update_array_geometries(np.asarray(current_vel, dtype=float)):
            return np.empty(shape=0)
        self.beamformed_resp = self.compute_synthetic_response(self.array_geometry)
        return self.beamformed_resp


# ---------------------------------------------------------------------------------------------------------------- self-calibration
def calibration_spectra(window: np.ndarray) -> np.ndarray:
    """``Fq [S, E]``: the range spectrum of every element of the window ``[S, E]`` under ``hamming(E)`` (no Hann over the samples)."""
    window = np.asarray(window, dtype=complex)
    return np.fft.fft(np.hamming(window.shape[1])[None, :] * window, axis=0)


def calibration_targets(Fq: np.ndarray, response: np.ndarray):
    """Up to three ``(range row, azimuth bin)`` pairs, strongest range row first: the three largest local maxima (value >= 0) of
    the mean over elements of ``20 log10 |Fq|``, each with the first maximum among the local maxima of ``|10 log10 |response[row,
    :, 0]||`` along azimuth; a row without a local maximum drops out.  Fewer than three range peaks, or a mean that is not finite
    (a window slot of zeros), is "no suitable targets": ``[]`` (the reference indexes three peaks unconditionally and raises
    ``IndexError`` there)."""
    from scipy.signal import find_peaks
    with np.errstate(divide="ignore"):
        avg = np.mean(20 * np.log10(np.abs(Fq)), axis=1)
    if not np.all(np.isfinite(avg)):
        return []
    peaks, _ = find_peaks(avg, height=0)
    if len(peaks) < 3:
        return []
    rows = peaks[np.argsort(avg[peaks])[-3:][::-1]]
    targets = []
    for row in rows:
        with np.errstate(divide="ignore"):
            u = np.abs(10 * np.log10(np.abs(response[row, :, 0])))
        az, _ = find_peaks(u, height=0)
        if len(az):
            targets.append((int(row), int(az[np.argmax(u[az])])))
    return targets


def calibrated_geometry(Fq: np.ndarray, P: np.ndarray, targets, d: np.ndarray, lambda_m: float) -> np.ndarray:
    """``Pcal [3, E]``: per target the phase history of its range row steered to its direction, the unwrapped phase steps between
    neighbouring elements, then per step the least-squares x / y displacement that explains the three steps
    (``lstsq`` on ``(2 pi / lambda) d[0:2]`` of the targets, minimum norm when rank deficient) and its running sum taken off
    ``P[0:2, 1:]``.  z is left alone."""
    steer = np.array([d[:, a, 0] for _, a in targets])                                      # [3 targets, 3]
    steps = np.stack([np.diff(np.unwrap(np.angle(Fq[r] * np.exp(2j * np.pi * (steer[t] @ P) / lambda_m))))
                      for t, (r, _) in enumerate(targets)])                                 # [3, E - 1]
    delta = np.linalg.lstsq(2 * np.pi / lambda_m * steer[:, 0:2], steps, rcond=None)[0]      # [2, E - 1]
    out = np.array(P, dtype=float)
    out[0:2, 1:] -= np.cumsum(delta, axis=1)
    return out


def calibrate_window(window: np.ndarray, P: np.ndarray, d: np.ndarray, lambda_m: float, num_iters: int, response: np.ndarray,
                     contract):
    """The calibration loop on one window ``[S, E]`` with geometry ``P [3, E]`` and uncalibrated image ``response [S, n_az, n_el]``;
    ``contract(P)`` returns the image for a geometry.  Returns ``(response, Pcal, targets, status)``.  Two quirks of the reference
    are kept: every iteration starts again from the UNCALIBRATED ``P`` (only the azimuth picks read the latest image, so
    corrections do not accumulate), and an iteration that ends with fewer than three targets stops the loop, makes the calibrated
    geometry the uncalibrated one and leaves the response of the iteration before."""
    Fq = calibration_spectra(window)
    Pcal, kept, status = np.array(P, dtype=float), [], 0
    for _ in range(int(num_iters)):
        targets = calibration_targets(Fq, response)
        if len(targets) < 3:
            Pcal = np.array(P, dtype=float)
            break
        Pcal = calibrated_geometry(Fq, P, targets, d, lambda_m)
        response = contract(Pcal)
        kept, status = targets, status + 1
    return response, Pcal, kept, status


class SelfCalibratingSyntheticArrayProcessor(SyntheticArrayBeamformerProcessor):
    """``SyntheticArrayBeamformerProcessor`` with the reference's ``enable_calibration=True``: ``process`` returns the response of
    the calibrated geometry.  After a valid frame ``array_geometry_calibrated [num_frames, 3, Cv]``, ``calibration_targets`` (the
    picks of the last iteration that found three) and ``calibration_status`` (iterations that applied a correction) are set.  The
    calibration runs in float64 numpy on the host history; the contractions go through ``SyntheticArrayBeamformerCore.contract``."""

    def __init__(self, config_manager, *args, num_calibration_iters: int = 1, **kwargs):
        if kwargs.pop("enable_calibration", True) is not True:
            raise ValueError("SelfCalibratingSyntheticArrayProcessor calibrates: use SyntheticArrayBeamformerProcessor without")
        if int(num_calibration_iters) < 1:
            raise ValueError(f"num_calibration_iters is {num_calibration_iters}")
        self.num_calibration_iters = int(num_calibration_iters)
        self.array_geometry_calibrated = np.empty(shape=0)
        self.calibration_targets, self.calibration_status = [], 0
        super().__init__(config_manager, *args, enable_calibration=False, **kwargs)

    def process(self, adc_cube: np.ndarray, current_vel, **kwargs) -> np.ndarray:
        resp = super().process(adc_cube, current_vel, **kwargs)
        if not self.array_geometry_valid:
            return resp
        hist = self.history_acd_cube_valid_chirps
        window = hist.transpose(1, 0, 2).reshape(hist.shape[1], -1)
        H = self.num_frames
        P = self.array_geometry.transpose(1, 0, 2).reshape(3, -1)
        contract = lambda g: self.compute_synthetic_response(g.reshape(3, H, -1).transpose(1, 0, 2))       # noqa: E731
        resp, Pcal, self.calibration_targets, self.calibration_status = calibrate_window(
            window, P, self.d, self.lambda_m, self.num_calibration_iters, resp, contract)
        self.array_geometry_calibrated = Pcal.reshape(3, H, -1).transpose(1, 0, 2)
        self.beamformed_resp = resp
        return resp
