"""Strip-map SAR slice of one antenna (reference: mmwave_radar_processing/processors/strip_map_SAR_processor.py:8-194).

A moving platform turns the chirps of a frame into a synthetic aperture along its track: the Doppler axis of the un-windowed
range-Doppler plane of ONE antenna is an azimuth axis whose scale depends on the platform speed.  ``process`` returns the part of
``fftshift(fft2(cube[rx]), axes=1)`` between the sensor height and ``max_SAR_distance`` in range and between the two angles of
``az_angle_range_rad`` in azimuth -- a few dozen rows by a speed-dependent handful of columns.  ``mmw_sar_slices`` computes only
that window on the device; which window it is, and the ground-plane bins and meshes the plotters read, is pure host arithmetic
in float64 and lives in ``strip_map_geometry`` -- ``FramePipeline.strip_map_sar`` calls the same function for every resident frame.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import numpy as np
import scipy.constants as constants

from .. import _lib
from ._processor import _Processor
from .virtual_array_reformater import VirtualArrayReformatter


class StripMapGeometry(NamedTuple):
    """What one (speed, height, distance) setting fixes.  The slices are end-exclusive, as the reference's are."""
    valid_ranges_slice: slice
    valid_angles_slice: slice
    angle_bins_rad: np.ndarray
    ground_range_bins: np.ndarray
    ground_az_bins_rad: np.ndarray
    thetas: Optional[np.ndarray]
    rhos: Optional[np.ndarray]
    x_s: Optional[np.ndarray]
    y_s: Optional[np.ndarray]


def strip_map_geometry(vel_m_per_s, sensor_height_m, max_SAR_distance, az_angle_range_rad, *, phase_shifts, lambda_m,
                       chirp_period_us, range_bins, meshes: bool = True) -> StripMapGeometry:
    """The window and the ground-plane tables of the reference's ``configure_array_geometry`` (:108-158), as a function of its
    inputs alone.  Every expression is the reference's, so its oddities come out the same: the angle bins are
    ``arcsin(phase * lambda) / (2 pi d_rx)`` with ``d_rx`` the two-way platform step per chirp, both slices leave their last
    index out, a height above every range bin (or a distance below all of them) is the ``IndexError`` of indexing an empty
    ``np.nonzero``, and a zero or non-finite speed gives whatever NumPy makes of the division (infinities and NaNs, whose
    ``argmin`` is NumPy's too).  ``meshes=False`` leaves the four plotting grids out (the batch form needs the slices only)."""
    with np.errstate(all="ignore"):
        step = 2 * chirp_period_us * 1e-6 * vel_m_per_s                     # tx and rx both move
        angle_bins = np.arcsin(phase_shifts * lambda_m) / (2 * np.pi * step)
        ends = [np.argmin(np.abs(angle_bins - edge(az_angle_range_rad))) for edge in (np.min, np.max)]
        az = slice(np.min(ends), np.max(ends))
        above = np.nonzero(range_bins > sensor_height_m)[0]
        below = np.nonzero(range_bins < max_SAR_distance)[0]
        rng = slice(above[0], below[-1])                                    # IndexError when either set is empty
        ground_range = np.sqrt(np.power(range_bins[rng], 2) - np.power(step, 2))
        ground_az = angle_bins[az]
        thetas = rhos = x_s = y_s = None
        if meshes:
            thetas, rhos = np.meshgrid(ground_az, ground_range, indexing="xy")
            x_s, y_s = np.multiply(rhos, np.cos(thetas)), np.multiply(rhos, np.sin(thetas))
    return StripMapGeometry(rng, az, angle_bins, ground_range, ground_az, thetas, rhos, x_s, y_s)


def slice_window(geom: StripMapGeometry, S: int, C: int) -> Tuple[int, int, int, int]:
    """(row_lo, row_hi, col_lo, col_hi), half open, of ``plane[valid_ranges_slice, valid_angles_slice]`` on an ``S x C`` plane:
    NumPy's own clipping of a slice, with a reversed slice (height beyond the distance) as the empty window it is."""
    r_lo, r_hi, _ = geom.valid_ranges_slice.indices(S)
    c_lo, c_hi, _ = geom.valid_angles_slice.indices(C)
    return r_lo, max(r_hi, r_lo), c_lo, max(c_hi, c_lo)


def pack_windows(windows) -> Tuple[np.ndarray, np.ndarray]:
    """int32 ``[F, 4]`` windows and the int64 ``[F + 1]`` element offsets of their blocks packed back to back."""
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 4))
    off = np.zeros(len(win) + 1, dtype=np.int64)
    np.cumsum((win[:, 1] - win[:, 0]).astype(np.int64) * (win[:, 3] - win[:, 2]), out=off[1:])
    return win, off


def frame_windows(proc, velocities, sensor_height_m, max_SAR_distance, S: int, C: int) -> Tuple[np.ndarray, np.ndarray]:
    """``pack_windows`` of the windows ``proc.process`` would keep at each speed of the float64 vector ``velocities``: the
    processor's own geometry function, once per distinct speed.  Distinct by bit pattern -- a NaN is never equal to itself and
    -0.0 equals 0.0, yet each has to find its own window again."""
    vel = np.ascontiguousarray(velocities, dtype=np.float64)
    keys, seen = vel.view(np.int64).tolist(), {}
    for key, v in zip(keys, vel.tolist()):
        if key not in seen:
            seen[key] = slice_window(proc.geometry(v, sensor_height_m, max_SAR_distance, meshes=False), S, C)
    return pack_windows([seen[key] for key in keys] if keys else np.zeros((0, 4)))


def sar_slices_call(ctx, d_cubes_ptr, n_frames, V, S, C, rx, win, off, d_out_ptr) -> None:
    _lib.check(ctx.lib.mmw_sar_slices(ctx.handle, d_cubes_ptr, int(n_frames), V, S, C, int(rx),
                                      win.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), d_out_ptr))


class StripMapSARProcessor(_Processor):
    def __init__(self, config_manager, az_angle_range_rad=np.deg2rad(np.array([-30, 30])), **kwargs):
        self.az_angle_range_rad = np.array(az_angle_range_rad) if isinstance(az_angle_range_rad, list) else az_angle_range_rad
        if config_manager.virtual_antennas_enabled:
            self.virtual_array_reformatter = VirtualArrayReformatter(config_manager)
        self.chirps_per_frame = self.chirp_period_us = self.lambda_m = None
        self.chirp_tx_masks = self.chirp_rx_positions_m = None              # declared by the reference, never filled
        self.phase_shifts = self.angle_bins_rad = None
        self.num_range_bins = self.radar_range_bins = self.range_bins = None
        self.valid_ranges_slice = self.valid_angles_slice = None
        self.ground_range_bins = self.ground_az_bins_rad = None
        self.thetas = self.rhos = self.x_s = self.y_s = None
        super().__init__(config_manager)

    def configure(self):
        self._compute_key_radar_parameters()

    def _compute_key_radar_parameters(self):
        cm = self.config_manager
        profile = cm.profile_cfgs[0]
        self.num_range_bins = cm.get_num_adc_samples(profile_idx=0)
        self.range_bins = np.linspace(start=0, stop=cm.range_max_m, num=self.num_range_bins)
        self.lambda_m = constants.c / (float(profile["startFreq_GHz"]) * 1e9)
        self.chirps_per_frame = cm.frameCfg_loops * (cm.frameCfg_end_index - cm.frameCfg_start_index + 1)
        self.phase_shifts = np.linspace(start=np.pi, stop=-np.pi, num=cm.frameCfg_loops)     # one per loop, not per chirp
        self.chirp_period_us = profile["idleTime_us"] + profile["rampEndTime_us"]

    def geometry(self, vel_m_per_s, sensor_height_m=0.24, max_SAR_distance=1.5, meshes: bool = True) -> StripMapGeometry:
        """``strip_map_geometry`` on this processor's tables; changes nothing."""
        return strip_map_geometry(vel_m_per_s, sensor_height_m, max_SAR_distance, self.az_angle_range_rad,
                                  phase_shifts=self.phase_shifts, lambda_m=self.lambda_m, chirp_period_us=self.chirp_period_us,
                                  range_bins=self.range_bins, meshes=meshes)

    def configure_array_geometry(self, vel_m_per_s: float, sensor_height_m: float, max_SAR_distance: float):
        g = self.geometry(vel_m_per_s, sensor_height_m, max_SAR_distance)
        (self.valid_ranges_slice, self.valid_angles_slice, self.angle_bins_rad, self.ground_range_bins, self.ground_az_bins_rad,
         self.thetas, self.rhos, self.x_s, self.y_s) = g
        return g

    def process(self, adc_cube, vel_m_per_s: float, sensor_height_m: float = 0.24, rx_index=0, max_SAR_distance: float = 1.5,
                **kwargs) -> np.ndarray:
        if self.config_manager.virtual_antennas_enabled:
            adc_cube = self.virtual_array_reformatter.process(adc_cube=adc_cube)
        g = self.configure_array_geometry(vel_m_per_s, sensor_height_m, max_SAR_distance)
        shape = np.shape(adc_cube)
        if len(shape) != 3:
            raise ValueError("adc_cube must be (rx antennas) x (adc samples) x (chirps)")
        V, S, C = shape
        rx = int(rx_index)
        if not -V <= rx < V:
            raise IndexError(f"rx_index {rx_index} is out of bounds for {V} antennas")
        win, off = pack_windows([slice_window(g, S, C)])
        r_lo, r_hi, c_lo, c_hi = (int(v) for v in win[0])
        if off[1] == 0:
            return np.zeros((r_hi - r_lo, c_hi - c_lo), dtype=np.complex128)
        ctx, bufs, d_cube, _ = self._upload_cube(adc_cube)
        d_out = bufs.get("sar_slice", int(off[1]) * 8)
        sar_slices_call(ctx, d_cube.ptr, 1, V, S, C, rx % V, win, off, d_out.ptr)
        return d_out.download((r_hi - r_lo, c_hi - c_lo), np.complex64).astype(np.complex128)
