"""Micro-Doppler spectrogram (reference: mmwave_radar_processing/processors/micro_doppler_resp.py:6-114).

A frame contributes one row: the un-windowed range-Doppler magnitude of one antenna, reduced with ``max`` over the range rows of
a window.  ``mmw_micro_doppler`` computes only those rows on the device (a partial DFT over fast time); the spectrogram itself is
the last ``num_frames_history`` rows kept on the host, newest first.  ``FramePipeline.micro_doppler`` makes the rows of a whole
resident batch with the same kernel, ``batch.micro_doppler_history`` stacks them into this buffer.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ._processor import _Processor


def window_rows(range_bins: np.ndarray, target_ranges) -> tuple:
    """(mask, row_lo, row_hi): the range rows with ``target_ranges[0] <= range <= target_ranges[1]``.  The bins ascend, so the
    mask is one contiguous run; a window that holds no bin (both ends between two bins, or reversed) is a ValueError here --
    the reference fails on it later, inside ``np.max`` of an empty slice."""
    lo_m, hi_m = (float(v) for v in np.asarray(target_ranges, dtype=np.float64).ravel()[:2])
    mask = (range_bins >= lo_m) & (range_bins <= hi_m)
    rows = np.flatnonzero(mask)
    if rows.size == 0:
        raise ValueError(f"target_ranges [{lo_m}, {hi_m}] m hold no range bin (bins are {range_bins[1] - range_bins[0]:.4g} m "
                         "apart)" if len(range_bins) > 1 else f"target_ranges [{lo_m}, {hi_m}] m hold no range bin")
    return mask, int(rows[0]), int(rows[-1])


def shifted_bin(c, C: int):
    """FFT bin behind column ``c`` of ``np.fft.fftshift`` over an axis of length ``C`` (odd ``C`` too)."""
    return (c + C - C // 2) % C


class MicroDopplerProcessor(_Processor):
    def __init__(self, config_manager, target_ranges=[0, 1.0], num_frames_history: int = 20, **kwargs):
        self.target_ranges = np.array(target_ranges) if isinstance(target_ranges, list) else target_ranges
        self.num_frames_history = num_frames_history
        self.vel_bins = self.range_bins = self.time_bins = None
        self.range_bin_idxs_to_keep = None
        self.micro_doppler_resp = None
        self.rows = (0, 0)              # (row_lo, row_hi) of the window: what the kernel is given
        super().__init__(config_manager)

    def configure(self):
        cm, H = self.config_manager, self.num_frames_history
        self.vel_bins = np.arange(-1 * cm.vel_max_m_s, cm.vel_max_m_s - cm.vel_res_m_s + 1e-3, cm.vel_res_m_s)
        self.range_bins = np.arange(0, cm.range_max_m - cm.range_res_m / 2 + 1e-3, cm.range_res_m)
        mask, lo, hi = window_rows(self.range_bins, self.target_ranges)
        self.range_bin_idxs_to_keep, self.rows = mask.astype(np.bool_), (lo, hi)
        self.time_bins = np.linspace(0, H * (cm.frameCfg_periodicity_ms * 1e-3), H)
        self.micro_doppler_resp = np.zeros((len(self.vel_bins), H))

    def reset(self):
        self.micro_doppler_resp = np.zeros((len(self.vel_bins), self.num_frames_history))
        super().reset()

    def push(self, row: np.ndarray) -> np.ndarray:
        """Age every column of the spectrogram by one frame and put ``row`` in front (pure host code)."""
        row = np.asarray(row, dtype=np.float64)
        if row.shape != (self.micro_doppler_resp.shape[0],):
            raise ValueError(f"a micro-Doppler row has {self.micro_doppler_resp.shape[0]} velocity bins, got shape {row.shape}")
        buf = self.micro_doppler_resp
        if buf.shape[1]:
            buf[:, 1:] = buf[:, :-1].copy()
            buf[:, 0] = row
        return buf

    def row(self, adc_cube: np.ndarray, rx_idx: int = 0) -> np.ndarray:
        """The frame's row, float64 ``(len(vel_bins),)``, without touching the spectrogram."""
        shape = np.shape(adc_cube)
        if len(shape) == 3 and shape[1:] != (len(self.range_bins), len(self.vel_bins)):
            raise ValueError(f"cube of {shape[1]} samples x {shape[2]} chirps does not match the configuration's "
                             f"{len(self.range_bins)} range bins x {len(self.vel_bins)} velocity bins")
        rx = int(rx_idx)
        if len(shape) == 3 and not -shape[0] <= rx < shape[0]:
            raise IndexError(f"rx_idx {rx_idx} is out of bounds for {shape[0]} antennas")
        ctx, bufs, d_cube, (V, S, C) = self._upload_cube(adc_cube)
        d_out = bufs.get("micro_doppler", C * 4)
        _lib.check(ctx.lib.mmw_micro_doppler(ctx.handle, d_cube.ptr, d_out.ptr, 1, V, S, C, rx % V, *self.rows))
        return d_out.download((C,), np.float32).astype(np.float64)

    def process(self, adc_cube: np.ndarray, rx_idx=0, **kwargs) -> np.ndarray:
        return self.push(self.row(adc_cube, rx_idx))
