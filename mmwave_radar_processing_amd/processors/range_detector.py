"""Range profile followed by a 1-D CFAR (reference: mmwave_radar_processing/processors/range_detector.py:11-98; the
``range_detector`` key of the GUI's processor registry).

The stock detectors run as one ``mmw_range_detect`` call: the float64 range profile of chirp 0, the thresholds of
``mmw_cfar1d`` and the ordered hit list, without the profile making a round trip through the host.  A detector the device
cannot stand in for -- a user's subclass, or one whose ``_compute_thresholds`` is its own -- gets the float64 profile on the
host and runs its own ``detect``, as the reference would.  ``FramePipeline.range_detections`` is the batch form.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import _lib
from ..detectors.base import BaseCFAR1D
from ..detectors.detector_registry import get_detector_registry, make_detector
from .range_resp import RangeProcessor


def device_cfar1d_args(det):
    """(kind, num_train, num_guard, scale, k_rank) when ``det`` is one of the registry's own 1-D CFAR classes with the stock
    threshold code, else None: only those are what ``cfar1d_threshold`` computes on the device."""
    stock = [cls for cls in get_detector_registry().values() if issubclass(cls, BaseCFAR1D)]
    if type(det) not in stock or type(det)._compute_thresholds is not BaseCFAR1D._compute_thresholds:
        return None
    return int(det.kind), int(det.num_train), int(det.num_guard), float(det._scale()), int(det._k_rank())


class RangeDetector(RangeProcessor):
    def __init__(self, config_manager, cfar_type: str = "os_cfar_1d", cfar_params: dict = {}, **kwargs):
        self.cfar_detector = make_detector(cfar_type, cfar_params)       # ValueError naming the registry's keys
        self.dets: Optional[np.ndarray] = None
        self.thresholds: Optional[np.ndarray] = None
        self.range_resp: Optional[np.ndarray] = None
        super().__init__(config_manager)
        self.logger.info(f"RangeDetector initialized with CFAR type: {cfar_type}")

    def profile64(self, adc_cube, chirp_idx: int = 0) -> np.ndarray:
        """The float64 range profile (``mmw_range_profile_f64``), what the reference's ``RangeProcessor.process`` returns."""
        ctx, bufs, d_cube, (V, S, C) = self._upload_cube(adc_cube)
        d_prof = bufs.get("profile64", S * 8)
        _lib.check(ctx.lib.mmw_range_profile_f64(ctx.handle, d_cube.ptr, d_prof.ptr, 1, V, S, C, int(chirp_idx)))
        return d_prof.download((S,), np.float64)

    def process(self, adc_cube: np.ndarray, **kwargs) -> np.ndarray:
        args = device_cfar1d_args(self.cfar_detector)
        if args is None:
            self.range_resp = self.profile64(adc_cube)
            idxs = self.cfar_detector.detect(self.range_resp)
            self.thresholds = self.cfar_detector.thresholds
        else:
            ctx, bufs, d_cube, (V, S, C) = self._upload_cube(adc_cube)
            d_prof, d_thr = bufs.get("profile64", S * 8), bufs.get("thr64", S * 8)
            d_dets, d_cnt = bufs.get("range_dets", S * 4), bufs.get("range_count", 4)
            kind, T, G, scale, k = args
            _lib.check(ctx.lib.mmw_range_detect(ctx.handle, d_cube.ptr, 1, V, S, C, 0, kind, T, G, scale, k, d_prof.ptr, d_thr.ptr,
                                                d_dets.ptr, d_cnt.ptr, S))
            self.range_resp = d_prof.download((S,), np.float64)
            self.thresholds = d_thr.download((S,), np.float64)
            n = int(d_cnt.download((1,), np.int32)[0])
            idxs = d_dets.download((S,), np.int32)[:n].tolist()
            det = self.cfar_detector                                     # the caches detect() leaves behind
            det.thresholds, det.detections = self.thresholds, self.range_resp > self.thresholds
        self.dets = np.array(idxs) if len(idxs) > 0 else np.array([])
        return self.dets

    def _map_detections_to_bins(self, dets: np.ndarray) -> np.ndarray:
        if self.range_bins is None:
            raise ValueError("Range bins are not configured.")
        return self.range_bins[dets]
