"""Range to ground from the chirp-0 range profile, tracked from frame to frame.

Behaviour pinned on sequences run by the reference (mmwave_radar_processing/processors/altimeter.py, fixtures
``tests/golden/detectors_rd.npz: ground_*``; a restatement of the reference's control flow exists only in the test
infrastructure).  Here the tracker is a small state machine:

* ``GroundLock`` holds the gate (lowest admissible range, how far a new measurement may lie from the last one) and the
  two altitudes the callers read;
* a frame is a list of *look stages* -- coarse profile, then optionally a zoom around the coarse hit -- each turning the
  cube into candidate ranges on the device (float64 range profile / chirp-z zoom) + one scipy peak pick on the host;
* ``GroundLock.step`` is the one statement of the rules: the coarse candidates pass the gate, the zoom around the admitted
  one (if any) passes it again; no admissible candidate at a stage ends the frame with the previous altitude, the last
  stage's hit is accepted.  ``GroundLock.advance`` runs the same step over a sequence of frames whose candidate lists were
  computed beforehand (the zoom candidates of EVERY coarse candidate): that is how ``batch.FramePipeline(ground=...)``
  tracks F frames after one batched device pass, on plain floats.

STATEFUL: one instance per frame sequence; the batch pipeline carries this lock from call to call.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from .. import _lib
from .range_resp import RangeProcessor


@dataclass
class GroundLock:
    floor_m: float                      # nothing nearer than this is ground
    reach_m: float                      # a new measurement lies within this of the last one
    bias_m: float = 0.0                 # added to what is reported, never to the gate
    measured_m: float = field(init=False)
    reported_m: float = field(init=False)

    def __post_init__(self):
        self.measured_m = self.reported_m = self.floor_m

    def pick(self, candidates_m: Sequence[float]) -> Optional[int]:
        """Position of the nearest candidate inside the gate (the first of equal ones), or None.  Plain float arithmetic:
        the same IEEE operations as the NumPy expression of the reference, without its per-call overhead."""
        floor, last, reach = self.floor_m, self.measured_m, self.reach_m
        best = None
        for i, c in enumerate(candidates_m):
            if c >= floor and abs(c - last) <= reach and (best is None or c < candidates_m[best]):
                best = i
        return best

    def admit(self, candidates_m) -> Optional[float]:
        """The nearest candidate inside the gate, or None."""
        c = [float(x) for x in np.ravel(candidates_m)]
        i = self.pick(c)
        return None if i is None else c[i]

    def step(self, coarse_m: Sequence[float], refine: Optional[Callable[[int], Sequence[float]]] = None) -> float:
        """One frame: the admitted coarse candidate, then (``refine`` given: the precise mode) the admitted one of
        ``refine(position of that coarse candidate)``; the last hit is accepted.  Returns the reported altitude."""
        i = self.pick(coarse_m)
        if i is None:
            return self.reported_m
        hit = coarse_m[i]
        if refine is not None:
            fine = refine(i)
            j = self.pick(fine)
            if j is None:
                return self.reported_m
            hit = fine[j]
        self.accept(float(hit))
        return self.reported_m

    def advance(self, coarse_per_frame: Sequence[Sequence[float]],
                fine_per_frame: Optional[Sequence[Sequence[Sequence[float]]]] = None) -> List[float]:
        """``step`` over a frame sequence whose candidates are known up front: ``fine_per_frame[f][i]`` is the zoom
        candidate list around ``coarse_per_frame[f][i]``.  Returns the reported altitude after every frame."""
        if fine_per_frame is None:
            return [self.step(coarse) for coarse in coarse_per_frame]
        return [self.step(coarse, fine.__getitem__) for coarse, fine in zip(coarse_per_frame, fine_per_frame)]

    def accept(self, range_m: float) -> None:
        self.measured_m = range_m
        self.reported_m = range_m + self.bias_m

    def release(self) -> None:
        """Forget the last measurement (the gate re-centres on the floor); the reported altitude stands until the next
        accepted frame, which is what the reference's reset leaves behind."""
        self.measured_m = self.floor_m


class Altimeter(RangeProcessor):
    def __init__(self, config_manager, min_altitude_m: float, zoom_search_region_m: float, altitude_search_limit_m: float,
                 range_bias: float = 0.0, **kwargs) -> None:
        super().__init__(config_manager)
        self.lock = GroundLock(float(min_altitude_m), float(altitude_search_limit_m), float(range_bias))
        self.zoom_half_width_m = float(zoom_search_region_m)
        self.coarse_fft_data = None

    # the names callers of the reference class read ---------------------------------------------------------------
    current_altitude_measured_m = property(lambda self: self.lock.measured_m)
    current_altitude_corrected_m = property(lambda self: self.lock.reported_m)
    min_altitude_m = property(lambda self: self.lock.floor_m)
    altitude_search_limit_m = property(lambda self: self.lock.reach_m)
    range_bias = property(lambda self: self.lock.bias_m)
    zoom_search_region_m = property(lambda self: self.zoom_half_width_m)

    def find_ground_peak(self, detected_peaks_m: np.ndarray) -> float:
        hit = self.lock.admit(detected_peaks_m)
        return -1.0 if hit is None else hit

    def reset(self):
        self.lock.release()
        return super().reset()

    # look stages: (cube, previous hit) -> candidate ranges ---------------------------------------------------------
    def _look_coarse(self, adc_cube: np.ndarray, _prev) -> np.ndarray:
        # float64 on the device: the 6-dB prominence test then sees the reference's numbers to ~1e-15
        ctx, bufs, d_cube, (V, S, C) = self._upload_cube(adc_cube)
        d_prof = bufs.get("profile64", S * 8)
        _lib.check(ctx.lib.mmw_range_profile_f64(ctx.handle, d_cube.ptr, d_prof.ptr, 1, V, S, C, 0))
        self.coarse_fft_data = d_prof.download((S,), np.float64)
        return self.find_peaks(20 * np.log10(self.coarse_fft_data), self.range_bins, max_peaks=3)[0]

    def _look_zoom(self, adc_cube: np.ndarray, prev_m: float) -> np.ndarray:
        lo = max(1e-6, prev_m - self.zoom_half_width_m)
        hi = min(self.range_bins.max() - 1e-6, prev_m + self.zoom_half_width_m)
        spectrum, bins = self.zoom_fft(adc_cube, lo, hi, 0)
        return self.find_peaks(20 * np.log10(spectrum), bins, max_peaks=2)[0]

    def process(self, adc_cube: np.ndarray, precise_est_enabled: bool = True, **kwargs) -> float:
        coarse = self._look_coarse(adc_cube, None).tolist()
        refine = (lambda i: self._look_zoom(adc_cube, coarse[i]).tolist()) if precise_est_enabled else None
        return self.lock.step(coarse, refine)
