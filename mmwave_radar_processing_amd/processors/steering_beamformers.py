"""Steering-matrix beamformers on the MI355X matrix cores.

``SyntheticArrayBeamformerCore`` is the dense contraction of the reference's
``SyntheticArrayBeamformerProcessor`` (mmwave_radar_processing/processors/
simple_synthetic_array_beamformer_processor_multiFrame.py:474-585): steering directions, Hamming over array
elements, phase-steer-and-sum, Hann over samples, range FFT.  The velocity-history / geometry bookkeeping
around it is sequential host state that SURVEY.md keeps out of scope; callers hand in the stacked history
``[frames, S, chirps]`` and geometry ``[frames, 3, chirps]`` exactly as the reference stores them.

``CaponBeamformer`` is the MVDR spectrum BASELINE.json config 4 asks for.  The reference has NO Capon code
(SURVEY.md F2): the definition is this build's own and its parity is "unpinned".
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib


class SyntheticArrayBeamformerCore:
    def __init__(self, az_angle_bins_rad, el_angle_bins_rad, lambda_m: float, ctx: _lib.Context = None):
        self.az_angle_bins_rad = np.asarray(az_angle_bins_rad, dtype=float)
        self.el_angle_bins_rad = np.asarray(el_angle_bins_rad, dtype=float)
        self.lambda_m = float(lambda_m)
        self._compute_beam_stearing_vectors()
        self._ctx = ctx
        self._bufs = None
        self.beamformed_resp = None

    def _compute_beam_stearing_vectors(self):
        """d[3, n_az, n_el] unit pointing vectors (reference :474-488)."""
        thetas, phis = np.meshgrid(self.az_angle_bins_rad, self.el_angle_bins_rad, indexing="ij")
        self.d = np.array([np.cos(thetas) * np.cos(phis), np.sin(thetas) * np.cos(phis), np.sin(phis)])

    def _device(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        if self._bufs is None:
            self._bufs = _lib.BufferSet(self._ctx)
        return self._ctx, self._bufs

    def compute_synthetic_response(self, history_adc_cube: np.ndarray, array_geometry: np.ndarray) -> np.ndarray:
        """history ``[frames, S, chirps]`` complex, geometry ``[frames, 3, chirps]`` -> complex128 ``[S, n_az, n_el]``."""
        hist = np.asarray(history_adc_cube)
        geom = np.asarray(array_geometry, dtype=np.float64)
        if hist.ndim == 2:      # already [S, E]
            X, P = hist, geom.reshape(3, -1)
        else:
            X = hist.transpose((1, 0, 2)).reshape(hist.shape[1], -1)        # [S, E]  (:551-555)
            P = geom.transpose((1, 0, 2)).reshape(3, -1)                    # [3, E]  (:558-559)
        return self.contract(X, P)

    def contract(self, X_se: np.ndarray, P_3e: np.ndarray) -> np.ndarray:
        """``X [S, E]`` with geometry ``P [3, E]`` -> ``[S, n_az, n_el]``; a batch ``X [F, S, E]``, ``P [F, 3, E]`` (every
        frame its own synthetic-array geometry) -> ``[F, S, n_az, n_el]`` in one launch group."""
        ctx, bufs = self._device()
        X = np.ascontiguousarray(X_se, dtype=np.complex64)
        P = np.ascontiguousarray(P_3e, dtype=np.float64)
        single = X.ndim == 2
        if single:
            X, P = X[None], P[None]
        if X.ndim != 3 or P.ndim != 3:
            raise ValueError("expected X [S, E] / P [3, E] or X [F, S, E] / P [F, 3, E]")
        F, S, E = X.shape
        if P.shape != (F, 3, E):
            raise ValueError(f"array geometry {P.shape} does not match {F} frames x {E} elements")
        dirs = np.ascontiguousarray(self.d.reshape(3, -1), dtype=np.float64)
        T = dirs.shape[1]
        d_X, d_P, d_D = bufs.get("bf_x", X.nbytes), bufs.get("bf_p", P.nbytes), bufs.get("bf_d", dirs.nbytes)
        d_Y = bufs.get("bf_y", F * S * T * 8)
        d_X.upload(X)
        d_P.upload(P)
        d_D.upload(dirs)
        _lib.check(ctx.lib.mmw_bartlett(ctx.handle, d_X.ptr, d_P.ptr, d_D.ptr, d_Y.ptr, F, S, E, T, self.lambda_m))
        out = d_Y.download((F, S, T), np.complex64).astype(np.complex128).reshape(F, S, self.d.shape[1], self.d.shape[2])
        self.beamformed_resp = out[0] if single else out
        return self.beamformed_resp

    def compute_array_factor_at_angle(self, array_geometry: np.ndarray, steering_vector: np.ndarray) -> complex:
        """The array factor of ``array_geometry [3, N]`` towards ``steering_vector [3]`` with unit signals at every element
        (reference :615-640).  One direction: plain numpy on the host."""
        return np.sum(np.exp(1j * 2 * np.pi * (np.asarray(steering_vector) @ np.asarray(array_geometry)) / self.lambda_m))

    def compute_synthetic_array_pattern(self, array_geometry: np.ndarray) -> np.ndarray:
        """The beam pattern float32 ``[n_az, n_el]`` of ``array_geometry [frames, 3, chirps]``: ``|array factor|`` over the
        steering grid, normalised to its maximum (reference :642-670), one ``mmw_synth_array_pattern`` call."""
        geom = np.asarray(array_geometry, dtype=np.float64)
        if geom.ndim != 3 or geom.shape[1] != 3:
            raise ValueError(f"compute_synthetic_array_pattern: array_geometry must be [frames, 3, chirps], got {geom.shape}")
        P = geom.transpose((1, 0, 2)).reshape(1, 3, -1)
        return array_patterns(P, self.d, self.lambda_m, ctx=self._ctx)[0]


def array_pattern_args(P, d, lambda_m, what: str = "array_patterns"):
    """The argument checks of ``array_patterns`` (no device is touched): ``(P float64 [n, 3, E], d float64 [3, n_az, n_el],
    lambda_m)``."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim != 3 or P.shape[1] != 3 or P.shape[2] < 1:
        raise ValueError(f"{what}: P must be [n, 3, E] element positions with E >= 1, got {P.shape}")
    d = np.ascontiguousarray(d, dtype=np.float64)
    if d.ndim != 3 or d.shape[0] != 3 or d.shape[1] < 1 or d.shape[2] < 1:
        raise ValueError(f"{what}: d must be [3, n_az, n_el] steering directions, got {d.shape}")
    lam = float(lambda_m)
    if not (lam > 0 and np.isfinite(lam)):
        raise ValueError(f"{what}: lambda_m {lambda_m} is not a positive finite wavelength")
    if P.shape[0] * d.shape[1] * d.shape[2] >= 2**31 or P.shape[0] * 3 * P.shape[2] >= 2**31:
        raise ValueError(f"{what}: P {P.shape} with {d.shape[1]} x {d.shape[2]} directions is beyond int32 entries: split the frames")
    return P, d, lam


def array_patterns_on(ctx: _lib.Context, d_P_ptr: int, n: int, E: int, d: np.ndarray, lam: float, d_pattern: _lib.DeviceBuffer,
                      d_af: _lib.DeviceBuffer = None) -> None:
    """``mmw_synth_array_pattern`` on a geometry table already in HBM (``d_P_ptr``: ``[n][3][E]`` float64)."""
    dirs = np.ascontiguousarray(d.reshape(3, -1))
    _lib.check(ctx.lib.mmw_synth_array_pattern(ctx.handle, d_P_ptr, n, E, dirs.ctypes.data_as(C.POINTER(C.c_double)), dirs.shape[1],
                                               lam, d_pattern.ptr, d_af.ptr if d_af is not None else None))


def array_patterns(P, d, lambda_m, ctx: _lib.Context = None, with_factor: bool = False):
    """Beam patterns float32 ``[n, n_az, n_el]`` of the geometries ``P [n, 3, E]`` (element positions, the layout of
    ``batch.synthetic_array_geometry``) over the directions ``d [3, n_az, n_el]``: per frame ``|sum_e exp(j 2 pi d . p_e /
    lambda)|`` rounded to float32 and divided by its maximum -- the reference's ``compute_synthetic_array_pattern`` for every
    frame in one ``mmw_synth_array_pattern`` call.  ``with_factor=True``: ``(patterns, factors)`` with the un-normalised
    complex128 array factors ``[n, n_az, n_el]``."""
    P, d, lam = array_pattern_args(P, d, lambda_m)
    n, E, (n_az, n_el) = P.shape[0], P.shape[2], d.shape[1:]
    if n == 0:
        out = np.zeros((0, n_az, n_el), np.float32)
        return (out, np.zeros((0, n_az, n_el), np.complex128)) if with_factor else out
    ctx = ctx if ctx is not None else _lib.default_context()
    T = n_az * n_el
    d_P, d_pat = ctx.cached("array_patterns_P", P.nbytes), ctx.cached("array_patterns", n * T * 4)
    d_af = ctx.cached("array_patterns_af", n * T * 16) if with_factor else None
    d_P.upload(P)
    array_patterns_on(ctx, d_P.ptr, n, E, d, lam, d_pat, d_af)
    out = d_pat.download((n, n_az, n_el), np.float32)
    return (out, d_af.download((n, n_az, n_el), np.complex128)) if with_factor else out


# Bytes of snapshots per pass.  Measured (profiles/capon_range_angle.json): 1024 MiB is the fastest of 16 / 64 /
# 256 / 1024 MiB and a single pass on both bench shapes; 256 MiB is within 1 % of it, the 64 MiB first guessed (a quarter of the
# Infinity Cache) 4-9 % slower, 16 MiB 1.8-2.4 times slower: the launches of a short pass do not fill the chip.
CAPON_PASS_BUDGET = 1024 << 20


def capon_pass_frames(n_rx: int, n_rows: int, C: int, budget_bytes: int = CAPON_PASS_BUDGET) -> int:
    """Frames per pass of ``capon_range_angle``: the largest count whose complex64 snapshot tensor ``[n][n_rx][n_rows][C]`` fits
    ``budget_bytes``, and at least 1."""
    per_frame = int(n_rx) * int(n_rows) * int(C) * 8
    if per_frame < 1:
        raise ValueError(f"capon_pass_frames: n_rx {n_rx}, n_rows {n_rows} and C {C} must all be positive")
    return max(1, int(budget_bytes) // per_frame)


def capon_passes(n_frames: int, frames_per_pass: int):
    """``[(f0, f1), ...]``: the frame intervals of the passes, in order; the last one may be shorter."""
    n, step = int(n_frames), int(frames_per_pass)
    if step < 1:
        raise ValueError(f"frames_per_pass must be a positive integer, got {frames_per_pass}")
    return [(f0, min(f0 + step, n)) for f0 in range(0, n, step)]


def capon_cube_args(V: int, S: int, thetas_rad, rx_antennas, range_bins, delta, frames_per_pass):
    """The argument checks of ``capon_range_angle`` / ``process_cube`` (no device is touched): ``(thetas float64 [T], rx list,
    (r_lo, r_hi), delta, frames_per_pass or None)``."""
    th = np.ascontiguousarray(thetas_rad, dtype=np.float64)
    if th.ndim != 1 or th.size < 1:
        raise ValueError(f"capon_range_angle: thetas_rad must be a non-empty 1-D grid of angles, got shape {th.shape}")
    if not np.all(np.isfinite(th)):
        raise ValueError(f"capon_range_angle: thetas_rad holds a value that is not finite ({th[~np.isfinite(th)][0]})")
    rx_in = np.asarray(rx_antennas)
    if rx_in.ndim != 1 or not 1 <= rx_in.size <= 16:
        raise ValueError(f"capon_range_angle: rx_antennas must list 1..16 antennas (a uniform line array in list order), got "
                         f"{rx_in.size} in shape {rx_in.shape}")
    if not np.all(rx_in == np.floor(rx_in)):
        raise ValueError(f"capon_range_angle: rx_antennas {rx_in.tolist()} are not integers")
    rx = [int(i) for i in rx_in]
    for i in rx:
        if not -V <= i < V:
            raise IndexError(f"capon_range_angle: rx_antennas index {i} is out of bounds for {V} antennas")
    if range_bins is None:
        range_bins = (0, S)
    try:
        r_lo, r_hi = (int(r) for r in range_bins)
    except (TypeError, ValueError):
        raise ValueError(f"capon_range_angle: range_bins must be a pair (r_lo, r_hi) of bin indices, got {range_bins!r}") from None
    if not 0 <= r_lo < r_hi <= S:
        raise ValueError(f"capon_range_angle: range_bins ({r_lo}, {r_hi}) is not 0 <= r_lo < r_hi <= {S}")
    d = float(delta)
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"capon_range_angle: delta {delta} is not a finite number >= 0")
    if frames_per_pass is not None:
        if int(frames_per_pass) != frames_per_pass or int(frames_per_pass) < 1:
            raise ValueError(f"capon_range_angle: frames_per_pass must be a positive integer, got {frames_per_pass}")
        frames_per_pass = int(frames_per_pass)
    return th, [i % V for i in rx], (r_lo, r_hi), d, frames_per_pass


def capon_from_cubes(ctx: _lib.Context, d_cubes: int, d_snap: _lib.DeviceBuffer, d_out: _lib.DeviceBuffer, n_frames: int, shape,
                     thetas: np.ndarray, rx, window, delta: float, perform_windowing: bool, frames_per_pass: int) -> None:
    """The two device stages of the Capon range-azimuth map on cubes at device address ``d_cubes`` (``[n_frames][V][S][C]``
    complex64): per pass of ``frames_per_pass`` frames ``mmw_range_snapshots`` into ``d_snap``, then ``mmw_capon`` from there into
    the pass's slice of ``d_out`` (float32 ``[n_frames][R_w][T]``), all on the context's queue in order -- the queue is what keeps
    a pass's snapshots alive until its Capon launch has read them."""
    V, S, C = shape
    (r_lo, r_hi), T, n_rx = window, len(thetas), len(rx)
    Rw = r_hi - r_lo
    rx_arr, _ = _lib.int_array(rx)
    th = thetas.ctypes.data_as(C_POINTER_DOUBLE)
    for f0, f1 in capon_passes(n_frames, frames_per_pass):
        _lib.check(ctx.lib.mmw_range_snapshots(ctx.handle, d_cubes + f0 * V * S * C * 8, d_snap.ptr, f1 - f0, V, S, C, rx_arr, n_rx,
                                               r_lo, r_hi, int(bool(perform_windowing))))
        _lib.check(ctx.lib.mmw_capon(ctx.handle, d_snap.ptr, th, d_out.at(f0 * Rw * T * 4), f1 - f0, n_rx, Rw, C, T, delta))


C_POINTER_DOUBLE = C.POINTER(C.c_double)

CAPON_DOPPLER_MAX_CHIRPS = 512      # include/mmwgpu.h mmw_capon_doppler: K of 1 .. 512
CAPON_POINTS_PASS_FRAMES = 32768    # frames of one mmw_cfar2d call (its grid), so of one pass


def capon_points_args(V: int, S: int, C_chirps: int, thetas_rad, rx_antennas, detector, range_bins=None, delta=1e-3,
                      frames_per_pass=None, det_capacity: int = 2048):
    """The argument checks of ``capon_point_clouds`` (no device is touched): those of ``capon_cube_args``, then the detector
    and the capacity.  ``detector``: a stock ``CaCFAR2D`` / ``OsCFAR2D`` of this package whose ``num_train`` / ``num_guard`` are
    (range, angle) pairs; it becomes (kind, train_r, train_a, guard_r, guard_a, scale, k_rank) the way ``FramePipeline(cfar=...)``
    reads its detector.  Any other object raises ``ValueError``.  Returns ``(thetas float64 [T], rx list, (r_lo, r_hi), delta,
    frames_per_pass or None, cfar tuple, cap)``."""
    from ..detectors.base import BaseCFAR2D
    th, rx, window, d, fpp = capon_cube_args(V, S, thetas_rad, rx_antennas, range_bins, delta, frames_per_pass)
    what = "capon_point_clouds"
    if not 1 <= int(C_chirps) <= CAPON_DOPPLER_MAX_CHIRPS:
        raise ValueError(f"{what}: {C_chirps} chirps per frame (the beamformed Doppler spectrum takes 1 .. {CAPON_DOPPLER_MAX_CHIRPS})")
    if not isinstance(detector, BaseCFAR2D) or type(detector)._compute_thresholds is not BaseCFAR2D._compute_thresholds or \
            detector.kind not in (_lib.CFAR_CA, _lib.CFAR_OS):
        raise ValueError(f"{what}: detector must be a stock CaCFAR2D or OsCFAR2D of this package, got {type(detector).__name__}")
    pairs = []
    for name in ("num_train", "num_guard"):
        try:
            a, b = getattr(detector, name)
            ok = int(a) == a and int(b) == b and a >= 0 and b >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{what}: detector.{name} must be a (range, angle) pair of non-negative integers, "
                             f"got {getattr(detector, name)!r}")
        pairs += [int(a), int(b)]
    scale, k_rank = float(detector._scale()), int(detector._k_rank())
    if not np.isfinite(scale):
        raise ValueError(f"{what}: the detector's threshold factor {scale} is not finite")
    if detector.kind == _lib.CFAR_OS:
        n_train = (2 * (pairs[0] + pairs[2]) + 1) * (2 * (pairs[1] + pairs[3]) + 1) - (2 * pairs[2] + 1) * (2 * pairs[3] + 1)
        if not 1 <= k_rank <= n_train:
            raise ValueError(f"{what}: the detector's rank {k_rank} is not one of its {n_train} training cells")
    if int(det_capacity) != det_capacity or int(det_capacity) < 1:
        raise ValueError(f"{what}: det_capacity must be a positive integer, got {det_capacity}")
    return th, rx, window, d, fpp, (int(detector.kind), *pairs, scale, k_rank), int(det_capacity)


def capon_doppler_on(ctx: _lib.Context, d_X: int, d_dets: int, d_counts: int, thetas: np.ndarray, d_dop: int, d_peak: int,
                     d_spec, d_points, d_range, d_vel, n_frames: int, n: int, R: int, K: int, cap: int, delta: float,
                     doppler_windowing: bool) -> None:
    """``mmw_capon_doppler`` on device addresses (``d_spec`` / ``d_points`` / ``d_range`` / ``d_vel`` may be None)."""
    _lib.check(ctx.lib.mmw_capon_doppler(ctx.handle, d_X, d_dets, d_counts, thetas.ctypes.data_as(C_POINTER_DOUBLE), d_dop, d_peak,
                                         d_spec, d_points, d_range, d_vel, n_frames, n, R, K, len(thetas), cap, delta,
                                         int(bool(doppler_windowing))))


class CaponBeamformer:
    """MVDR angle spectrum per range bin on a V-element half-wavelength ULA (no upstream oracle).

    ``R_r = X_r X_r^H / K + delta tr(R_r)/V I``, ``P(r, theta) = 1 / Re(a^H R_r^-1 a)``,
    ``a_v(theta) = exp(-j pi v sin(theta))``.  float64 on the f64 matrix cores."""

    def __init__(self, thetas_rad, delta: float = 1e-3, ctx: _lib.Context = None):
        self.thetas_rad = np.ascontiguousarray(thetas_rad, dtype=np.float64)
        self.delta = float(delta)
        self._ctx = ctx
        self._bufs = None

    def process(self, X_vrk: np.ndarray) -> np.ndarray:
        """X ``[V, R, K]`` complex snapshots (e.g. range-FFT output per chirp) -> float64 ``[R, T]``;
        a batch ``[F, V, R, K]`` -> ``[F, R, T]`` in one launch."""
        if self._ctx is None:
            self._ctx = _lib.default_context()
        if self._bufs is None:
            self._bufs = _lib.BufferSet(self._ctx)
        ctx, bufs = self._ctx, self._bufs
        X = np.ascontiguousarray(X_vrk, dtype=np.complex64)
        single = X.ndim == 3
        if single:
            X = X[None]
        if X.ndim != 4:
            raise ValueError("expected [V, R, K] or [F, V, R, K] snapshots")
        F, V, R, K = X.shape
        T = len(self.thetas_rad)
        d_X, d_out = bufs.get("cap_x", X.nbytes), bufs.get("cap_p", F * R * T * 4)
        d_X.upload(X)
        th = self.thetas_rad.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(ctx.lib.mmw_capon(ctx.handle, d_X.ptr, th, d_out.ptr, F, V, R, K, T, self.delta))
        out = d_out.download((F, R, T), np.float32).astype(np.float64)
        return out[0] if single else out

    def beamformed_doppler(self, X_vrk: np.ndarray, dets, doppler_windowing: bool = True, return_spectra: bool = False):
        """The Doppler bin of detections made on ``process(X)``, each through the MVDR weights of its own cell (DESIGN.md 4.28,
        ``mmw_capon_doppler``).  ``X [V, R, K]`` with ``dets`` an ``(N, 2)`` integer array of (row, angle index) ->
        ``(dop int64 (N,), peak float64 (N,))``; a batch ``[F, V, R, K]`` with a list of F such arrays -> two lists.  Per
        detection ``(q, t)``: ``w = R_q^-1 a / Re(a^H R_q^-1 a)`` with ``a = a(thetas_rad[t])``, ``y[k] = w^H X[:, q, k]``,
        ``z = fftshift(fft(hanning(K) * y))`` (no window with ``doppler_windowing=False``), ``dop = argmax |z|``,
        ``peak = |z[dop]|``.  ``return_spectra=True`` adds ``|z|`` as float64 ``(N, K)``.  A row whose loaded covariance is not
        positive definite, and a detection outside the map, give ``dop`` -1 and ``peak`` NaN."""
        X = np.ascontiguousarray(X_vrk, dtype=np.complex64)
        single = X.ndim == 3
        if single:
            X, dets = X[None], [dets]
        if X.ndim != 4:
            raise ValueError("expected [V, R, K] or [F, V, R, K] snapshots")
        F, V, R, K = X.shape
        if len(dets) != F:
            raise ValueError(f"beamformed_doppler: {len(dets)} detection lists for {F} frames")
        lists = [np.asarray(d, dtype=np.int64).reshape(-1, 2) for d in dets]
        for d in lists:
            if d.size and (np.abs(d).max() >= 2**31):
                raise ValueError("beamformed_doppler: a detection index does not fit int32")
        if not 1 <= K <= CAPON_DOPPLER_MAX_CHIRPS:
            raise ValueError(f"beamformed_doppler: {K} snapshots per bin (1 .. {CAPON_DOPPLER_MAX_CHIRPS})")
        empty = (np.zeros(0, np.int64), np.zeros(0), np.zeros((0, K)))[:3 if return_spectra else 2]
        cap = max([len(d) for d in lists] + [1])
        if F == 0:
            return ([], [], []) if return_spectra else ([], [])
        if self._ctx is None:
            self._ctx = _lib.default_context()
        if self._bufs is None:
            self._bufs = _lib.BufferSet(self._ctx)
        ctx, bufs = self._ctx, self._bufs
        packed = np.zeros((F, cap, 2), np.int32)
        for f, d in enumerate(lists):
            packed[f, :len(d)] = d
        counts = np.array([len(d) for d in lists], np.int32)
        d_X, d_dets, d_cnt = bufs.get("cap_x", X.nbytes), bufs.get("cd_dets", packed.nbytes), bufs.get("cd_cnt", counts.nbytes)
        d_dop, d_peak = bufs.get("cd_dop", F * cap * 4), bufs.get("cd_peak", F * cap * 8)
        d_spec = bufs.get("cd_spec", F * cap * K * 8) if return_spectra else None
        d_X.upload(X)
        d_dets.upload(packed)
        d_cnt.upload(counts)
        capon_doppler_on(ctx, d_X.ptr, d_dets.ptr, d_cnt.ptr, self.thetas_rad, d_dop.ptr, d_peak.ptr,
                         d_spec.ptr if return_spectra else None, None, None, None, F, V, R, K, cap, self.delta, doppler_windowing)
        dop = d_dop.download((F, cap), np.int32)
        peak = d_peak.download((F, cap), np.float64)
        spec = d_spec.download((F, cap, K), np.float64) if return_spectra else None
        out = []
        for f, n in enumerate(counts):
            row = (dop[f, :n].astype(np.int64), peak[f, :n].copy()) if n else empty[:2]
            if return_spectra:
                row += (spec[f, :n].copy() if n else empty[2],)
            out.append(row)
        if single:
            return out[0]
        return tuple(list(col) for col in zip(*out))

    def process_cube(self, cube_vsc: np.ndarray, rx_antennas, range_bins=None, perform_windowing: bool = True) -> np.ndarray:
        """One radar cube ``[V, S, C]`` (samples on the slow axis, chirps contiguous) -> float64 ``[R_w, T]``; a batch
        ``[F, V, S, C]`` -> ``[F, R_w, T]``.  ``rx_antennas``: the 1..16 antennas of the azimuth row, a half-wavelength line
        array in list order; ``range_bins=(r_lo, r_hi)`` in bin indices (default: the whole profile).  The cube is uploaded as
        it is and the snapshots -- the Hann-windowed range FFT of every chirp of the listed antennas -- are made on the device
        (``mmw_range_snapshots``) and handed to ``mmw_capon`` there, in passes of ``capon_pass_frames`` frames: the two calls
        ``FramePipeline.capon_range_angle`` makes on resident frames."""
        cube = np.asarray(cube_vsc)
        single = cube.ndim == 3
        if cube.ndim not in (3, 4):
            raise ValueError(f"expected a [V, S, C] cube or a [F, V, S, C] batch, got shape {cube.shape}")
        F = 1 if single else cube.shape[0]
        V, S, Cc = cube.shape[-3:]
        if min(V, S, Cc) < 1:
            raise ValueError(f"expected a [V, S, C] cube or a [F, V, S, C] batch with V, S, C >= 1, got shape {cube.shape}")
        th, rx, (r_lo, r_hi), delta, _ = capon_cube_args(V, S, self.thetas_rad, rx_antennas, range_bins, self.delta, None)
        Rw, T = r_hi - r_lo, len(th)
        if F == 0:
            return np.zeros((0, Rw, T))
        if self._ctx is None:
            self._ctx = _lib.default_context()
        if self._bufs is None:
            self._bufs = _lib.BufferSet(self._ctx)
        ctx, bufs = self._ctx, self._bufs
        cube = np.ascontiguousarray(cube, dtype=np.complex64)
        fpp = min(F, capon_pass_frames(len(rx), Rw, Cc))
        d_cube, d_out = bufs.get("cap_cube", cube.nbytes), bufs.get("cap_p", F * Rw * T * 4)
        d_snap = bufs.get("cap_snap", fpp * len(rx) * Rw * Cc * 8)
        d_cube.upload(cube)
        capon_from_cubes(ctx, d_cube.ptr, d_snap, d_out, F, (V, S, Cc), th, rx, (r_lo, r_hi), delta, perform_windowing, fpp)
        out = d_out.download((F, Rw, T), np.float32).astype(np.float64)
        return out[0] if single else out
