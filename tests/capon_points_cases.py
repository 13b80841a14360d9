"""The float64 NumPy restatement of the Capon point-cloud definition and the seeded inputs of its tests
(test_capon_points_host.py, test_gpu_capon_points.py).  Pure NumPy; nothing here touches a device or the library.

Restatement, per frame, on snapshots X [n][R][K] (complex64 promoted exactly to complex128):
    R_q = X_q X_q^H / K + delta tr(X_q X_q^H / K) / n I,   a_i(theta) = exp(-j pi i sin(theta)),
    u = solve(R_q, a),  w = u / Re(a^H u),  y = w^H X_q,  z = fftshift(fft(hanning(K) * y)),  dop = argmax |z|,  peak = |z[dop]|,
    point = (rng cos(theta), rng sin(theta), 0, vel_bins[dop]).
A row whose R_q is not positive definite (np.linalg.cholesky refuses it, or it holds a non-finite value) is degenerate:
dop -1, peak NaN.

Cubes: 3 point targets plus complex Gaussian noise, integer-valued complex64 like synth.synth_cube.  Every target sits on a
range bin of its own, at a Doppler frequency at least 0.1 bin away from any half-integer bin (so the peak bin of its spectrum is
not a near-tie of two neighbours), with an antenna phase exp(-j pi v sin(theta0)).
"""
import functools

import numpy as np

DELTA = 1e-3
T_ANGLES = 33
THETAS = np.deg2rad(np.linspace(-60.0, 60.0, T_ANGLES))
SPEC_TOL = 1e-9             # |z| within SPEC_TOL * peak of the restatement (the issue's bound: cond * n * eps ~ 6e-11)
DOP_BAND = 1e-8             # dop must agree where the restatement's two largest |z| differ by more than this, relatively
AMPLITUDE = 220.0
NOISE_SIGMA = 3.0


def steering(n, thetas):
    """complex128 [n][T]"""
    return np.exp(-1j * np.pi * np.arange(n)[:, None] * np.sin(np.asarray(thetas, dtype=np.float64))[None, :])


def covariance(Xq, delta):
    """The loaded covariance of one row's snapshots Xq [n][K] (complex128)."""
    n, K = Xq.shape
    Rm = (Xq @ Xq.conj().T) / K
    return Rm + delta * np.real(np.trace(Rm)) / n * np.eye(n)


def is_degenerate(Rm):
    if not np.all(np.isfinite(Rm)):
        return True
    try:
        np.linalg.cholesky(Rm)
    except np.linalg.LinAlgError:
        return True
    return False


def doppler_reference(X, dets, thetas, delta=DELTA, doppler_windowing=True):
    """One frame: X [n][R][K] complex, dets (N, 2) of (row, angle index) -> (dop int64 (N,), peak (N,), |z| (N, K)).
    A degenerate row and a detection outside the map give -1 / NaN."""
    X = np.asarray(X).astype(np.complex128)
    n, R, K = X.shape
    dets = np.asarray(dets, dtype=np.int64).reshape(-1, 2)
    A = steering(n, thetas)
    h = np.hanning(K) if doppler_windowing else np.ones(K)
    dop = np.full(len(dets), -1, dtype=np.int64)
    peak = np.full(len(dets), np.nan)
    spec = np.full((len(dets), K), np.nan)
    rows = {}
    for j, (q, t) in enumerate(dets):
        if not (0 <= q < R and 0 <= t < len(thetas)):
            continue
        if q not in rows:
            Rm = covariance(X[:, q, :], delta)
            rows[q] = None if is_degenerate(Rm) else Rm
        if rows[q] is None:
            continue
        a = A[:, t]
        u = np.linalg.solve(rows[q], a)
        w = u / np.real(np.vdot(a, u))
        y = w.conj() @ X[:, q, :]
        z = np.abs(np.fft.fftshift(np.fft.fft(h * y)))
        spec[j] = z
        dop[j] = int(np.argmax(z))
        peak[j] = z[dop[j]]
    return dop, peak, spec


def top_two_gap(spec_row):
    """Relative gap between the two largest values of one |z| (inf for a single bin)."""
    if len(spec_row) < 2:
        return np.inf
    a = np.sort(spec_row)[-2:]
    return (a[1] - a[0]) / a[1] if a[1] > 0 else 0.0


def points_reference(dets, dop, thetas, range_rows, vel_bins, cos_t=None, sin_t=None):
    """(N, 4) float64 points of one frame from (row, angle index) detections and Doppler bins; velocity NaN where dop < 0."""
    dets = np.asarray(dets, dtype=np.int64).reshape(-1, 2)
    cos_t = np.cos(thetas) if cos_t is None else cos_t
    sin_t = np.sin(thetas) if sin_t is None else sin_t
    rng = np.asarray(range_rows)[dets[:, 0]]
    vel = np.where(np.asarray(dop) >= 0, np.asarray(vel_bins)[np.maximum(dop, 0)], np.nan)
    return np.column_stack((rng * cos_t[dets[:, 1]], rng * sin_t[dets[:, 1]], np.zeros(len(dets)), vel))


def targets_of(shape, seed, n_targets=3):
    """[(range bin, Doppler frequency in bins in [-C/2, C/2), theta0)]: rows spread over the profile, |offset| <= 0.4 from a bin."""
    V, S, C = shape
    rng = np.random.default_rng(seed)
    rows = np.linspace(S // 6, S - 1 - S // 6, n_targets).round().astype(int) if S >= 6 else np.arange(min(S, n_targets))
    out = []
    for i, r in enumerate(rows):
        fd = float(rng.integers(-(C // 2), (C + 1) // 2)) + float(rng.uniform(-0.4, 0.4)) if C > 2 else 0.0
        out.append((int(r), fd, np.deg2rad(float(rng.uniform(-45.0, 45.0)))))
    return out


@functools.lru_cache(maxsize=None)
def cubes(shape, n_frames, seed, amplitude=AMPLITUDE, noise_sigma=NOISE_SIGMA):
    """complex64 [F][V][S][C], integer-valued I/Q; frame f holds targets_of(shape, seed + f).  Treat as read-only."""
    V, S, C = shape
    v = np.arange(V)[:, None, None]
    s = np.arange(S)[None, :, None]
    c = np.arange(C)[None, None, :]
    out = np.empty((n_frames, V, S, C), dtype=np.complex64)
    for f in range(n_frames):
        rng = np.random.default_rng(100003 * (seed + f) + 17)
        x = noise_sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        for r0, fd, th0 in targets_of(shape, seed + f):
            phase = 2.0 * np.pi * (r0 * s / S + fd * c / C) - np.pi * v * np.sin(th0) + rng.uniform(0, 2 * np.pi)
            x = x + amplitude * np.exp(1j * phase)
        out[f] = (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)
    out.setflags(write=False)
    return out


def snapshots_of(cube_batch, rx, window, windowing=True):
    """complex64 [F][n][R_w][C]: the (Hann-windowed) range FFT of the listed antennas in float64, rounded once to complex64 -- what
    mmw_range_snapshots computes in float32, up to that kernel's rounding."""
    x = np.asarray(cube_batch).astype(np.complex128)[:, list(rx)]
    S = x.shape[2]
    w = np.hanning(S) if windowing else np.ones(S)
    return np.ascontiguousarray(np.fft.fft(x * w[None, None, :, None], axis=2)[:, :, window[0]:window[1], :]).astype(np.complex64)


# (n, R, K, seed) of the host cases: K = 1 (one bin), K = 2 (an all-zero Hann window), n = 1 and n = 16 (the extremes), K not a
# power of two.  The seeds were checked with the restatement alone: no detection of host_dets falls inside DOP_BAND.
HOST_SHAPES = ((8, 6, 16, 11), (12, 5, 10, 12), (1, 3, 7, 13), (16, 2, 1, 14), (4, 3, 2, 15))


@functools.lru_cache(maxsize=None)
def host_snapshots(n, R, K, seed, n_frames=2):
    """complex64 [F][n][R][K] snapshots of cubes((n, R, K), ...): all antennas, the whole profile, no range window."""
    X = snapshots_of(cubes((n, R, K), n_frames, seed), range(n), (0, R), windowing=False)
    X.setflags(write=False)
    return X


def host_dets(n, R, K, seed, n_frames=2, cap=24):
    """int32 [F][cap][2] and counts [F]: per frame, row-major, several detections in the first and in the last row, the targets'
    own cells (nearest angle index) and one more cell per row."""
    dets = np.zeros((n_frames, cap, 2), np.int32)
    counts = np.zeros(n_frames, np.int32)
    for f in range(n_frames):
        cells = {(0, 0), (0, T_ANGLES // 2), (0, T_ANGLES - 1), (R - 1, 1), (R - 1, T_ANGLES - 2), (R - 1, 7)}
        for q in range(R):
            cells.add((q, (5 * q + 3 * f) % T_ANGLES))
        for r0, _, th0 in targets_of((n, R, K), seed + f):
            cells.add((r0, int(np.argmin(np.abs(THETAS - th0)))))
        lst = sorted(cells)
        counts[f] = len(lst)
        dets[f, :len(lst)] = lst
    return dets, counts


def tables(R, K):
    """(range rows [R], velocity bins [K]) of the host cases: any float64 tables serve."""
    return 0.1 * np.arange(R) + 0.05, 0.2 * (np.arange(K) - K // 2)
