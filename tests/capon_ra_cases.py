"""Inputs and float64 references of the Capon range-azimuth tests (test_capon_range_angle_host.py,
test_gpu_capon_range_angle.py).  Pure NumPy.

The cubes are point targets: x[f][v][s][c] = A exp(2 pi j r0 s / S) exp(-j pi v sin theta0) exp(j phi_c) + noise, phi_c random
per chirp (the snapshots of a bin are then not one vector repeated), the noise about 30 dB below A.  A frame's target sits at
(r0, theta0 + 0.05 f): every frame's map differs from the others', so a map written to another frame's slot is seen.

SHAPES lists the smallest (V, S, C) at which each mechanism of mmw_range_snapshots can go wrong; every shape is paired with four
range windows, four antenna lists and the window switch (snapshot_cases).
"""
import functools

import numpy as np

F = 3
AMPLITUDE = 8.0
NOISE_DB = -30.0
DELTA = 1e-3
# (V, S, C): what it exercises
SHAPES = (
    (4, 16, 5),         # smallest FFT path; C below a strip of 16 chirps; a K tail in Capon's 32-snapshot chunks
    (12, 64, 32),       # aligned: two full strips, K one whole chunk
    (16, 256, 33),      # 16 antennas; a strip tail of one chirp
    (12, 1024, 8),      # largest S (512 threads, 132 KiB of LDS)
    (12, 63, 100),      # direct path; K not a multiple of 32; rows not a multiple of the 64 a workgroup carries at once
    (5, 100, 70),       # direct path; strip tail of six chirps
    (3, 4, 2),          # tiny direct path (a power of two below the FFT path's smallest)
)
THETAS = np.deg2rad(np.linspace(-60.0, 60.0, 41))       # 3 degree grid


def is_fft_path(S):
    return 16 <= S <= 1024 and S & (S - 1) == 0


def target_of(shape, f=0):
    """(r0, theta0) of frame f's target: r0 inside the interior window, theta0 off the grid."""
    V, S, C = shape
    return max(1, (2 * S) // 5) if S > 4 else 1, np.deg2rad(-17.0) + 0.05 * f


def windows(S):
    """(0, S), (0, 1), (S - 1, S) and one interior window (holding the target's bin), without repeats."""
    r0 = target_of((1, S, 1))[0]
    interior = (max(0, r0 - 3), min(S, r0 + 4)) if S > 4 else (1, 3)
    out = []
    for w in ((0, S), (0, 1), (S - 1, S), interior):
        if w not in out:
            out.append(w)
    return out


def interior_window(S):
    return windows(S)[-1]


def antenna_lists(V):
    """n_rx = 0 (all, in order), one antenna, a permuted subset, a list with a duplicate."""
    perm = list(np.random.default_rng(V).permutation(V)[:max(2, (2 * V) // 3)])
    return [[], [V - 1], [int(i) for i in perm], [0, V - 1, 0] if V > 1 else [0, 0]]


def ula(V):
    """The antenna list of the end-to-end cases: the first min(V, 16) antennas in order (a half-wavelength line array)."""
    return list(range(min(V, 16)))


@functools.lru_cache(maxsize=None)
def cubes(shape):
    """complex64 [F][V][S][C], fixed seed per shape.  Treat as read-only."""
    V, S, C = shape
    rng = np.random.default_rng(7000 + 131 * V + 17 * S + C)
    sigma = AMPLITUDE * 10.0 ** (NOISE_DB / 20.0) / np.sqrt(2.0)
    x = sigma * (rng.standard_normal((F, V, S, C)) + 1j * rng.standard_normal((F, V, S, C)))
    s = np.arange(S).reshape(1, 1, S, 1)
    v = np.arange(V).reshape(1, V, 1, 1)
    phi = rng.uniform(0, 2 * np.pi, (F, 1, 1, C))
    for f in range(F):
        r0, th0 = target_of(shape, f)
        x[f] += (AMPLITUDE * np.exp(2j * np.pi * r0 * s / S) * np.exp(-1j * np.pi * v * np.sin(th0)) * np.exp(1j * phi[f]))[0]
    out = x.astype(np.complex64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def full_reference(shape, windowing):
    """complex128 [F][V][S][C]: the windowed range transform of every antenna in float64, the complex64 cube promoted exactly --
    np.fft.fft for a power-of-two S, an explicit DFT matrix (its phases reduced mod S in integers) for the others.  Read-only."""
    V, S, C = shape
    x = cubes(shape).astype(np.complex128)
    w = np.hanning(S) if windowing else np.ones(S)
    xw = x * w.reshape(1, 1, S, 1)
    if S & (S - 1) == 0:
        ref = np.fft.fft(xw, axis=2)
    else:
        m = (np.arange(S)[:, None] * np.arange(S)[None, :]) % S
        W = np.exp(-2j * np.pi * m / S)
        ref = np.einsum("rs,fvsc->fvrc", W, xw)
    ref.setflags(write=False)
    return ref


def reference_snapshots(shape, rx, window, windowing):
    """complex128 [F][n_rx][r_hi - r_lo][C]: what mmw_range_snapshots defines (rx == []: all antennas in order)."""
    V = shape[0]
    ants = list(rx) if len(rx) else list(range(V))
    return np.ascontiguousarray(full_reference(shape, bool(windowing))[:, ants, window[0]:window[1], :])


def snapshot_cases(shape):
    """(rx, window, windowing) for every pairing of the shape's windows, antenna lists and the window switch."""
    V, S, C = shape
    return [(rx, w, win) for rx in antenna_lists(V) for w in windows(S) for win in (True, False)]


def point_target_cases():
    """(shape, rx, window, row of r0 inside the window): the end-to-end cases, one per shape."""
    out = []
    for shape in SHAPES:
        w = interior_window(shape[1])
        out.append((shape, ula(shape[0]), w, target_of(shape)[0] - w[0]))
    return out


def pass_list(n_frames, frames_per_pass):
    return [(f0, min(f0 + frames_per_pass, n_frames)) for f0 in range(0, n_frames, frames_per_pass)]
