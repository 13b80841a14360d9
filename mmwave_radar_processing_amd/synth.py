"""Synthetic IWR1843-style inputs: TI ``.cfg`` text and raw ADC cubes.

Input generation only -- no signal processing happens here.  The recipe is
the one SURVEY.md section 8(d) fixes for the headline workload: K point
targets plus complex Gaussian noise, rounded to integers (16-bit-ADC-like)
and stored complex64 in the reference's cube layout ``[virtRx, sample,
chirp]``, C-order, chirp fastest (reference:
mmwave_radar_processing/processors/_processor.py:58).
"""
from __future__ import annotations

import numpy as np

# 4 Rx x 3 Tx (TDM), 256 samples, 128 loops -> virtual cube (12, 256, 128).
# Field order per TI mmWave SDK; parsed by config_managers.ConfigManager.
SYNTH_CFG_256x128x12 = """\
channelCfg 15 7 0
adcCfg 2 1
profileCfg 0 77 7 7 60 0 0 30 1 256 5000 0 0 30
chirpCfg 0 0 0 0 0 0 0 1
chirpCfg 1 1 0 0 0 0 0 2
chirpCfg 2 2 0 0 0 0 0 4
frameCfg 0 2 128 0 100 1 0
"""


def synth_cfg_text(num_samples: int = 256, num_loops: int = 128, num_tx: int = 3,
                   rx_mask: int = 15, sample_rate_ksps: int = 5000,
                   slope_mhz_us: float = 30.0, start_freq_ghz: float = 77.0) -> str:
    """Text of a minimal TI cfg producing ``(popcount(rx_mask)*num_tx, num_samples, num_loops)``."""
    tx_mask = (1 << num_tx) - 1
    lines = [
        f"channelCfg {rx_mask} {tx_mask} 0",
        "adcCfg 2 1",
        f"profileCfg 0 {start_freq_ghz:g} 7 7 60 0 0 {slope_mhz_us:g} 1 {num_samples} {sample_rate_ksps} 0 0 30",
    ]
    for i in range(num_tx):
        lines.append(f"chirpCfg {i} {i} 0 0 0 0 0 {1 << i}")
    lines.append(f"frameCfg 0 {num_tx - 1} {num_loops} 0 100 1 0")
    return "\n".join(lines) + "\n"


def synth_cube(seed: int, shape=(12, 256, 128), num_targets: int = 8,
               noise_sigma: float = 30.0) -> np.ndarray:
    """One virtual-array ADC cube ``[V, S, C]`` complex64 with integer-valued I/Q.

    ``default_rng(seed)`` (PCG64) is stable across numpy versions, so tests
    and the golden generator regenerate identical inputs from the seed.
    """
    V, S, C = shape
    rng = np.random.default_rng(seed)
    f_r = rng.uniform(0.02, 0.45, num_targets)
    f_d = rng.uniform(-0.45, 0.45, num_targets)
    f_a = rng.uniform(-0.4, 0.4, num_targets)
    amp = rng.uniform(20.0, 400.0, num_targets)
    phi = rng.uniform(0.0, 2.0 * np.pi, num_targets)
    v = np.arange(V)[:, None, None]
    n = np.arange(S)[None, :, None]
    m = np.arange(C)[None, None, :]
    x = np.zeros(shape, dtype=np.complex128)
    for k in range(num_targets):
        x += amp[k] * np.exp(1j * (2.0 * np.pi * (f_r[k] * n + f_d[k] * m + f_a[k] * v) + phi[k]))
    x += noise_sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    return (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)


def synth_raw_cube(seed: int, num_rx: int = 4, num_tx: int = 3, num_samples: int = 256,
                   num_loops: int = 128) -> np.ndarray:
    """Raw TDM-interleaved cube ``[num_rx, S, num_tx*loops]`` (input of VirtualArrayReformatter).

    Built by interleaving a virtual cube so that de-interleaving it gives
    ``synth_cube(seed, (num_rx*num_tx, S, loops))`` back.
    """
    virt = synth_cube(seed, (num_rx * num_tx, num_samples, num_loops))
    raw = np.empty((num_rx, num_samples, num_tx * num_loops), dtype=np.complex64)
    for t in range(num_tx):
        raw[:, :, t::num_tx] = virt[t * num_rx:(t + 1) * num_rx]
    return raw


def synth_tdm_targets(seed: int, num_rx: int, num_tx: int, S: int, loops: int, targets, noise_sigma: float = 0.0,
                      num_angle_bins: int = 64, shift: bool = True):
    """Raw TDM-MIMO cube ``[num_rx, S, num_tx * loops]`` complex64 of point targets, and each target's true angle bin.

    ``targets``: rows ``(amplitude, f_range, f_doppler, f_spatial)`` -- cycles per sample, cycles per RAW chirp and cycles per
    virtual element.  Raw chirp ``n = loop * num_tx + tx`` is sent by transmitter ``tx``; receiver ``rx`` then is element
    ``tx * num_rx + rx`` of a uniform virtual array (the order VirtualArrayReformatter stacks).  The Doppler phase runs over the raw
    chirp index, so the antennas of transmit slot ``tx`` carry ``2 pi f_doppler tx`` from the chirp timing itself: nothing is
    injected.  A target on Doppler bin ``kd`` of the de-interleaved cube has ``f_doppler = kd / (num_tx * loops)``.
    ``noise_sigma``: complex Gaussian noise from ``default_rng(seed)``; the samples are NOT rounded to integers.
    The true bin of a target is ``round(f_spatial * num_angle_bins)`` modulo the FFT size, fftshifted with ``shift``."""
    t = np.asarray(targets, dtype=np.float64).reshape(-1, 4)
    rng = np.random.default_rng(seed)
    rx = np.arange(num_rx)[:, None, None]
    s = np.arange(S)[None, :, None]
    n = np.arange(num_tx * loops)[None, None, :]
    elem = (n % num_tx) * num_rx + rx
    x = np.zeros((num_rx, S, num_tx * loops), dtype=np.complex128)
    for amp, f_r, f_d, f_a in t:
        x += amp * np.exp(2j * np.pi * (f_r * s + f_d * n + f_a * elem))
    if noise_sigma:
        x += noise_sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    A = int(num_angle_bins)
    bins = np.rint(t[:, 3] * A).astype(np.int64) % A
    if shift:
        bins = (bins + A // 2) % A
    return x.astype(np.complex64), bins


def synth_ground_sequence(seed: int, n_frames: int = 5, shape=(12, 256, 128), range_res_m: float = 0.0975887,
                          altitude0_m: float = 1.02, climb_m: float = 0.07, ground_amp: float = 350.0,
                          num_clutter: int = 3, noise_sigma: float = 30.0) -> np.ndarray:
    """``[n_frames, V, S, C]`` cubes of a platform over flat ground: one strong return whose range grows by ``climb_m``
    per frame (what ``Altimeter`` tracks), spread over a few Doppler lines, plus ``num_clutter`` weaker point targets
    farther out and complex Gaussian noise; integer-valued complex64 like ``synth_cube``."""
    V, S, C = shape
    rng = np.random.default_rng(seed)
    v = np.arange(V)[:, None, None]
    n = np.arange(S)[None, :, None]
    m = np.arange(C)[None, None, :]
    cubes = np.empty((n_frames,) + tuple(shape), dtype=np.complex64)
    for f in range(n_frames):
        x = np.zeros(shape, dtype=np.complex128)
        alt = altitude0_m + climb_m * f
        for dv, a in ((-0.06, 0.5), (0.0, 1.0), (0.05, 0.6)):          # ground patch: a few Doppler lines
            fr = alt / range_res_m / S
            x += a * ground_amp * np.exp(1j * (2.0 * np.pi * (fr * n + dv * m + 0.02 * v) + rng.uniform(0, 2 * np.pi)))
        for _ in range(num_clutter):
            fr = rng.uniform(2.5, 9.0) / range_res_m / S
            x += rng.uniform(30.0, 120.0) * np.exp(1j * (2.0 * np.pi * (fr * n + rng.uniform(-0.4, 0.4) * m +
                                                                        rng.uniform(-0.3, 0.3) * v) + rng.uniform(0, 2 * np.pi)))
        x += noise_sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        cubes[f] = (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)
    return cubes


# element positions (azimuth, elevation) in half wavelengths of the 12 virtual antennas, consistent with the antenna sets of
# processors/velocity_estimator.py: along an azimuth set the first coordinate counts up, along an elevation set the second
PLATFORM_LAYOUT = {
    "standard": [(k, 0) for k in range(8)] + [(k, 1) for k in range(2, 6)],
    "ods": [(0, 3), (0, 2), (1, 2), (1, 3), (2, 3), (2, 2), (3, 2), (3, 3), (2, 1), (2, 0), (3, 0), (3, 1)],
}


def synth_moving_platform_sequence(seed: int, n_frames: int, shape=(12, 256, 128), range_res_m: float = 0.0975887,
                                   vel_res_m_s: float = 0.05, geometry: str = "standard", range_window_m=(0.6, 2.4),
                                   velocities=None, num_scatterers: int = 48, noise_sigma: float = 20.0, movers=None,
                                   dropouts=()):
    """``(cubes [n_frames, V, S, C], velocities [n_frames, 2])``: a static scene seen from a moving platform.  Every frame has
    ``num_scatterers`` point scatterers of its own, spread over azimuth and elevation (+-60 degrees) at ranges inside
    ``range_window_m``; a scatterer at azimuth theta shows the Doppler velocity -(vx cos(theta) + vy sin(theta)) for the frame's
    ``(vx, vy)``, which drifts from frame to frame (``velocities=None``: vx from 0.3 up by 0.04 per frame, vy from -0.5 up by
    0.03) -- the cosine law the Doppler-azimuth velocity estimator regresses.  ``movers[f]`` of frame f's scatterers (behind the
    boresight one) move on their own: a Doppler velocity drawn from +-20 velocity bins instead of the law's.  Frames listed in
    ``dropouts`` are all zeros (a lost frame: no peak anywhere).  Antenna phases follow ``PLATFORM_LAYOUT``.
    Deterministic from ``seed``; integer-valued complex64 like ``synth_cube``."""
    V, S, C = shape
    layout = np.array(PLATFORM_LAYOUT[geometry][:V], dtype=np.float64)
    rng = np.random.default_rng(seed)
    if velocities is None:
        velocities = np.stack([0.3 + 0.04 * np.arange(n_frames), -0.5 + 0.03 * np.arange(n_frames)], axis=1)
    velocities = np.asarray(velocities, dtype=np.float64).reshape(n_frames, 2)
    n = np.arange(S)[None, :, None]
    m = np.arange(C)[None, None, :]
    cubes = np.empty((n_frames,) + tuple(shape), dtype=np.complex64)
    for f in range(n_frames):
        x = np.zeros(shape, dtype=np.complex128)
        theta = rng.uniform(-np.pi / 3, np.pi / 3, num_scatterers)
        phi = rng.uniform(-np.pi / 3, np.pi / 3, num_scatterers)
        theta[0] = phi[0] = 0.0                                       # one scatterer on boresight: the zero-azimuth peak
        rng_m = rng.uniform(range_window_m[0], range_window_m[1], num_scatterers)
        amp = rng.uniform(150.0, 400.0, num_scatterers)
        vd = -(velocities[f, 0] * np.cos(theta) + velocities[f, 1] * np.sin(theta))
        n_movers = 0 if movers is None else int(movers[f])
        vd[1:1 + n_movers] = rng.uniform(-20.0, 20.0, n_movers) * vel_res_m_s
        if f in dropouts:
            cubes[f] = 0
            continue
        for k in range(num_scatterers):
            ant = np.pi * (layout[:, 0] * np.sin(theta[k]) + layout[:, 1] * np.sin(phi[k]))[:, None, None]
            x += amp[k] * np.exp(1j * (2.0 * np.pi * (rng_m[k] / range_res_m / S * n + vd[k] / vel_res_m_s / C * m) + ant
                                       + rng.uniform(0, 2 * np.pi)))
        x += noise_sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        cubes[f] = (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)
    return cubes, velocities
