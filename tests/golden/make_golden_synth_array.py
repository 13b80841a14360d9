#!/usr/bin/env python3
"""Generate ``synth_array.npz`` from the IMPORTED reference ``SyntheticArrayBeamformerProcessor`` with the reference's own
``ConfigManager`` on ``configs/6843_RadVel_ods_10Hz.cfg`` (build container only: the reference never has to exist where the tests
run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth_array.py

The reference's ``process`` calls its Cartesian ``griddata`` step unconditionally, and that step raises ``ValueError: different
number of values and points`` for more than one elevation bin; it is presentation and plays no part in the response, so
``get_interpolated_response_cart`` is replaced ON THE INSTANCE with a no-op.  Nothing else of the reference is touched.

Configuration: receiver 1, chirp configuration 2 (virtual antenna 2 * 4 + 1 = 9), 3 frames of history, every 3rd chirp (34 of the
100 loops: raw chirps 2, 11, 20, ...; E = 102 elements), 7 azimuth bins over +-30 degrees x elevation {0, 10} degrees.  Eight
frames whose velocities open the gate at frames 2, 3 and 7 only (a gap, and the last frame).  The virtual cubes are integer-valued
complex64 ``[8, 12, 63, 100]``; only antenna 9 and a decoy antenna (5, a different scene) are non-zero, and only those two slabs
are stored.  Stored besides: the parameters, velocities, valid flags, ``array_geometry`` after every frame, the mask, the chirp
start times, the steering directions, every valid response and its peak magnitude.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.config_managers.cfgManager import ConfigManager                                      # noqa: E402
from mmwave_radar_processing.processors.simple_synthetic_array_beamformer_processor_multiFrame import (            # noqa: E402
    SyntheticArrayBeamformerProcessor)

CFG = "6843_RadVel_ods_10Hz.cfg"
PARAMS = dict(receiver_idx=1, chirp_cfg_idx=2, num_frames=3, stride=3)
AZ_DEG, EL_DEG = np.linspace(-30, 30, 7), np.array([0.0, 10.0])
VELS = np.array([[.2, .01, 0]] * 3 + [[.21, 0, .01], [.3, 0, 0]] + [[.2, 0, 0]] * 3)
LIVE = (9, 5)                # the antenna of the array, a decoy
NUM_RX, NUM_TX = 4, 3


def scene(rng, S, C, targets, noise):
    """Integer-valued I/Q like an ADC's: complex tones (range row, Doppler bin, amplitude) plus noise, rounded."""
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    x = noise * (rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
    for row, dop, amp in targets:
        x = x + amp * np.exp(2j * np.pi * ((row + 0.3) * s / S + (dop + 0.2) * c / C))
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


def raw_of(virt):
    """[V, S, loops] virtual cube -> [num_rx, S, num_tx * loops] raw cube (the inverse of VirtualArrayReformatter)."""
    V, S, L = virt.shape
    raw = np.zeros((NUM_RX, S, NUM_TX * L), dtype=np.complex64)
    for tx in range(NUM_TX):
        raw[:, :, tx::NUM_TX] = virt[tx * NUM_RX:(tx + 1) * NUM_RX]
    return raw


def main():
    cm = ConfigManager()
    cm.load_cfg(os.path.join(REF, "configs", CFG))
    p = SyntheticArrayBeamformerProcessor(cm, az_angle_bins_rad=np.deg2rad(AZ_DEG), el_angle_bins_rad=np.deg2rad(EL_DEG),
                                          min_vel=np.array([0.17, 0.0, 0.0]), max_vel=np.array([0.25, 0.05, 0.05]),
                                          max_vel_stdev=np.array([0.1, 0.1, 0.1]), **PARAMS)
    p.get_interpolated_response_cart = lambda *a, **k: None
    S, L = p.num_range_bins, cm.frameCfg_loops
    rng = np.random.default_rng(20261019)
    n = len(VELS)
    slabs = np.zeros((n, len(LIVE), S, L), dtype=np.complex64)
    for f in range(n):
        slabs[f, 0] = scene(rng, S, L, [(9 + f, 3, 60.0), (30, -7 + f, 25.0)], 2.0)
        slabs[f, 1] = scene(rng, S, L, [(50 - f, 11, 80.0)], 2.0)
    valid, geoms, frames, resps = [], [], [], []
    for f in range(n):
        virt = np.zeros((NUM_RX * NUM_TX, S, L), dtype=np.complex64)
        virt[list(LIVE)] = slabs[f]
        out = p.process(raw_of(virt), VELS[f])
        valid.append(bool(p.array_geometry_valid))
        geoms.append(p.array_geometry.copy())
        assert (out.size > 0) == valid[-1]
        if valid[-1]:
            frames.append(f)
            resps.append(np.array(out, dtype=np.complex128))
            assert np.array_equal(p.history_acd_cube_valid_chirps[-1], virt[9][:, ::PARAMS["stride"]])
    assert frames == [2, 3, 7], frames
    resps = np.stack(resps)
    path = os.path.join(HERE, "synth_array.npz")
    np.savez_compressed(path, cfg=CFG, params=np.array([PARAMS[k] for k in ("receiver_idx", "chirp_cfg_idx", "num_frames", "stride")]),
                        az_rad=np.deg2rad(AZ_DEG), el_rad=np.deg2rad(EL_DEG), min_vel=p.min_vel, max_vel=p.max_vel,
                        max_vel_stdev=p.max_vel_stdev, velocities=VELS, valid=np.array(valid), array_geometry=np.stack(geoms),
                        valid_chirps_mask=p.valid_chirps_mask, chirp_start_times_us=p.chirp_start_times_us, d=p.d,
                        lambda_m=p.lambda_m, live=np.array(LIVE), slabs=slabs, frames=np.array(frames), responses=resps,
                        peaks=np.abs(resps).reshape(len(frames), -1).max(1))
    print(path, os.path.getsize(path), "bytes; valid", valid, "peaks", np.abs(resps).reshape(len(frames), -1).max(1))


if __name__ == "__main__":
    main()
