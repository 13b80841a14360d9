#!/usr/bin/env python3
"""Generate ``micro_doppler.npz`` from the IMPORTED reference ``MicroDopplerProcessor`` (build container only: the reference never
has to exist where the tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_micro_doppler.py

The reference class reads five scalars of its config manager (``vel_max_m_s``, ``vel_res_m_s``, ``range_res_m``, ``range_max_m``,
``frameCfg_periodicity_ms``); a stub carries those of ``6843_RadVel_ods_10Hz.cfg`` (12 x 63 x 100 cubes) as
``tests/golden/cfg_scalars.json`` records them.  Stored: the scalars, the bin tables and the window mask the reference derives
from them, a sequence of 3 cubes as complex64 (what the device sees -- the reference computes on exactly those values), and per
antenna in ``rx`` the row of every frame and the reference's ``(C, H)`` buffer after every frame (H = 2 < 3 frames, so the oldest
row has already left the buffer at the end).  Antennas 0, 5 and 11 carry different scenes, the other nine are zero: they are
never read for these ``rx``, and zeros keep the file to a few hundred KB.  Frame 0 has its strongest target inside the window,
frame 1 just outside it (one row past ``row_hi``), frame 2 far outside.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.processors.micro_doppler_resp import MicroDopplerProcessor    # noqa: E402

CFG = "6843_RadVel_ods_10Hz.cfg"
TARGET_RANGES = [0, 1.0]
H = 2
RX = (0, 11)
LIVE = (0, 5, 11)


class StubConfig:
    pass


def stub_config():
    with open(os.path.join(HERE, "cfg_scalars.json")) as fh:
        ent = json.load(fh)[CFG]
    cm = StubConfig()
    for k in ("vel_max_m_s", "vel_res_m_s", "range_res_m", "range_max_m"):
        setattr(cm, k, ent["expect"][k])
    frame_cfg = [ln for ln in ent["lines"] if ln.startswith("frameCfg")][0].split()
    cm.frameCfg_periodicity_ms = float(frame_cfg[5])
    shape = (ent["expect"]["num_rx"] * ent["expect"]["num_tx"], ent["expect"]["num_samples"], ent["expect"]["loops"])
    return cm, shape


def scene(rng, S, C, targets, noise):
    """Integer-valued I/Q like an ADC's: complex tones (range row, Doppler bin, amplitude) plus noise, rounded."""
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    x = noise * (rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
    for row, dop, amp in targets:
        x = x + amp * np.exp(2j * np.pi * ((row + 0.3) * s / S + (dop + 0.2) * c / C))       # off-bin: leakage into every row
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


def main():
    cm, (V, S, C) = stub_config()
    proc = MicroDopplerProcessor(cm, target_ranges=list(TARGET_RANGES), num_frames_history=H)
    assert proc.vel_bins.shape == (C,) and proc.range_bins.shape == (S,)
    rows = np.flatnonzero(proc.range_bin_idxs_to_keep)
    lo, hi = int(rows[0]), int(rows[-1])
    assert np.array_equal(rows, np.arange(lo, hi + 1)) and hi + 1 < S
    rng = np.random.default_rng(20261019)
    strongest = [5, hi + 1, 40]                 # per frame: inside the window, one row past it, far outside
    cubes = np.zeros((3, V, S, C), dtype=np.complex64)
    for f in range(3):
        for i, v in enumerate(LIVE):
            targets = [(strongest[f], 10 + 7 * i + f, 300.0), (lo + 2 + i, 60 + f, 40.0), (hi, 90 - 3 * i, 25.0)]
            cubes[f, v] = scene(rng, S, C, targets, noise=6.0)
    d = dict(cfg=np.array(CFG), target_ranges=np.array(TARGET_RANGES, dtype=np.float64), num_frames_history=np.array(H),
             rx=np.array(RX), scalars=np.array([cm.vel_max_m_s, cm.vel_res_m_s, cm.range_res_m, cm.range_max_m,
                                                cm.frameCfg_periodicity_ms]),
             vel_bins=proc.vel_bins, range_bins=proc.range_bins, time_bins=proc.time_bins, mask=proc.range_bin_idxs_to_keep,
             rows=np.array([lo, hi]), cubes=cubes)
    out_rows = np.zeros((len(RX), 3, C))
    buffers = np.zeros((len(RX), 3, C, H))
    peaks = np.zeros((len(RX), 3))
    for i, rx in enumerate(RX):
        proc.reset()
        for f in range(3):
            buf = proc.process(cubes[f], rx_idx=rx)
            buffers[i, f] = buf
            out_rows[i, f] = buf[:, 0]
            peaks[i, f] = np.abs(np.fft.fft2(cubes[f, rx])).max()
    assert out_rows[0, 0].max() == peaks[0, 0] and out_rows[0, 1].max() < peaks[0, 1]
    d.update(out_rows=out_rows, buffers=buffers, peaks=peaks)
    path = os.path.join(HERE, "micro_doppler.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, window rows [{lo}, {hi}]")


if __name__ == "__main__":
    main()
