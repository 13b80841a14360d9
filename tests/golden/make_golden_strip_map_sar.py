#!/usr/bin/env python3
"""Generate ``strip_map_sar.npz`` from the IMPORTED reference ``StripMapSARProcessor`` (build container only: the reference never
has to exist where the tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_strip_map_sar.py

Two configurations out of ``tests/golden/cfg_scalars.json`` (their cfg command lines are what that file records):
``6843_RadVel_ods_20Hz.cfg`` (12 x 63 x 70) and the synthetic 12 x 256 x 128 one.  Both enable virtual antennas, so the
reference's ``process`` takes the RAW ``[4, S, 3 C]`` cube; one raw cube per configuration is stored as complex64 with only the
samples of the virtual antennas in ``LIVE`` non-zero (the others are never read for the recorded ``rx_index`` values, and zeros
keep the file small).  Per call: the velocity, height, distance and antenna, the start / stop of both slices as the reference
left them, ``ground_range_bins``, ``ground_az_bins_rad``, ``angle_bins_rad`` and the complex128 slice.  The velocities are
searched for, not guessed: between them the calls of a configuration must show a wide window, a single column, an empty one
(the platform at rest: every angle bin is infinite or NaN and NumPy's argmin puts both ends on one index), a negative velocity
and one that touches column 0 or C - 1; one call uses a non-default height and distance.  The amplitudes are small (a few bits
per sample) so that the cubes compress.  Calls marked
``geometry only`` (non-finite speed, negative zero) record what NumPy makes of the reference's expressions, slices and bins alike.
"""
import json
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.config_managers.cfgManager import ConfigManager                      # noqa: E402
from mmwave_radar_processing.processors.strip_map_SAR_processor import StripMapSARProcessor      # noqa: E402

CFGS = {"ods": "6843_RadVel_ods_20Hz.cfg", "synth": "__synth_256x128x12__"}
LIVE = {"ods": (0, 5), "synth": (0,)}                  # virtual antennas with samples
CANDIDATES = [0.02, 0.05, 0.1, 0.2, 0.35, 0.5, 0.8, 1.0, 1.5, 2.5, 4.0, 7.0, 12.0, 20.0, 35.0, 60.0]
GEOMETRY_ONLY = [float("inf"), float("nan"), -0.0]


def load_cm(lines):
    with tempfile.NamedTemporaryFile("w", suffix=".cfg", delete=False) as fh:
        fh.write("\n".join(lines) + "\n")
        path = fh.name
    cm = ConfigManager()
    cm.load_cfg(path)
    os.unlink(path)
    return cm


def raw_scene(rng, num_rx, num_tx, S, C, live):
    """Integer-valued I/Q: three off-bin tones plus noise on each live virtual antenna (t * num_rx + r <-> rx r, chirps t::num_tx)."""
    raw = np.zeros((num_rx, S, num_tx * C), dtype=np.complex64)
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    for n, v in enumerate(live):
        t, r = divmod(v, num_rx)
        x = 1.0 * (rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
        for row, dop, amp in ((S * 0.08 + n, 2.3, 12.0), (S * 0.15, -3.4 - n, 7.0), (S * 0.5, C * 0.4, 10.0)):
            x = x + amp * np.exp(2j * np.pi * (row * s / S + dop * c / C))
        raw[r, :, t::num_tx] = (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)
    return raw


def window_of(proc, v, h=0.24, d=1.5):
    proc.configure_array_geometry(vel_m_per_s=v, sensor_height_m=h, max_SAR_distance=d)
    a = proc.valid_angles_slice
    return int(a.start), int(a.stop)


def pick(proc, C):
    """Velocities of the five kinds, found by trying the candidates on the reference's own geometry."""
    width = {v: window_of(proc, v) for v in CANDIDATES}
    wide = max(CANDIDATES, key=lambda v: width[v][1] - width[v][0])
    single = [v for v in CANDIDATES if width[v][1] - width[v][0] == 1]
    width[0.0] = window_of(proc, 0.0)      # an even C has no centre bin for both angles to share; a platform at rest has no bins at all
    empty = [v for v in (0.0,) if width[v][1] == width[v][0]]
    touch = [v for v in CANDIDATES if width[v][0] == 0 or width[v][1] == C - 1]
    mid = [v for v in CANDIDATES if 1 < width[v][1] - width[v][0] < C // 2]
    assert single and empty and touch and mid, (width, "a kind of window is missing")
    assert width[wide][1] - width[wide][0] >= C // 2
    kinds = dict(wide=wide, single=single[0], empty=empty[-1], negative=-mid[len(mid) // 2], touching=touch[0])
    if wide in touch:                       # one call shows both: the widest window starts at column 0
        del kinds["wide"], kinds["touching"]
        kinds = {"wide and touching": wide, **kinds}
    return kinds


def main():
    with open(os.path.join(HERE, "cfg_scalars.json")) as fh:
        table = json.load(fh)
    rng = np.random.default_rng(20261020)
    d = {}
    warnings.simplefilter("ignore")
    for tag, name in CFGS.items():
        ent = table[name]
        cm = load_cm(ent["lines"])
        e = ent["expect"]
        num_rx, num_tx, S, C = e["num_rx"], e["num_tx"], e["num_samples"], e["loops"]
        proc = StripMapSARProcessor(cm)
        assert cm.virtual_antennas_enabled and proc.phase_shifts.shape == (C,) and proc.range_bins.shape == (S,)
        raw = raw_scene(rng, num_rx, num_tx, S, C, LIVE[tag])
        kinds = pick(proc, C)
        calls = [(k, v, 0.24, 1.5, LIVE[tag][i % len(LIVE[tag])]) for i, (k, v) in enumerate(kinds.items())]
        calls.append(("custom", kinds["negative"] * -1.5, 0.4, 1.1, LIVE[tag][-1]))
        calls += [("geometry only", v, 0.24, 1.5, 0) for v in GEOMETRY_ONLY]
        d[f"{tag}_cfg"] = np.array(name)
        d[f"{tag}_raw"] = raw
        d[f"{tag}_tables"] = np.array([proc.lambda_m, proc.chirp_period_us, proc.chirps_per_frame])
        d[f"{tag}_phase_shifts"], d[f"{tag}_range_bins"] = proc.phase_shifts, proc.range_bins
        d[f"{tag}_kinds"] = np.array([c[0] for c in calls])
        d[f"{tag}_params"] = np.array([c[1:4] for c in calls], dtype=np.float64)
        d[f"{tag}_rx"] = np.array([c[4] for c in calls])
        slices = np.zeros((len(calls), 4), dtype=np.int64)
        for i, (kind, v, h, dist, rx) in enumerate(calls):
            if kind == "geometry only":
                proc.configure_array_geometry(vel_m_per_s=v, sensor_height_m=h, max_SAR_distance=dist)
            else:
                out = proc.process(raw, vel_m_per_s=v, sensor_height_m=h, rx_index=rx, max_SAR_distance=dist)
                assert out.dtype == np.complex128
                d[f"{tag}_{i}_out"] = out
            r, a = proc.valid_ranges_slice, proc.valid_angles_slice
            slices[i] = [r.start, r.stop, a.start, a.stop]
            d[f"{tag}_{i}_ground_range"], d[f"{tag}_{i}_ground_az"] = proc.ground_range_bins, proc.ground_az_bins_rad
            d[f"{tag}_{i}_angle_bins"] = proc.angle_bins_rad
            print(f"{tag} {kind:14s} v={v:7.3f} rows [{r.start}, {r.stop}) cols [{a.start}, {a.stop})")
        d[f"{tag}_slices"] = slices
        # no range bin qualifies: the reference's IndexError
        for h, dist in ((1e3, 1.5), (0.24, -1.0)):
            try:
                proc.configure_array_geometry(vel_m_per_s=1.0, sensor_height_m=h, max_SAR_distance=dist)
            except IndexError:
                continue
            raise AssertionError("expected IndexError")
    path = os.path.join(HERE, "strip_map_sar.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size / 1024:.0f} KiB")
    assert size <= os.path.getsize(os.path.join(HERE, "micro_doppler.npz"))


if __name__ == "__main__":
    main()
