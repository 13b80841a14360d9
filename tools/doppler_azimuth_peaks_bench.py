#!/usr/bin/env python3
"""Peak picking on the Doppler-azimuth maps of a resident batch -- the ODS ego-velocity case of tools/doppler_azimuth_bench.py: four
sets of four antennas, two groups (azimuth pair, elevation pair), a window of 20 range rows centred somewhere else in every frame,
a zoom range of its own per frame -- on 12x256x128 and 12x63x100, coarse and precise:

* ``FramePipeline.doppler_azimuth_peaks``: host clock between two syncs around the whole call (maps, kernel, the two index tables
  downloaded, the per-frame arrays built), the same for ``doppler_azimuth_peaks_device`` (no per-frame arrays), and the device
  time of the picker (profile family ``dopaz_peaks``) next to the phases of the maps it follows (``rd``, ``dopaz_batch``;
  ``dopaz_zoom_range``, ``dopaz_zoom_rows``, ``dopaz_zoom_mean``);
* the route without the kernel: ``FramePipeline.doppler_azimuth`` on the whole batch (maps downloaded and widened), then
  ``detect_peaks_rows`` / ``detect_peak_zero_az`` per frame and group on the first ``--loop-frames`` frames, scaled to the batch.

Also recorded: the undecided (group, frame) pairs of the run, and whether the peaks of the loop frames equal the host pickers'.

One warm-up call, ``--reps`` timed calls, median / min / max.

    python tools/doppler_azimuth_peaks_bench.py [--frames 1250] [--reps 9] [--loop-frames 40] [--loop-reps 3]
                                                [--out profiles/doppler_azimuth_peaks.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor  # noqa: E402

SHAPES = [(12, 256, 128), (12, 63, 100)]
SETS = [[0, 3, 4, 7], [1, 2, 5, 6], [10, 11, 6, 7], [9, 8, 5, 4]]
SHIFTS = [True, True, False, False]
GROUPS = [(0, 1), (2, 3)]
ROWS = 20
FAMILIES = ("rd", "dopaz_batch", "dopaz_zoom_batch", "dopaz_zoom_range", "dopaz_zoom_rows", "dopaz_zoom_mean", "dopaz_peaks")


def stats(walls):
    w = np.array(walls) * 1e3
    return {"ms": float(np.median(w)), "ms_min": float(w.min()), "ms_max": float(w.max()), "reps": len(w)}


def timed(ctx, fn, reps):
    fn()                                        # warm-up: code objects, tables, buffers
    walls = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    return stats(walls)


def families_ms(ctx, fn, reps):
    """Device milliseconds per call of every profile family the call touches."""
    ctx.profile_reset()
    ctx.profile_enable(1)
    for _ in range(reps):
        fn()
    ctx.sync()
    out = {}
    for name in FAMILIES:
        ms, n = ctx.profile_get(name)
        if n:
            out[name] = float(ms) / reps
    ctx.profile_enable(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=40)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "frames": F, "sets": SETS, "groups": GROUPS, "window_rows": ROWS, "cases": []}
    for V, S, C in SHAPES:
        cm = ConfigManager()
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C), array_geometry="ods")
        proc = DopplerAzimuthProcessor(cm)
        pipe = FramePipeline(cm, F, (V, S, C))
        pipe.synth(F, seed0=7000)
        res = cm.range_res_m
        lo = 2 + (np.arange(F) * 7) % (S - ROWS - 4)                   # the altitude wanders through the range axis
        wins = np.stack([(lo - 0.25) * res, (lo + ROWS - 0.75) * res], axis=1)
        centre = -0.5 + (np.arange(F) % 11) * 0.1                       # the coarse estimate the zoom is centred on
        vrs = np.stack([centre - 0.25, centre + 0.25], axis=1)
        L = min(a.loop_frames, F)
        for mode, pv in (("coarse", None), ("precise", vrs)):
            case = {"shape": [V, S, C], "mode": mode}
            whole = lambda: pipe.doppler_azimuth_peaks(proc, SETS, GROUPS, wins, SHIFTS, pv)           # noqa: E731
            tables = lambda: pipe.doppler_azimuth_peaks_device(proc, SETS, GROUPS, wins, SHIFTS, pv)   # noqa: E731
            case["peaks_call"] = timed(ctx, whole, a.reps)
            case["peaks_device_call"] = timed(ctx, tables, a.reps)
            case["device_ms"] = families_ms(ctx, tables, 3)
            rows, zero = whole()
            case["undecided"] = pipe.n_peaks_undecided
            case["row_peaks_per_frame"] = float(np.mean([len(rows[g][f]) for g in range(len(GROUPS)) for f in range(F)]))
            case["rows_per_frame"] = int(pipe.dopaz_peak_maps[1][2])
            # the route without the kernel: all maps to the host, the scipy pickers per frame and group
            maps_call = lambda: pipe.doppler_azimuth(proc, SETS, wins, SHIFTS, pv)                     # noqa: E731
            case["maps_to_host_call"] = timed(ctx, maps_call, max(1, a.reps // 3))
            got = maps_call()
            maps, bins = got if pv is not None else (got, [proc.vel_bins] * F)
            walls, same = [], True
            for rep in range(a.loop_reps + 1):
                t0 = time.perf_counter()
                for f in range(L):
                    mf = maps[f] if isinstance(maps, list) else maps[:, f]
                    for g, (s1, s2) in enumerate(GROUPS):
                        resp = (mf[s1] + mf[s2]) / 2
                        r = proc.detect_peaks_rows(resp, bins[f], 30.0)
                        z = proc.detect_peak_zero_az(resp, bins[f], 30.0)
                        if rep == 0:
                            same = same and np.array_equal(r, rows[g][f]) and np.array_equal(z, zero[g][f])
                if rep:
                    walls.append(time.perf_counter() - t0)
            st = stats(walls)
            case["host_pickers"] = dict(st, frames=L, ms_per_frame=st["ms"] / L, ms_scaled_to_batch=st["ms"] / L * F)
            case["parent_route_ms"] = case["maps_to_host_call"]["ms"] + case["host_pickers"]["ms_scaled_to_batch"]
            case["equal_to_host_pickers_on_loop_frames"] = bool(same)
            del maps, got
            report["cases"].append(case)
            print(json.dumps(case), flush=True)
        pipe.bufs.free()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
