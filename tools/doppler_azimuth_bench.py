#!/usr/bin/env python3
"""Doppler-azimuth maps of a resident batch for the ODS ego-velocity case -- four sets of four antennas, a window of 20 range rows
centred somewhere else in every frame, a zoom range of its own per frame -- on 12x256x128 and 12x63x100:

* ``FramePipeline.doppler_azimuth_device`` in coarse and in precise mode: host clock between two syncs around the call (tables
  included), and the device time of each phase from the profile families (``rd``, ``dopaz_batch``; ``dopaz_zoom_range``,
  ``dopaz_zoom_rows``, ``dopaz_zoom_mean`` inside ``dopaz_zoom_batch``);
* baseline 1: the per-frame ``DopplerAzimuthProcessor.process`` loop producing the same maps (all four sets, host cubes) on the
  first ``--loop-frames`` frames, scaled to the batch;
* baseline 2, the floor of the coarse entry: ``mmw_doppler_azimuth`` on four pre-gathered ``[F, 4, S, C]`` subset cubes with one
  window of 20 rows shared by all frames (the gather and its upload are not timed).

Also recorded: the worst difference, relative to the map's peak, between the batch maps and the loop's on the loop frames.

One warm-up call, ``--reps`` timed calls, median / min / max; the loop is one warm-up pass and ``--loop-reps`` timed passes.

    python tools/doppler_azimuth_bench.py [--frames 1250] [--reps 9] [--loop-frames 40] [--loop-reps 3]
                                          [--out profiles/doppler_azimuth_batch.json]
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
ROWS = 20
FAMILIES = ("rd", "dopaz_batch", "dopaz_zoom_batch", "dopaz_zoom_range", "dopaz_zoom_rows", "dopaz_zoom_mean")


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
    report = {"device": _lib.device_info(0)["name"], "frames": F, "sets": SETS, "window_rows": ROWS, "cases": []}
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
        case = {"shape": [V, S, C]}
        coarse = lambda: pipe.doppler_azimuth_device(proc, SETS, wins, SHIFTS)                 # noqa: E731
        precise = lambda: pipe.doppler_azimuth_device(proc, SETS, wins, SHIFTS, vrs)           # noqa: E731
        case["coarse_call"] = timed(ctx, coarse, a.reps)
        case["coarse_device_ms"] = families_ms(ctx, coarse, 3)
        case["precise_call"] = timed(ctx, precise, a.reps)
        case["precise_device_ms"] = families_ms(ctx, precise, 3)
        case["zoom_bins_per_frame"] = int(precise()[1][2])
        # baseline 2: the single-window entry on pre-gathered subset cubes
        n = min(F, 1250)
        host = pipe.cubes(0, n)
        subs = [ctx.alloc(n * 4 * S * C * 8) for _ in SETS]
        for d, rx in zip(subs, SETS):
            d.upload(np.ascontiguousarray(host[:, rx]))
        d_out = ctx.alloc(n * C * 64 * 4)

        def floor():
            for d, sh in zip(subs, SHIFTS):
                _lib.check(ctx.lib.mmw_doppler_azimuth(ctx.handle, d.ptr, d_out.ptr, n, 4, S, C, 64, 10, 10 + ROWS,
                                                       _lib.ANGLE_NO_WINDOW | (0 if sh else _lib.ANGLE_NO_SHIFT)))
        case["floor_pre_gathered_shared_window"] = dict(timed(ctx, floor, a.reps), frames=n, device_ms=families_ms(ctx, floor, 3))
        for d in subs + [d_out]:
            d.free()
        # baseline 1: the per-frame loop, and the difference between its maps and the batch's
        L = min(a.loop_frames, n)
        got_c = pipe.doppler_azimuth(proc, SETS, wins, SHIFTS)
        got_p, _ = pipe.doppler_azimuth(proc, SETS, wins, SHIFTS, vrs)
        worst = {"coarse": 0.0, "precise": 0.0}
        for mode, kw in (("coarse", {}), ("precise", {"use_precise_fft": True})):
            walls = []
            for rep in range(a.loop_reps + 1):
                t0 = time.perf_counter()
                for f in range(L):
                    for k, (rx, sh) in enumerate(zip(SETS, SHIFTS)):
                        if mode == "precise":
                            kw["precise_vel_range"] = vrs[f]
                        m = proc.process(host[f], rx_antennas=rx, range_window=wins[f], shift_angle=sh, **kw)
                        if rep == 0:
                            mine = got_c[k, f] if mode == "coarse" else (got_p[k, f] if isinstance(got_p, np.ndarray) else got_p[f][k])
                            d = float(np.max(np.abs(mine - m)) / np.max(m))
                            worst[mode] = worst[mode] if d <= worst[mode] else d        # (a NaN stays visible)
                if rep:
                    walls.append(time.perf_counter() - t0)
            st = stats(walls)
            case[f"loop_{mode}"] = dict(st, frames=L, ms_per_frame=st["ms"] / L, ms_scaled_to_batch=st["ms"] / L * F)
        case["worst_difference_to_loop"] = worst
        report["cases"].append(case)
        pipe.bufs.free()
        print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
