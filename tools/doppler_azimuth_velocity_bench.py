#!/usr/bin/env python3
"""The Doppler-azimuth velocity estimator over a resident batch -- an ods array, two directions, a moving
altitude -- on 12x256x128 and 12x63x100, coarse and precise:

* ``FramePipeline.doppler_azimuth_velocities``: host clock between two syncs around the whole call (maps, picker, RANSAC kernel,
  the host refit of flagged pairs, the state scan), the same for ``doppler_azimuth_fits``, the device time of the fit (profile
  family ``dopaz_ransac``) next to the phases it follows, and the flagged share of the (group, frame) pairs;
* the route that exists without the kernel: ``FramePipeline.doppler_azimuth_peaks`` on the whole batch, then the class's vx
  and ``lsq_fit_ego_vy_ransac`` (scikit-learn) per frame and group on the first ``--loop-frames`` frames, scaled to the batch.

One warm-up call, ``--reps`` timed calls, median / min / max.

    python tools/doppler_azimuth_velocity_bench.py [--frames 1250] [--reps 9] [--loop-frames 40] [--loop-reps 3]
                                                   [--out profiles/doppler_azimuth_velocity.json]
"""
import argparse
import copy
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, precise_ranges_from_zero_az  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors.velocity_estimator import VelocityEstimator, antenna_plan  # noqa: E402

SHAPES = [(12, 256, 128), (12, 63, 100)]
FAMILIES = ("rd", "dopaz_batch", "dopaz_zoom_batch", "dopaz_zoom_range", "dopaz_zoom_rows", "dopaz_zoom_mean", "dopaz_peaks",
            "dopaz_ransac")


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
    report = {"device": _lib.device_info(0)["name"], "frames": F, "cases": []}
    for V, S, C in SHAPES:
        cm = ConfigManager()
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C), array_geometry="ods")
        res = cm.range_res_m
        make = lambda: VelocityEstimator(cm, lower_range_bound=5 * res, upper_range_bound=15 * res)   # noqa: E731
        est = make()
        sets, groups, shifts = antenna_plan(cm)
        G = len(groups)
        pipe = FramePipeline(cm, F, (V, S, C))
        # scenes of a moving platform, a block of frames repeated to fill the batch (the work per frame does not depend on it)
        block = min(F, 50)
        f = np.arange(block)
        vel = np.stack([0.3 + 0.6 * f, -12.0 + 0.5 * f], axis=1) * cm.vel_res_m_s
        alt = (8 + (np.arange(F) * 7) % max(S - 30, 1)) * res            # the altitude wanders through the range axis
        cubes = np.concatenate([synth.synth_moving_platform_sequence(
            4000 + k, 1, (V, S, C), res, cm.vel_res_m_s, "ods", (alt[k] - 4 * res, alt[k] + 14 * res), vel[k:k + 1],
            num_scatterers=96, movers=[12 if k % 5 == 1 else 0])[0] for k in range(block)])
        pipe.load(np.concatenate([cubes] * (-(-F // block)))[:F])
        alt = np.concatenate([alt[:block]] * (-(-F // block)))[:F]
        L = min(a.loop_frames, F)
        for mode, precise in (("coarse", False), ("precise", True)):
            case = {"shape": [V, S, C], "mode": mode}
            whole = lambda: pipe.doppler_azimuth_velocities(make(), alt, precise)      # noqa: E731
            fits_call = lambda: pipe.doppler_azimuth_fits(est, alt, precise)           # noqa: E731
            case["velocities_call"] = timed(ctx, whole, a.reps)
            case["fits_call"] = timed(ctx, fits_call, a.reps)
            case["device_ms"] = families_ms(ctx, fits_call, 3)
            fits, status = fits_call()
            case["flagged_pairs"] = int(pipe.n_dopaz_fits_flagged)
            case["flagged_share"] = pipe.n_dopaz_fits_flagged / float(status.size)
            case["status_counts"] = [int(np.count_nonzero(status == k)) for k in range(3)]
            case["rows_per_frame"] = int(pipe.dopaz_peak_maps[1][2])
            # the route without the kernel: the peak lists of the whole batch, then the class's fit per frame and group
            wins = np.stack([est.get_range_window(altitude=x, sensing_direction=cm.array_direction) for x in alt])

            def peaks_call():
                pv = None
                if precise:
                    _, z = pipe.doppler_azimuth_peaks(est, sets, groups, wins, shifts, None, est.peak_threshold_dB)
                    pv = precise_ranges_from_zero_az(z[0], z[1] if G == 2 else None, est.precise_vel_bound)
                return pipe.doppler_azimuth_peaks(est, sets, groups, wins, shifts, pv, est.peak_threshold_dB)

            case["peaks_call"] = timed(ctx, peaks_call, max(1, a.reps // 3))
            rows, zero = peaks_call()
            walls, same = [], True
            tmp = copy.copy(est)
            for rep in range(a.loop_reps + 1):
                t0 = time.perf_counter()
                for k in range(L):
                    tmp.azimuth_peak_zero_az = zero[0][k]
                    tmp.elevation_peak_zero_az = zero[1][k] if G == 2 else np.empty((0, 2))
                    vx = tmp.estimate_ego_vx_velocity()
                    for g in range(G):
                        if rows[g][k].shape[0] == 0:
                            continue
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            fit = tmp.lsq_fit_ego_vy_ransac(peaks=rows[g][k])
                        if rep == 0 and status[k, g] == _lib.DOPAZ_STATUS_OK:
                            same = same and fits[k, g, 0] == vx and fits[k, g, 3] == fit[2] and \
                                abs(fits[k, g, 1] - fit[0]) <= 1e-12 * max(1.0, abs(fit[0]))
                if rep:
                    walls.append(time.perf_counter() - t0)
            st = stats(walls)
            case["host_fits"] = dict(st, frames=L, ms_per_frame=st["ms"] / L, ms_scaled_to_batch=st["ms"] / L * F)
            case["parent_route_ms"] = case["peaks_call"]["ms"] + case["host_fits"]["ms_scaled_to_batch"]
            case["equal_to_host_fits_on_loop_frames"] = bool(same)
            report["cases"].append(case)
            print(json.dumps(case), flush=True)
        pipe.bufs.free()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
