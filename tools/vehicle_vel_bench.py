#!/usr/bin/env python3
"""Batched VehicleVelEstimator RANSAC against the host class over the same frames.

    python tools/vehicle_vel_bench.py [--frames 1250] [--points 200] [--reps 5] [--host-frames 100] [--out profiles/vehicle_vel.json]

Frames are seeded synthetic scenes (static points seen at a drifting ego velocity, a tenth of them movers, continuous
coordinates), max_iters = 100, 2-D.  Timed, host clock around calls that end in a device-to-host copy, median of ``reps`` calls
after one warm-up call: ``vehicle_fits`` on uploaded point clouds unchained and chained (the upload and the draw tables are part of
the call; the tables are cached after the warm-up), the kernel alone from the library profiler, and the host class's
``estimate_ego_vel`` loop over the first ``host-frames`` frames, unchained and chained.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmwave_radar_processing_amd import _lib, synth                                        # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline                                # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager                      # noqa: E402
from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator         # noqa: E402


def scene(rng, n, u, movers=0.1):
    az, el, r = rng.uniform(-1.0, 1.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 9.0, n)
    p = np.column_stack((r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)))
    v = -(p / np.linalg.norm(p, axis=1, keepdims=True)) @ np.asarray(u) + rng.normal(0.0, 0.02, n)
    k = int(round(movers * n))
    v[rng.permutation(n)[:k]] = rng.uniform(-5.0, 5.0, k)
    return np.column_stack((p, v))


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=100)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    frames = [scene(rng, int(rng.integers(args.points - 20, args.points + 21)), (1.0 + 4e-4 * f, -0.3, 0.0)) for f in range(args.frames)]
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=16, num_loops=8))
    pipe = FramePipeline(cm, args.frames, (4, 16, 8), det_capacity=args.points + 24)
    est = VehicleVelEstimator(seed=args.seed)
    res = dict(device=_lib.device_info(0)["name"], frames=args.frames, points=args.points, max_iters=est.max_iters, dim=2,
               seed=args.seed, reps=args.reps, label="builder-run")
    for name, track in (("batch", False), ("chain", True)):
        res[name] = median_ms(lambda: pipe.vehicle_fits(est, frames, track=track), args.reps)
        res[name]["flagged"] = int(pipe.n_vehicle_flagged)
        res[name]["frames_per_s"] = args.frames / res[name]["median_ms"] * 1e3
        pipe.ctx.profile_reset()
        pipe.ctx.profile_enable(True)
        fits, status = pipe.vehicle_fits(est, frames, track=track)
        pipe.ctx.sync()
        ms, n = pipe.ctx.profile_get("vehicle_vel")
        pipe.ctx.profile_enable(False)
        res[name].update(kernel_ms=float(ms), kernel_launches=int(n), found=int(status.sum()))
        res[name + "_fits"] = fits
    H = min(args.host_frames, args.frames)
    for name, track in (("host_batch", False), ("host_chain", True)):
        host, prev, rows = VehicleVelEstimator(seed=args.seed), np.empty(0), []
        t0 = time.perf_counter()
        for pts in frames[:H]:
            v = host.estimate_ego_vel(pts, prev if track else np.empty(0))
            rows.append(v if v.size else np.full(2, np.nan))
            prev = v if v.size else prev
        dt = time.perf_counter() - t0
        res[name] = dict(frames=H, ms=dt * 1e3, frames_per_s=H / dt)
        dev = res[("chain" if track else "batch") + "_fits"][:H, :2]
        ok = ~np.isnan(np.array(rows)[:, 0])
        res[name]["max_abs_difference_to_device"] = float(np.abs(np.array(rows)[ok] - dev[ok]).max()) if ok.any() else 0.0
    for name in ("batch", "chain"):
        del res[name + "_fits"]
        res[name]["speedup_over_host_loop"] = res[name]["frames_per_s"] / res["host_" + name]["frames_per_s"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
