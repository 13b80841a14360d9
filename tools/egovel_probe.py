#!/usr/bin/env python3
"""Device point clouds and batched ego velocity on the 1250-frame batches of DESIGN.md 4.12 / 4.13 (ground= coarse parameters,
sequential= YAML parameters), on resident 12x256x128 frames:

* ``point_clouds()`` against ``point_clouds_device()`` (+ the download, ``fetch_point_clouds()``), bit equality checked;
* ``ego_velocities()`` against the per-frame loop of the mirrored ``VelocityEstimator`` (scikit-learn) fed the host point clouds
  of the first ``--loop-frames`` frames, equality of the two tracks on those frames, and the flagged share of the batch.

    python tools/egovel_probe.py [--frames 1250] [--reps 5] [--loop-frames 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.point_cloud_processing import VelocityEstimator  # noqa: E402
from mmwave_radar_processing_amd.processors.range_doppler_detection import (RangeDopplerDetectorSequential,  # noqa: E402
                                                                           RangeDopplerGroundDetector)
from ground_batch_probe import PARAMS as GROUND_PARAMS, frames as ground_frames  # noqa: E402
from seq_batch_probe import PARAMS as SEQ_PARAMS  # noqa: E402

AZ, EL = [0, 3, 4, 7], [9, 8, 5, 4]
SHAPE = (12, 256, 128)


def med(walls, F):
    w = np.array(walls)
    return {"frames_per_s": F / float(np.median(w)), "ms": float(np.median(w)) * 1e3, "ms_min": float(w.min()) * 1e3,
            "ms_max": float(w.max()) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    warnings.simplefilter("ignore")
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    F = a.frames
    ctx = _lib.default_context()
    seq_cubes = np.ascontiguousarray(np.resize(np.stack([synth.synth_cube(8000 + s) for s in range(min(125, F))]), (F,) + SHAPE))
    batches = {
        "ground": (lambda: dict(ground=RangeDopplerGroundDetector(cm, **GROUND_PARAMS["coarse"])), ground_frames(F)),
        "sequential": (lambda: dict(sequential=RangeDopplerDetectorSequential(cm, **SEQ_PARAMS["yaml"])), seq_cubes),
    }
    report = {"device": _lib.device_info(0)["name"], "frames": F, "reps": a.reps, "loop_frames": a.loop_frames}
    for name, (kw, cubes) in batches.items():
        def fresh():
            p = FramePipeline(cm, F, SHAPE, az_antenna_idxs=AZ, el_antenna_idxs=EL, **kw())
            p.load(cubes)
            return p
        host, dev = fresh(), fresh()
        want = host.point_clouds()
        dev.point_clouds_device()
        got = dev.fetch_point_clouds()
        rec = {"points_per_frame_mean": float(np.mean([len(w) for w in want])),
               "device_points_bit_identical": bool(all(x.tobytes() == y.tobytes() for x, y in zip(got, want)))}
        walls = {k: [] for k in ("point_clouds", "point_clouds_device", "point_clouds_device_fetch", "ego_velocities")}
        est = VelocityEstimator(cm)
        dev.ego_velocities(est)                                # warm-up: tables of every point count, code objects
        for _ in range(a.reps):
            for key, fn in (("point_clouds", host.point_clouds), ("point_clouds_device", dev.point_clouds_device),
                            ("point_clouds_device_fetch", lambda: (dev.point_clouds_device(), dev.fetch_point_clouds())),
                            ("ego_velocities", lambda: dev.ego_velocities(est))):
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                walls[key].append(time.perf_counter() - t0)
        for k, w in walls.items():
            rec[k] = med(w, F)
        rec["flagged_frames"] = int(dev.n_ego_flagged)
        rec["flagged_share"] = dev.n_ego_flagged / F
        rec["flag_reasons"] = {str(b): int(np.count_nonzero(dev.ego_flags & b)) for b in (1, 2, 4, 8, 16, 32)}
        # device time of the two new kernels alone
        ctx.profile_reset()
        ctx.profile_enable(1)
        dev.ego_velocities(VelocityEstimator(cm))
        ctx.sync()
        ms, n = ctx.profile_get("egovel")
        ctx.profile_enable(0)
        rec["device_ms_point_cloud_and_ransac"] = {"ms": float(ms), "launch_groups": int(n)}
        # the per-frame host loop: the mirrored estimator (scikit-learn) on the host point clouds
        n_loop = min(a.loop_frames, F)
        fresh_dev = fresh()
        track = fresh_dev.ego_velocities(VelocityEstimator(cm))
        loop_est = VelocityEstimator(cm)
        pcs = fresh().point_clouds()[:n_loop]
        t0 = time.perf_counter()
        loop = np.array([np.array(loop_est.process(points=pc)) for pc in pcs])
        rec["loop_ego_velocities"] = {"frames_per_s": n_loop / (time.perf_counter() - t0), "frames": n_loop}
        rec["track_max_abs_difference_to_loop"] = float(np.abs(track[:n_loop] - loop).max())
        rec["batch_over_loop"] = rec["ego_velocities"]["frames_per_s"] / rec["loop_ego_velocities"]["frames_per_s"]
        report[name] = rec
        print(name, json.dumps(rec), flush=True)
        for p in (host, dev, fresh_dev):
            p.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
