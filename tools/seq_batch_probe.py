#!/usr/bin/env python3
"""Throughput of the batched sequential detector (FramePipeline(sequential=...)) against the per-frame loop.

    python tools/seq_batch_probe.py [--frames 1250] [--reps 7] [--loop-frames 300] [--out FILE.json]

Reports, for the YAML_SEQ and GOSO_SEQ parameter sets, frames/s of detect() and point_clouds() on resident 12x256x128
frames by the row kernel (MMW_SEQ_FULL_PLANE=0) and by the full-plane route (=1), the two alternated repetition by
repetition in one run (median, minimum and maximum of the wall times, downloads and host assembly included), the device
time of the detection launches alone (HIP-event spans of the library's profiler), and frames/s of
RangeDopplerDetectorSequential.process / PointCloudGenerator.process called frame by frame.
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
from mmwave_radar_processing_amd.processors import PointCloudGenerator  # noqa: E402
from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerDetectorSequential  # noqa: E402

PARAMS = {
    "yaml": dict(rng_cfar_type="os_cfar_1d", rng_cfar_params={"num_train": 5, "num_guard": 3, "rho": 0.6, "alpha": 2},
                 vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 5, "num_guard": 2, "rho": 0.7, "alpha": 3}),
    "goso": dict(rng_cfar_type="go_cfar_1d", rng_cfar_params={"num_train": 8, "num_guard": 2, "pfa": 1e-3},
                 vel_cfar_type="so_cfar_1d", vel_cfar_params={"num_train": 6, "num_guard": 2, "pfa": 1e-4}),
}
AZ, EL = [0, 3, 4, 7], [9, 8, 5, 4]
SHAPE = (12, 256, 128)
ROUTES = {"row_kernel": 0, "full_plane": 1}


def stats(walls, F):
    w = np.array(walls)
    return {"frames_per_s": F / float(np.median(w)), "ms": float(np.median(w)) * 1e3, "ms_min": float(w.min()) * 1e3,
            "ms_max": float(w.max()) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--distinct", type=int, default=125)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-frames", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    base = np.stack([synth.synth_cube(8000 + s) for s in range(min(a.distinct, a.frames))])
    cubes = np.ascontiguousarray(np.resize(base, (a.frames,) + SHAPE))
    F = cubes.shape[0]
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "frames": F, "distinct_frames": int(base.shape[0]), "shape": list(SHAPE),
              "reps": a.reps}
    for name, params in PARAMS.items():
        p = FramePipeline(cm, F, SHAPE, sequential=RangeDopplerDetectorSequential(cm, **params), az_antenna_idxs=AZ,
                          el_antenna_idxs=EL)
        p.load(cubes)
        walls = {(r, w): [] for r in ROUTES for w in ("detect", "point_clouds")}
        lists = {}
        for r, v in ROUTES.items():                       # warm-up: buffers, tables, code objects of both routes
            ctx.set_option("MMW_SEQ_FULL_PLANE", v)
            lists[r] = p.detect()
            p.point_clouds()
        same = all(np.array_equal(x, y) for x, y in zip(lists["row_kernel"], lists["full_plane"]))
        for _ in range(a.reps):                           # the two routes alternate
            for r, v in ROUTES.items():
                ctx.set_option("MMW_SEQ_FULL_PLANE", v)
                for what in ("detect", "point_clouds"):
                    ctx.sync()
                    t0 = time.perf_counter()
                    getattr(p, what)()
                    walls[(r, what)].append(time.perf_counter() - t0)
        rec = {"detections_per_batch": int(sum(d.shape[0] for d in lists["row_kernel"])), "routes_identical": bool(same),
               "rows_per_frame_mean": float(p.bufs.get("s_nrows", F * 4).download((F,), np.int32).mean())}
        for r in ROUTES:
            rec[r] = {what: stats(walls[(r, what)], F) for what in ("detect", "point_clouds")}
        # device time of the launches alone, per scope of the library's profiler, one detect() per route
        for r, v in ROUTES.items():
            ctx.set_option("MMW_SEQ_FULL_PLANE", v)
            ctx.profile_reset()
            ctx.profile_enable(1)
            p.detect()
            ctx.sync()
            spans = {}
            for scope in ("seq", "rd64", "cfar", "compact"):
                ms, n = ctx.profile_get(scope)
                if n:
                    spans[scope] = {"ms": float(ms), "launch_groups": int(n)}
            ctx.profile_enable(0)
            rec[r]["device_ms_by_scope"] = spans
        ctx.set_option("MMW_SEQ_FULL_PLANE", None)
        # the per-frame loops the reference's scripts run
        n_loop = min(a.loop_frames, F)
        det = RangeDopplerDetectorSequential(cm, **params)
        pcg = PointCloudGenerator(cm, az_antenna_idxs=AZ, el_antenna_idxs=EL, detector_type="range_doppler_detector_sequential",
                                  detector_params=params)
        for worker, key in ((det, "loop_detect"), (pcg, "loop_point_clouds")):
            for f in range(3):
                worker.process(cubes[f])
            t0 = time.perf_counter()
            for f in range(n_loop):
                worker.process(cubes[f])
            rec[key] = {"frames_per_s": n_loop / (time.perf_counter() - t0), "frames": n_loop}
        for r in ROUTES:
            rec[r]["speedup_detect_vs_loop"] = rec[r]["detect"]["frames_per_s"] / rec["loop_detect"]["frames_per_s"]
            rec[r]["speedup_point_clouds_vs_loop"] = rec[r]["point_clouds"]["frames_per_s"] / rec["loop_point_clouds"]["frames_per_s"]
        report[name] = rec
        print(name, json.dumps(rec), flush=True)
        p.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
