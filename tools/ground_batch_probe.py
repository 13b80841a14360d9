#!/usr/bin/env python3
"""Throughput of the batched ground detector (FramePipeline(ground=...)) against the per-frame loop.

    python tools/ground_batch_probe.py [--frames 1250] [--reps 5] [--loop-frames 200] [--out FILE.json]

Reports frames/s of point_clouds() on resident 12x256x128 frames, of stream() over int16 raw chunks, of
PointCloudGenerator(detector_type="range_doppler_ground_detector").process frame by frame, and the share of the host's
serial part (the Altimeter scan + the gate table) in the batch's wall time, for the precise and the coarse parameter sets.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, ground_gates  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors import PointCloudGenerator  # noqa: E402
from mmwave_radar_processing_amd.processors.range_doppler_detection import RangeDopplerGroundDetector  # noqa: E402

PARAMS = {
    "precise": dict(vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 16, "num_guard": 4, "rho": 0.5, "alpha": 12},
                    altimeter_params={"min_altitude_m": 0.6, "zoom_search_region_m": 0.2, "altitude_search_limit_m": 0.6,
                                      "range_bias": 0.03, "precise_est_enabled": True}),
    "coarse": dict(vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 12, "num_guard": 4, "rho": 0.5, "alpha": 6},
                   altimeter_params={"min_altitude_m": 0.6, "zoom_search_region_m": 0.2, "altitude_search_limit_m": 0.6,
                                     "range_bias": 0.0, "precise_est_enabled": False}),
}
AZ, EL = [0, 3, 4, 7], [9, 8, 5, 4]
SHAPE = (12, 256, 128)


def frames(n):
    """n frames of a platform climbing from 0.7 m and back (125 distinct frames, repeated)."""
    base = np.concatenate([synth.synth_ground_sequence(700, 75, altitude0_m=0.7, climb_m=0.04),
                           synth.synth_ground_sequence(701, 50, altitude0_m=3.7, climb_m=-0.06)])
    return np.ascontiguousarray(np.resize(base, (n,) + SHAPE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    cubes = frames(a.frames)
    F = cubes.shape[0]
    num_tx, num_rx = 3, 4
    raw = np.empty((F, num_rx, SHAPE[1], num_tx * SHAPE[2]), dtype=np.complex64)
    for t in range(num_tx):
        raw[:, :, :, t::num_tx] = cubes[:, t * num_rx:(t + 1) * num_rx]
    iq = np.ascontiguousarray(np.stack([raw.real, raw.imag], axis=-1).astype(np.int16))
    del raw
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "frames": F, "shape": list(SHAPE), "reps": a.reps}
    for name, params in PARAMS.items():
        det = RangeDopplerGroundDetector(cm, **params)
        p = FramePipeline(cm, F, SHAPE, ground=det, az_antenna_idxs=AZ, el_antenna_idxs=EL)
        p.load(cubes)
        p.point_clouds()                                  # warm-up: buffers, tables, code objects
        walls, points = [], 0
        for _ in range(a.reps):
            det.reset()
            ctx.sync()
            t0 = time.perf_counter()
            pcs = p.point_clouds()
            walls.append(time.perf_counter() - t0)
            points += sum(pc.shape[0] for pc in pcs)
        wall = float(np.median(walls))
        # the serial host part: the Altimeter scan over F frames' candidate lists + the gate table, timed alone
        cand = [[float(x) for x in c] for c in p._scan_inputs[0]]
        fine = p._scan_inputs[1]
        scans = []
        for _ in range(max(a.reps, 5)):
            det.reset()
            t0 = time.perf_counter()
            alts = det.altimeter.lock.advance(cand, fine)
            ground_gates(det.range_bins, np.array(alts))
            scans.append(time.perf_counter() - t0)
        scan = float(np.median(scans))
        # int16 raw chunks through stream()
        chunk = max(1, F // 5)
        ps = FramePipeline(cm, chunk, SHAPE, ground=RangeDopplerGroundDetector(cm, **params), az_antenna_idxs=AZ,
                           el_antenna_idxs=EL)
        list(ps.stream([iq[i:i + chunk] for i in range(0, F, chunk)], num_tx=num_tx))       # warm-up
        t0 = time.perf_counter()
        list(ps.stream([iq[i:i + chunk] for i in range(0, F, chunk)], num_tx=num_tx))
        stream_s = time.perf_counter() - t0
        # the per-frame loop the reference's scripts run
        n_loop = min(a.loop_frames, F)
        pcg = PointCloudGenerator(cm, az_antenna_idxs=AZ, el_antenna_idxs=EL, detector_type="range_doppler_ground_detector",
                                  detector_params=params)
        for f in range(3):
            pcg.process(cubes[f])
        pcg.reset()
        t0 = time.perf_counter()
        for f in range(n_loop):
            pcg.process(cubes[f])
        loop_s = time.perf_counter() - t0
        report[name] = {
            "batch_frames_per_s": F / wall, "batch_ms": wall * 1e3, "points_per_batch": points // a.reps,
            "host_scan_ms": scan * 1e3, "host_scan_share": scan / wall, "flagged": int(p.n_flagged),
            "stream_i16_frames_per_s": F / stream_s, "stream_chunk": chunk,
            "loop_frames_per_s": n_loop / loop_s, "loop_frames": n_loop,
            "speedup_batch_vs_loop": (F / wall) / (n_loop / loop_s),
        }
        print(name, json.dumps(report[name]), flush=True)
        p.bufs.free()
        ps.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
