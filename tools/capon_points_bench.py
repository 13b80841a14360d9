#!/usr/bin/env python3
"""Capon point clouds of a resident batch (``FramePipeline.capon_point_clouds_device``), measured stage by stage.

Workload: ``--frames`` (1250) frames of 12x256x128 from ``mmw_synth_cubes``, 8 azimuth antennas, all 256 range bins, 181 angles,
CA-CFAR (4, 4) / (2, 2) at pfa 1e-5 on the (range, angle) map.

(a) the whole call -- snapshots, Capon map, widening, CFAR mask, compaction, beamformed Doppler and points, counts downloaded --
    by the host clock between two syncs: one warm-up, then ``--reps`` (7) calls, median / min / max;
(b) the device time of every stage per call (the profile families ``range_snapshots``, ``capon``, ``cfar``, ``compact``,
    ``capon_doppler``; the widening has no family and is timed alone by the host clock) and which stage dominates;
(c) the detections per frame, so that the per-detection cost of ``mmw_capon_doppler`` can be read off;
(d) the NumPy restatement of the definition (tests/capon_points_cases.py: covariance, ``np.linalg.solve``, ``np.fft``) on the
    device's own snapshots and detections of ``--loop-frames`` (3) frames on the host.  It is measured on those frames only and
    SCALED to the batch (``scaled_to_batch_ms``): an extrapolation, not a measurement.  The Capon map and the CFAR of those
    frames are not part of it (they would add to the host's time).

No pass/fail threshold is applied here.

    python tools/capon_points_bench.py [--frames 1250] [--reps 7] [--loop-frames 3] [--out profiles/capon_points.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import capon_points_cases as cases  # noqa: E402
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.detectors import CaCFAR2D  # noqa: E402

THETAS = np.deg2rad(np.linspace(-90.0, 90.0, 181))
SHAPE, N_RX = (12, 256, 128), 8
FAMILIES = ("range_snapshots", "capon", "cfar", "compact", "capon_doppler")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-frames", type=int, default=3)
    ap.add_argument("--det-capacity", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capon_points.json"))
    a = ap.parse_args()
    ctx = _lib.default_context()
    V, S, C = SHAPE
    F, T, rx = a.frames, len(THETAS), list(range(N_RX))
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
    p = FramePipeline(cm, F, SHAPE, det_capacity=a.det_capacity)
    p.synth(F, seed0=4000)
    det = CaCFAR2D((4, 4), (2, 2), 1e-5)
    call = lambda: p.capon_point_clouds_device(THETAS, rx, det)      # noqa: E731
    call()                                                            # warm-up: code objects, tables, buffers
    walls = []
    for _ in range(a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    w = np.array(walls)
    counts = p.capon_counts.astype(np.int64)
    report = {"device": _lib.device_info(ctx.device), "workload": {"frames": F, "shape": list(SHAPE), "antennas": N_RX,
                                                                  "range_rows": S, "angles": T, "cfar": "CA (4,4)/(2,2) pfa 1e-5",
                                                                  "det_capacity": a.det_capacity},
              "a_whole_call": {"ms": float(np.median(w)) * 1e3, "ms_min": float(w.min()) * 1e3, "ms_max": float(w.max()) * 1e3,
                               "reps": a.reps, "frames_per_s": F / float(np.median(w))},
              "c_detections": {"total": int(counts.sum()), "per_frame_mean": float(counts.mean()), "per_frame_max": int(counts.max()),
                               "rows_with_detections_per_frame_mean": None}}
    # (b) stages
    ctx.profile_reset()
    ctx.profile_enable(1)
    for _ in range(a.reps):
        call()
    ctx.sync()
    stages = {}
    for name in FAMILIES:
        ms, n = ctx.profile_get(name)
        stages[name] = {"ms_per_call": float(ms) / a.reps, "launch_groups_per_call": n / a.reps}
    ctx.profile_enable(0)
    d64 = p.bufs.get("capon_map64", 0)
    n_widen = min(F * S * T, d64.nbytes // 8)
    widen = lambda: _lib.check(ctx.lib.mmw_widen_f32_f64(ctx.handle, p.d_capon.ptr, d64.ptr, n_widen))     # noqa: E731
    widen()
    ww = []
    for _ in range(a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        widen()
        ctx.sync()
        ww.append(time.perf_counter() - t0)
    stages["widen (host clock, alone)"] = {"ms_per_call": float(np.median(ww)) * 1e3 * (F * S * T / n_widen), "launch_groups_per_call": 1}
    report["b_stages"] = stages
    report["b_dominant_stage"] = max(stages, key=lambda k: stages[k]["ms_per_call"])
    if counts.sum():
        report["c_detections"]["capon_doppler_us_per_detection"] = stages["capon_doppler"]["ms_per_call"] * 1e3 / float(counts.sum())
    # (d) the restatement on the host, a few frames, scaled
    n_loop = min(a.loop_frames, F)
    dets = p.d_capon_dets.download((F, p.cap, 2), np.int32)[:n_loop]
    rx_arr, _ = _lib.int_array(rx)
    d_snap = ctx.alloc(n_loop * N_RX * S * C * 8)
    _lib.check(ctx.lib.mmw_range_snapshots(ctx.handle, p.d_in.ptr, d_snap.ptr, n_loop, V, S, C, rx_arr, N_RX, 0, S, 1))
    X = d_snap.download((n_loop, N_RX, S, C), np.complex64).copy()
    d_snap.free()
    dop_dev = p.d_capon_dop.download((F, p.cap), np.int32)[:n_loop]
    rows = [len(np.unique(dets[f, :counts[f], 0])) for f in range(n_loop)]
    report["c_detections"]["rows_with_detections_per_frame_mean"] = float(np.mean(rows)) + 0.0
    report["c_detections"]["rows_with_detections_measured_on_frames"] = n_loop
    t0 = time.perf_counter()
    agree = total = 0
    for f in range(n_loop):
        m = int(min(counts[f], p.cap))
        dop, _, _ = cases.doppler_reference(X[f], dets[f, :m], THETAS, 1e-3, True)
        agree += int(np.sum(dop == dop_dev[f, :m]))
        total += m
    host_s = time.perf_counter() - t0
    report["d_numpy_restatement_on_host"] = {
        "frames": n_loop, "ms": host_s * 1e3, "scaled_to_batch_ms": host_s * 1e3 * F / n_loop, "detections": total,
        "doppler_bins_equal_to_device": agree,
        "note": "measured on these frames only; scaled_to_batch_ms is that time times frames / loop frames, not a measurement; the "
                "host's Capon map and CFAR are not included"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
