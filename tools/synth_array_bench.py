#!/usr/bin/env python3
"""Synthetic-array images of a resident batch (``FramePipeline.synthetic_array``) against what it replaces.

Per case (shape, ``num_frames`` H, ``stride``, 60 azimuth x 1 elevation bins, a steady velocity so that every frame from H - 1 on
is valid):

* ``synth_array``: the ``synth_array`` profile family (device time of one ``mmw_synth_array`` call, table upload included), the
  host clock of ``synthetic_array_device`` (adds the host geometry scan) and of ``synthetic_array`` (adds the download);
* ``bartlett_prestacked``: ``mmw_bartlett`` on the same windows stacked as ``[n, S, E]`` in HBM -- the ``bartlett`` family, the
  floor the in-place operand should meet -- and the host stacking + upload that the in-place path removes;
* ``per_frame_class_loop``: ``SyntheticArrayBeamformerProcessor.process`` on the first ``--loop-frames`` frames.

One warm-up call, ``--reps`` timed calls, median / min / max.  Also the worst deviation between the two device results.

    python tools/synth_array_bench.py [--frames 1250] [--reps 9] [--loop-frames 50] [--out profiles/synth_array_batch.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, synthetic_array_geometry  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors import SyntheticArrayBeamformerProcessor  # noqa: E402

CASES = [((12, 256, 128), 2, 1), ((12, 256, 128), 2, 2), ((12, 63, 100), 2, 1)]         # shape, H, stride
NUM_RX, NUM_TX = 4, 3


def stats(walls):
    w = np.array(walls) * 1e3
    return {"ms": float(np.median(w)), "ms_min": float(w.min()), "ms_max": float(w.max()), "reps": len(w)}


def timed(ctx, fn, reps):
    fn()
    walls = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    return stats(walls)


def family(ctx, fn, reps, name):
    fn()
    per_call = []
    for _ in range(reps):
        ctx.profile_reset()
        ctx.profile_enable(1)
        fn()
        ctx.sync()
        ms, n = ctx.profile_get(name)
        ctx.profile_enable(0)
        per_call.append(ms / max(n, 1) * 1e-3)
    return stats(per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "frames": F}
    for (V, S, C), H, stride in CASES:
        cm = ConfigManager()
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
        fp = FramePipeline(cm, F, (V, S, C))
        fp.synth(F, seed0=4000)
        proc = SyntheticArrayBeamformerProcessor(cm, receiver_idx=1, chirp_cfg_idx=2, num_frames=H, stride=stride,
                                                 az_angle_bins_rad=np.deg2rad(np.linspace(-30, 30, 60)), el_angle_bins_rad=np.array([0.0]))
        vel = np.tile([0.2, 0.01, 0.0], (F, 1))
        v, T = 2 * NUM_RX + 1, 60
        Cv = -(-C // stride)
        E = H * Cv
        rec = {"H": H, "stride": stride, "E": E, "T": T}
        rec["host_geometry_scan"] = stats([(lambda t0: (synthetic_array_geometry(proc, vel), time.perf_counter() - t0)[1])(time.perf_counter())
                                           for _ in range(3)])
        rec["synth_array_family"] = family(ctx, lambda: fp.synthetic_array_device(proc, vel), a.reps, "synth_array")
        rec["synthetic_array_device_host_clock"] = timed(ctx, lambda: fp.synthetic_array_device(proc, vel), a.reps)
        rec["synthetic_array_with_download_host_clock"] = timed(ctx, lambda: fp.synthetic_array(proc, vel), max(a.reps // 3, 2))
        frames, resp = fp.synthetic_array(proc, vel)
        rec["n_valid"] = int(len(frames))
        # the same windows stacked on the host and uploaded: what callers of mmw_bartlett had to do
        valid, P = synthetic_array_geometry(proc, vel)
        cubes = fp.cubes()[:, v][:, :, ::stride]                                 # [F, S, Cv]
        t0 = time.perf_counter()
        X = np.zeros((len(frames), S, E), dtype=np.complex64)
        for h in range(H):
            src = frames - H + 1 + h
            X[src >= 0, :, h * Cv:(h + 1) * Cv] = cubes[src[src >= 0]]
        t_stack = time.perf_counter() - t0
        d_X, d_P = ctx.alloc(X.nbytes), ctx.alloc(P.nbytes)
        dirs = np.ascontiguousarray(proc.d.reshape(3, -1))
        d_D, d_Y = ctx.alloc(dirs.nbytes), ctx.alloc(len(frames) * S * T * 8)
        rec["host_stack_ms"] = t_stack * 1e3
        rec["stacked_upload"] = timed(ctx, lambda: d_X.upload(X), 3)
        d_P.upload(P)
        d_D.upload(dirs)
        call = lambda: _lib.check(ctx.lib.mmw_bartlett(ctx.handle, d_X.ptr, d_P.ptr, d_D.ptr, d_Y.ptr, len(frames), S, E, T,  # noqa: E731
                                                        proc.lambda_m))
        rec["bartlett_prestacked_family"] = family(ctx, call, a.reps, "bartlett")
        ref = d_Y.download((len(frames), S, T), np.complex64)
        got = resp.reshape(len(frames), S, T)
        rec["worst_deviation_from_prestacked_over_peak"] = float(np.abs(got - ref).max() / np.abs(ref).max())
        for b in (d_X, d_P, d_D, d_Y):
            b.free()
        # the per-frame class loop on raw cubes
        n_loop = min(a.loop_frames, F)
        virt = fp.cubes(0, n_loop)
        raw = np.zeros((n_loop, NUM_RX, S, NUM_TX * C), dtype=np.complex64)
        for tx in range(NUM_TX):
            raw[:, :, :, tx::NUM_TX] = virt[:, NUM_RX * tx:NUM_RX * (tx + 1)]
        walls = []
        for rep in range(3):
            proc.reset()
            t0 = time.perf_counter()
            for f in range(n_loop):
                proc.process(raw[f], vel[f])
            if rep:
                walls.append(time.perf_counter() - t0)
        rec["per_frame_class_loop"] = dict(stats(walls), frames=n_loop)
        report[f"{V}x{S}x{C} H={H} stride={stride}"] = rec
        print(f"{V}x{S}x{C} H={H} stride={stride}", json.dumps(rec), flush=True)
        fp.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
