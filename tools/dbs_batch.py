#!/usr/bin/env python3
"""Doppler beam sharpening of a resident batch, timed three ways on synthetic 12x256x128 and 12x63x100 frames:

* (a) the per-frame ``RangeAngleProcessorDBSEnhanced.process`` loop on the first ``--loop-frames`` frames (host cubes);
* (b) ``FramePipeline.chain3d(magnitude=True)`` plus one ``mmw_dbs_gather`` per frame on the resident batch -- what the C ABI
  offered before ``mmw_dbs_sharpen`` (one index table per call) --, index tables made beforehand;
* (c) ``FramePipeline.dbs_range_angle_device`` (no download) and ``dbs_range_angle`` (with it), the host's share for the index
  tables, the device time of the two profile families (``rd``, ``dbs_sharpen``), and a sweep of ``MMW_DBS_CHUNK_MB``.

Every frame moves at its own velocity above ``min_vel_dbs``.  One warm-up call, ``--reps`` timed calls between two syncs, median
and extremes reported.  The images of (a), (b) and (c) are compared with each other on the loop's frames.

    python tools/dbs_batch.py [--frames 1250] [--reps 7] [--loop-frames 100] [--out profiles/dbs_batch.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, dbs_index_tables  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors import RangeAngleProcessorDBSEnhanced  # noqa: E402

SHAPES = [(12, 256, 128), (12, 63, 100)]
A = 64


def stats(walls, F):
    w = np.array(walls)
    return {"frames_per_s": F / float(np.median(w)), "ms": float(np.median(w)) * 1e3, "ms_min": float(w.min()) * 1e3,
            "ms_max": float(w.max()) * 1e3, "reps": len(w)}


def timed(ctx, fn, reps, F):
    fn()                                        # warm-up: code objects, tables, buffers
    walls = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        walls.append(time.perf_counter() - t0)
    return stats(walls, F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    ctx = _lib.default_context()
    lib, h = ctx.lib, ctx.handle
    report = {"device": _lib.device_info(0)["name"], "frames": F, "angle_bins": A, "n_out": A}
    for V, S, C in SHAPES:
        cm = ConfigManager()
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
        dbs = RangeAngleProcessorDBSEnhanced(cm, num_angle_bins_range_angle_response=A, num_angle_bins_dbs_enhanced_response=A)
        n_out = len(dbs.angle_bins_dbs_enhanced)
        rng = np.random.default_rng(1)
        phi, speed = rng.uniform(0, 2 * np.pi, F), rng.uniform(0.3, 0.8, F) * cm.vel_max_m_s
        v = np.stack([speed * np.cos(phi), speed * np.sin(phi), rng.normal(size=F)], axis=1)
        p = FramePipeline(cm, F, (V, S, C), num_angle_bins=A)
        p.synth(F, seed0=4000)
        rec = {"bytes_per_frame": {"cube": V * S * C * 8, "magnitude_cube": A * S * C * 4, "image": S * n_out * 4}}

        # (a) per-frame loop
        n_loop = min(a.loop_frames, F)
        host = p.cubes(0, n_loop)
        dbs.process(host[0], velocity_ned=v[0])
        t0 = time.perf_counter()
        loop = [dbs.process(host[f], velocity_ned=v[f]) for f in range(n_loop)]
        rec["a_per_frame_loop"] = {"frames_per_s": n_loop / (time.perf_counter() - t0), "frames": n_loop}

        # (b) chain3d(magnitude) + one gather per frame
        t0 = time.perf_counter()
        ang_tab, vel_tab = dbs_index_tables(dbs, v)
        rec["host_index_tables_ms"] = (time.perf_counter() - t0) * 1e3
        d_b = p.bufs.get("gather_out", F * S * n_out * 4)
        ip = _lib._ip

        def gather_all():
            p.chain3d(magnitude=True)
            for f in range(F):
                _lib.check(lib.mmw_dbs_gather(h, p.d_cube3d.at(f * A * S * C * 4), ang_tab[f].ctypes.data_as(ip),
                                              vel_tab[f].ctypes.data_as(ip), d_b.at(f * S * n_out * 4), 1, A, S, C, n_out))
        rec["b_chain3d_plus_gather"] = timed(ctx, gather_all, a.reps, F)
        rec["b_chain3d_alone"] = timed(ctx, lambda: p.chain3d(magnitude=True), a.reps, F)
        got_b = d_b.download((n_loop, S, n_out), np.float32)

        # (c) the batched method
        rec["c_device"] = timed(ctx, lambda: p.dbs_range_angle_device(dbs, v), a.reps, F)
        rec["c_with_download"] = timed(ctx, lambda: p.dbs_range_angle(dbs, v), a.reps, F)

        def abi_only():
            _lib.check(lib.mmw_dbs_sharpen(h, p.d_in.ptr, None, ang_tab.ctypes.data_as(ip), vel_tab.ctypes.data_as(ip), p.d_dbs.ptr,
                                           F, V, S, C, A, None, 0, n_out))
        rec["c_abi_call_tables_given"] = timed(ctx, abi_only, a.reps, F)
        ctx.profile_reset()
        ctx.profile_enable(1)
        for _ in range(a.reps):
            abi_only()
        ctx.sync()
        fam = {}
        for name in ("rd", "dbs_sharpen"):
            ms, n = ctx.profile_get(name)
            fam[name] = {"ms_per_call": float(ms) / a.reps, "launch_groups_per_call": int(n) // a.reps}
        ctx.profile_enable(0)
        rec["c_profile_families"] = fam
        sweep = {}
        for mb in (32, 64, 128, 256, 1024, 8192):
            ctx.set_option("MMW_DBS_CHUNK_MB", mb)
            sweep[str(mb)] = timed(ctx, abi_only, a.reps, F)
        ctx.set_option("MMW_DBS_CHUNK_MB", None)
        rec["c_chunk_mb_sweep"] = sweep
        got_c = p.d_dbs.download((n_loop, S, n_out), np.float32)
        peak = float(max(np.max(x) for x in loop))
        rec["max_abs_difference_over_loop_peak"] = {
            "b_vs_c": float(np.max(np.abs(got_b - got_c))) / peak,
            "loop_vs_c": float(max(np.max(np.abs(loop[f] - got_c[f])) for f in range(n_loop))) / peak}
        rec["c_over_b"] = rec["c_device"]["frames_per_s"] / rec["b_chain3d_plus_gather"]["frames_per_s"]
        rec["c_abi_over_b_chain3d_alone"] = rec["c_abi_call_tables_given"]["frames_per_s"] / rec["b_chain3d_alone"]["frames_per_s"]
        report[f"{V}x{S}x{C}"] = rec
        print(f"{V}x{S}x{C}", json.dumps(rec), flush=True)
        p.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
