#!/usr/bin/env python3
"""Capon range-azimuth maps of a resident batch (``FramePipeline.capon_range_angle_device``), measured against their parts:

(a) the whole call: ``mmw_range_snapshots`` + ``mmw_capon`` per pass of frames, result left in HBM;
(b) ``mmw_capon`` alone on snapshots of the whole batch already resident -- the floor, the new call cannot beat it;
(c) the snapshot kernel's device time (profile family ``range_snapshots``) against its bytes, cube read plus snapshot write, as
    a fraction of the in-situ copy ceiling (``--membw FILE``: the JSON line ``tools/membw.py`` prints on the same card);
(d) today's route on ``--loop-frames`` frames: host cubes, a NumPy Hann + range FFT of the listed antennas, then
    ``CaponBeamformer.process`` (upload + ``mmw_capon`` + download).  It is measured on those frames only and SCALED to the batch
    (``scaled_to_batch_ms``): the figure for the whole batch is an extrapolation, not a measurement;
(e) (a) again with ``frames_per_pass`` set from snapshot budgets of 16, 64, 256 and 1024 MiB, and as a single pass.

Batches: ``--frames`` (1250) frames of 12x256x128 with 8 azimuth antennas, and the BASELINE shape 12x512x128 with 12 antennas at
``--baseline-frames`` (625: the same bytes of cubes); all range bins, 181 angles.  One warm-up call, then ``--reps`` (9) timed
calls by the host clock between two syncs: median / min / max.  The per-stage device times are per-call means of the profile
families over the same number of calls.  No pass/fail threshold is applied here.

    python tools/capon_range_angle_bench.py [--frames 1250] [--baseline-frames 625] [--reps 9] [--loop-frames 40]
                                            [--membw FILE] [--out profiles/capon_range_angle.json]
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
from mmwave_radar_processing_amd.batch import FramePipeline, capon_pass_frames  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.processors.steering_beamformers import CaponBeamformer  # noqa: E402

THETAS = np.deg2rad(np.linspace(-90.0, 90.0, 181))
BUDGETS_MIB = (16, 64, 256, 1024)


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


def families_ms(ctx, fn, reps, names=("range_snapshots", "capon")):
    """Device time per call of fn of each profile family (every launch group timed by an event pair)."""
    ctx.profile_reset()
    ctx.profile_enable(1)
    for _ in range(reps):
        fn()
    ctx.sync()
    out = {}
    for name in names:
        ms, n = ctx.profile_get(name)
        out[name] = {"ms_per_call": float(ms) / reps, "launch_groups_per_call": n / reps}
    ctx.profile_enable(0)
    return out


def run_case(ctx, report, shape, n_rx, F, a):
    V, S, C = shape
    T = len(THETAS)
    lib, h = ctx.lib, ctx.handle
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
    p = FramePipeline(cm, F, shape)
    p.synth(F, seed0=4000)
    rx = list(range(n_rx))
    snap_bytes = n_rx * S * C * 8
    rec = {"frames": F, "antennas": n_rx, "range_bins": S, "angles": T,
           "bytes_per_frame": {"cube_read": snap_bytes, "snapshots_written": snap_bytes, "snapshots_read_by_capon": snap_bytes,
                               "map_out": S * T * 4},
           "default_frames_per_pass": capon_pass_frames(n_rx, S, C)}

    # (a) the whole call, default pass size
    call = lambda fpp=None: p.capon_range_angle_device(THETAS, rx, frames_per_pass=fpp)      # noqa: E731
    rec["a_whole_call"] = timed(ctx, call, a.reps, F)
    rec["a_whole_call"]["stages"] = families_ms(ctx, call, a.reps)

    # (b) mmw_capon alone on the whole batch's snapshots, already resident
    d_snap_all = p.bufs.get("bench_snap_all", F * snap_bytes)
    d_map = p.bufs.get("bench_map", F * S * T * 4)
    rx_arr, _ = _lib.int_array(rx)
    _lib.check(lib.mmw_range_snapshots(h, p.d_in.ptr, d_snap_all.ptr, F, V, S, C, rx_arr, n_rx, 0, S, 1))
    th = THETAS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    capon_alone = lambda: _lib.check(lib.mmw_capon(h, d_snap_all.ptr, th, d_map.ptr, F, n_rx, S, C, T, 1e-3))    # noqa: E731
    rec["b_capon_alone_on_resident_snapshots"] = timed(ctx, capon_alone, a.reps, F)
    rec["b_capon_alone_on_resident_snapshots"]["stages"] = families_ms(ctx, capon_alone, a.reps, ("capon",))

    # (c) the snapshot kernel alone over the whole batch against its bytes
    snaps_alone = lambda: _lib.check(lib.mmw_range_snapshots(h, p.d_in.ptr, d_snap_all.ptr, F, V, S, C, rx_arr, n_rx, 0, S, 1))  # noqa: E731
    fam = families_ms(ctx, snaps_alone, a.reps, ("range_snapshots",))["range_snapshots"]["ms_per_call"]
    moved = 2 * F * snap_bytes
    rec["c_snapshot_kernel_alone"] = {"family_ms": fam, "bytes_moved": moved, "GBps": moved / fam / 1e6,
                                      "host_clock": timed(ctx, snaps_alone, a.reps, F)}
    in_call = rec["a_whole_call"]["stages"]["range_snapshots"]["ms_per_call"]
    rec["c_snapshot_kernel_in_the_call"] = {"family_ms": in_call, "GBps": moved / in_call / 1e6}
    if report.get("copy_ceiling_GBps"):
        rec["c_snapshot_kernel_alone"]["fraction_of_copy_ceiling"] = rec["c_snapshot_kernel_alone"]["GBps"] / report["copy_ceiling_GBps"]
        rec["c_snapshot_kernel_in_the_call"]["fraction_of_copy_ceiling"] = moved / in_call / 1e6 / report["copy_ceiling_GBps"]

    # (d) today's route on a few frames, scaled
    n_loop = min(a.loop_frames, F)
    host = p.cubes(0, n_loop)
    bf = CaponBeamformer(THETAS, delta=1e-3, ctx=ctx)
    win = np.hanning(S).astype(np.float32)[None, :, None]

    def todays_route():
        return [bf.process(np.fft.fft(host[f][rx] * win, axis=1)) for f in range(n_loop)]
    walls = []
    for rep in range(4):                                   # the first pass is the warm-up
        t0 = time.perf_counter()
        maps_host = todays_route()
        if rep:
            walls.append(time.perf_counter() - t0)
    d = stats(walls, n_loop)
    d.update(frames=n_loop, scaled_to_batch_ms=d["ms"] * F / n_loop,
             note="measured on these frames only; scaled_to_batch_ms is that time times frames / loop frames, not a measurement")
    rec["d_host_fft_then_process"] = d
    # the two routes give the same maps up to the float32 FFTs in front of them (figures only)
    dev = p.capon_range_angle(THETAS, rx)[:n_loop]
    rec["d_host_fft_then_process"]["median_rel_diff_to_device_route"] = float(np.median(np.abs(dev - np.stack(maps_host)) / dev))

    # (e) pass-size sweep
    sweep = {}
    for mib in BUDGETS_MIB:
        fpp = min(F, capon_pass_frames(n_rx, S, C, mib << 20))
        sweep[f"{mib}MiB"] = dict(timed(ctx, lambda: call(fpp), a.reps, F), frames_per_pass=fpp)
    sweep["single_pass"] = dict(timed(ctx, lambda: call(F), a.reps, F), frames_per_pass=F)
    rec["e_frames_per_pass_sweep"] = sweep
    report[f"{V}x{S}x{C}_rx{n_rx}"] = rec
    print(f"{V}x{S}x{C}_rx{n_rx}", json.dumps(rec), flush=True)
    bf._bufs.free()
    p.bufs.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--baseline-frames", type=int, default=625)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=40)
    ap.add_argument("--membw", default=None, help="JSON line printed by tools/membw.py on the same card")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "timing": f"median of {a.reps} calls, host clock between two syncs"}
    if a.membw:
        with open(a.membw) as fh:
            table = json.loads([ln for ln in fh.read().splitlines() if ln.startswith("{")][-1])
        report["membw_copy_GBps"] = {k: v for k, v in table.items() if k.startswith("copy_")}
        report["copy_ceiling_GBps"] = float(max(report["membw_copy_GBps"].values()))
    run_case(ctx, report, (12, 256, 128), 8, a.frames, a)
    run_case(ctx, report, (12, 512, 128), 12, a.baseline_frames, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
