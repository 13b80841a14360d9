#!/usr/bin/env python3
"""Micro-Doppler rows of a resident batch, three ways, on 12x256x128 and the shipped 12x63x100 shape:

* ``FramePipeline.micro_doppler_device()`` -- device time (host clock between two syncs, and the ``micro_doppler`` profile family);
* ``FramePipeline.micro_doppler()`` -- with the download;
* the per-frame ``MicroDopplerProcessor.process`` loop on the first ``--loop-frames`` frames (host cubes), as the comparison.

The window is rows 0 .. 24 of 256 (the viewer's 1 m at 4 cm per bin) and 0 .. 16 of 63 (1 m under the shipped cfg).  Also
recorded: the same call with 4, 8 and 16 window rows per pass (``MMW_MD_KT``) and with the full span; the time of the existing
FULL-PLANE kernels on the same batch -- ``mmw_range_doppler`` (windowed float32, all V antennas: there is no un-windowed or
single-antenna float32 full-plane kernel) and ``mmw_range_doppler_mag64`` (one antenna, float64) -- as the yardstick for
"partial DFT against a full transform"; the HBM read ceiling and the fraction of it that S * C * 8 bytes per frame reach; the
worst error against NumPy over the loop frames.

The read ceiling is the best ``read_b*`` figure of ``tools/membw.py`` (``--membw FILE``: the JSON line that tool prints, from a run
on the same card); the tool also repeats that measurement itself on a 2 GiB buffer and records both, so that they can be compared.

One warm-up call, ``--reps`` timed calls, median / min / max; the per-frame loop is one warm-up pass and ``--loop-reps`` timed
passes over its frames, reported the same way.

    python tools/micro_doppler_bench.py [--frames 1250] [--reps 9] [--loop-frames 100] [--loop-reps 5] [--membw FILE]
                                        [--out profiles/micro_doppler.json]
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
from mmwave_radar_processing_amd.processors import MicroDopplerProcessor  # noqa: E402

CASES = [((12, 256, 128), 24), ((12, 63, 100), 16)]         # shape, row_hi of the window (row_lo = 0)


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


def family_ms(ctx, fn, reps, name="micro_doppler"):
    ctx.profile_reset()
    ctx.profile_enable(1)
    for _ in range(reps):
        fn()
    ctx.sync()
    ms, n = ctx.profile_get(name)
    ctx.profile_enable(0)
    return float(ms) / max(n, 1)


def read_ceiling(ctx):
    """GB/s of the streaming-read kernel of tools/membw.py (mode 2), best launch shape, on a 2 GiB buffer."""
    n = 2 << 30
    buf = ctx.alloc(n)
    best = 0.0
    for bpc in (8, 16, 32, 64):
        fn = lambda: _lib.check(ctx.lib.mmw_diag_membw(ctx.handle, buf.ptr, buf.ptr, n, 2, 256 * bpc))      # noqa: E731
        fn()
        ctx.sync()
        ctx.timer_start()
        for _ in range(5):
            fn()
        best = max(best, n / (ctx.timer_stop() / 5) / 1e6)
    buf.free()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=100)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--membw", default=None, help="JSON line printed by tools/membw.py on the same card")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    ctx = _lib.default_context()
    lib, h = ctx.lib, ctx.handle
    report = {"device": _lib.device_info(0)["name"], "frames": F, "read_ceiling_in_tool_GBps": read_ceiling(ctx)}
    report["read_ceiling_GBps"] = report["read_ceiling_in_tool_GBps"]
    if a.membw:
        with open(a.membw) as fh:
            table = json.loads([ln for ln in fh.read().splitlines() if ln.startswith("{")][-1])
        report["membw_read_GBps"] = {k: v for k, v in table.items() if k.startswith("read_")}
        report["read_ceiling_GBps"] = float(max(report["membw_read_GBps"].values()))
    for (V, S, C), hi in CASES:
        cm = ConfigManager()
        cm.load_cfg_text(synth.synth_cfg_text(num_samples=S, num_loops=C))
        p = FramePipeline(cm, F, (V, S, C))
        p.synth(F, seed0=4000)
        tr = (0.0, float(p.range_bins[hi]))
        proc = MicroDopplerProcessor(cm, target_ranges=list(tr))
        assert proc.rows == (0, hi), proc.rows
        K = hi + 1
        rec = {"window_rows": [0, hi], "bytes_per_frame": {"slab_in": S * C * 8, "row_out": C * 4},
               "flop_per_frame": 8 * (K * S * C + K * C * C)}

        n_loop = min(a.loop_frames, F)
        host = p.cubes(0, n_loop)
        walls = []
        for rep in range(a.loop_reps + 1):                  # the first pass is the warm-up
            t0 = time.perf_counter()
            loop = [proc.process(host[f])[:, 0].copy() for f in range(n_loop)]
            if rep:
                walls.append(time.perf_counter() - t0)
        rec["per_frame_processor_loop"] = dict(stats(walls, n_loop), frames=n_loop)

        rec["device"] = timed(ctx, lambda: p.micro_doppler_device(tr), a.reps, F)
        rec["with_download"] = timed(ctx, lambda: p.micro_doppler(tr), a.reps, F)
        rec["device_family_ms"] = family_ms(ctx, lambda: p.micro_doppler_device(tr), a.reps)
        bytes_in = F * S * C * 8
        rec["read_GBps"] = bytes_in / rec["device_family_ms"] / 1e6
        rec["fraction_of_read_ceiling"] = rec["read_GBps"] / report["read_ceiling_GBps"]
        rec["TFLOPs"] = F * rec["flop_per_frame"] / rec["device_family_ms"] / 1e9
        rows = p.micro_doppler(tr)
        worst = 0.0
        for f in range(n_loop):
            plane = np.abs(np.fft.fftshift(np.fft.fft2(host[f][0]), axes=1))
            worst = max(worst, float(np.max(np.abs(rows[f] - plane[:K].max(0)))) / float(plane.max()))
            assert np.array_equal(rows[f], loop[f])
        rec["worst_err_over_plane_peak"] = worst

        sweep = {}
        for kt in (4, 8, 16):
            ctx.set_option("MMW_MD_KT", kt)
            sweep[str(kt)] = family_ms(ctx, lambda: p.micro_doppler_device(tr), a.reps)
        ctx.set_option("MMW_MD_KT", None)
        rec["rows_per_pass_family_ms"] = sweep
        full = (0.0, float(p.range_bins[-1]))
        rec["full_span_family_ms"] = family_ms(ctx, lambda: p.micro_doppler_device(full), 3)

        d_rd = p.bufs.get("bench_rd", F * V * S * C * 8)
        d_m64 = p.bufs.get("bench_mag64", F * S * C * 8)
        rd_all = family_ms(ctx, lambda: _lib.check(lib.mmw_range_doppler(h, p.d_in.ptr, d_rd.ptr, None, F, V, S, C)), a.reps, "rd")
        t64 = timed(ctx, lambda: _lib.check(lib.mmw_range_doppler_mag64(h, p.d_in.ptr, d_m64.ptr, F, V, S, C, 0)), a.reps, F)
        rec["full_plane_kernels"] = {"range_doppler_f32_windowed_all_antennas_ms": rd_all,
                                     "the_same_per_antenna_ms": rd_all / V, "range_doppler_mag64_one_antenna_ms": t64["ms"]}
        report[f"{V}x{S}x{C}"] = rec
        print(f"{V}x{S}x{C}", json.dumps(rec), flush=True)
        p.bufs.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
