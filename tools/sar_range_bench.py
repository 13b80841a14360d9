#!/usr/bin/env python3
"""Strip-map SAR slices and range detections of a resident batch of 12x256x128 frames, against their natural yardsticks:

* ``FramePipeline.strip_map_sar_device()`` with the default window and a platform speed per frame -- host clock between two syncs,
  and the device time of the ``sar_slices`` profile family; ``strip_map_sar()`` with the download and the split into blocks;
* ``mmw_micro_doppler`` over the same range rows: the same fast-time stage and ALL C columns of the slow-time one, so its time is
  the ceiling the SAR kernel should stay under;
* the per-frame ``StripMapSARProcessor.process`` loop on the first ``--loop-frames`` frames (host cubes);
* ``FramePipeline.range_detections()`` (OS-CFAR) against the per-frame ``RangeDetector.process`` loop, with the ``range_detect``
  family's device time.

Also recorded: bytes of the antenna's slab per frame, the rate at which the SAR kernel reads them and its share of the HBM read
ceiling (``--membw FILE``: the JSON line of ``tools/membw.py`` from the same card; without it the share is left out), and the
worst error of the loop frames against NumPy.  One warm-up call, ``--reps`` timed calls, median / min / max.

    python tools/sar_range_bench.py [--frames 1250] [--reps 9] [--loop-frames 50] [--membw FILE] [--out profiles/sar_range.json]
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
from mmwave_radar_processing_amd.processors import RangeDetector, StripMapSARProcessor  # noqa: E402

SHAPE = (12, 256, 128)


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


def family_ms(ctx, fn, reps, name):
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    ctx.sync()
    ms, n = ctx.profile_get(name)
    ctx.profile_enable(False)
    return ms / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=50)
    ap.add_argument("--membw", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V, S, C = SHAPE
    F = a.frames
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    ctx = _lib.default_context()
    fp = FramePipeline(cm, max_frames=F, shape=SHAPE)
    fp.synth(F, seed0=7)
    proc = StripMapSARProcessor(cm)
    rng = np.random.default_rng(5)
    vel = rng.uniform(0.5, 4.0, size=F) * rng.choice([-1.0, 1.0], size=F)
    res = {"device": _lib.device_info(ctx.device), "shape": list(SHAPE), "frames": F}

    _, off, win = fp.strip_map_sar_device(proc, vel)
    r_lo, r_hi = int(win[0, 0]), int(win[0, 1])
    cols = win[:, 3] - win[:, 2]
    res["sar"] = {"rows": [r_lo, r_hi], "columns_min_median_max": [int(cols.min()), float(np.median(cols)), int(cols.max())],
                  "output_elements": int(off[-1]),
                  "call": timed(ctx, lambda: fp.strip_map_sar_device(proc, vel), a.reps, F),
                  "with_download": timed(ctx, lambda: fp.strip_map_sar(proc, vel), a.reps, F),
                  "kernel_ms": family_ms(ctx, lambda: fp.strip_map_sar_device(proc, vel), a.reps, "sar_slices")}
    md_range = (proc.range_bins[r_lo], proc.range_bins[r_hi - 1])
    lo_hi = (r_lo, r_hi - 1)

    def micro():
        d = fp.bufs.get("md_ceiling", F * C * 4)
        _lib.check(ctx.lib.mmw_micro_doppler(ctx.handle, fp.d_in.ptr, d.ptr, F, V, S, C, 0, *lo_hi))
    res["micro_doppler_same_rows"] = {"rows": list(lo_hi), "range_m": [float(x) for x in md_range], "call": timed(ctx, micro, a.reps, F),
                                      "kernel_ms": family_ms(ctx, micro, a.reps, "micro_doppler")}
    slab = S * C * 8
    k_s = res["sar"]["kernel_ms"] * 1e-3
    res["sar"]["slab_bytes_per_frame"] = slab
    res["sar"]["slab_read_GBps"] = F * slab / k_s / 1e9 if k_s > 0 else None
    res["sar"]["flops_per_frame_stage1"] = 8 * (r_hi - r_lo) * S * C
    res["sar"]["tflops"] = F * 8.0 * (r_hi - r_lo) * S * C / k_s / 1e12 if k_s > 0 else None
    if a.membw:
        with open(a.membw) as fh:
            mb = json.loads(fh.read().strip().splitlines()[-1])
        ceiling = max(v for k, v in mb.items() if k.startswith("read_b") and isinstance(v, (int, float)))
        res["sar"]["read_ceiling_GBps"] = ceiling
        res["sar"]["share_of_read_ceiling"] = res["sar"]["slab_read_GBps"] / ceiling

    n = min(a.loop_frames, F)
    cubes = fp.cubes(0, n)
    batch, _ = fp.strip_map_sar(proc, vel)
    cm_loop = ConfigManager()                     # a configuration of the per-frame loops' own: the resident cubes are
    cm_loop.load_cfg_text(synth.SYNTH_CFG_256x128x12)   # virtual-array cubes already, so their classes must not reformat
    cm_loop.virtual_antennas_enabled = False
    loop_proc = StripMapSARProcessor(cm_loop)

    def loop():
        return [loop_proc.process(cubes[f], vel[f]) for f in range(n)]
    worst = 0.0
    for f, blk in enumerate(loop()):
        assert np.array_equal(blk, batch[f])
        want = np.fft.fftshift(np.fft.fft2(cubes[f, 0].astype(np.complex128)), axes=1)
        w = win[f]
        if blk.size:
            worst = max(worst, float(np.abs(blk - want[w[0]:w[1], w[2]:w[3]]).max() / np.abs(want).max()))
    res["sar"]["per_frame_loop"] = timed(ctx, loop, 3, n)
    res["sar"]["worst_error_of_peak"] = worst

    det = RangeDetector(cm, "os_cfar_1d", dict(num_train=8, num_guard=2, rho=0.75, alpha=3.0))
    dets = fp.range_detections(det)
    loop_det = RangeDetector(cm_loop, "os_cfar_1d", dict(num_train=8, num_guard=2, rho=0.75, alpha=3.0))

    def rloop():
        return [loop_det.process(cubes[f]) for f in range(n)]
    for f, d in enumerate(rloop()):
        assert np.array_equal(d, dets[f])
    res["range"] = {"call": timed(ctx, lambda: fp.range_detections(det), a.reps, F),
                    "kernel_ms": family_ms(ctx, lambda: fp.range_detections(det), a.reps, "range_detect"),
                    "per_frame_loop": timed(ctx, rloop, 3, n), "mean_detections": float(np.mean([len(d) for d in dets]))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
