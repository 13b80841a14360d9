#!/usr/bin/env python3
"""TDM-MIMO Doppler phase compensation on a resident CA-CFAR batch of 12x256x128 frames:

* ``FramePipeline.point_clouds_device()`` with ``tdm_compensation`` off and on -- the whole call (host clock between two syncs)
  and the device time of its argmax stage (profile families ``argmax`` / ``argmax_tdm`` / ``argmax_tdm64``);
* ``mmw_angle_argmax_tdm`` alone against ``mmw_angle_argmax_exact`` over the same detection lists of the same batch, azimuth
  list 0..7 (two transmit slots) and elevation list 8..11 (one slot: the compensated entry hands over to the exact one);
* the share of detections re-evaluated in float64 by either entry.

The batch is ``FramePipeline.synth`` (the benchmark's scenes); CFAR, antenna lists and capacity are bench.py's.  One warm-up
call, ``--reps`` timed calls, median / min / max.

    python tools/tdm_argmax_probe.py [--frames 1250] [--reps 7] [--out profiles/tdm_argmax.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, tdm_phase_table  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.detectors import CaCFAR2D  # noqa: E402

SHAPE = (12, 256, 128)
AZ, EL = list(range(8)), [8, 9, 10, 11]
FAMILIES = ("argmax", "argmax_tdm", "argmax_tdm64", "argmax_refine")


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


def families(ctx, fn, reps):
    """Device ms per call of each argmax profile family."""
    ctx.profile_reset()
    ctx.profile_enable(1)
    for _ in range(reps):
        fn()
    ctx.sync()
    out = {}
    for name in FAMILIES:
        ms, n = ctx.profile_get(name)
        if n:
            out[name] = float(ms) / reps
    ctx.profile_enable(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    V, S, C = SHAPE
    ctx = _lib.default_context()
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    report = {"device": _lib.device_info(0)["name"], "frames": F, "shape": list(SHAPE), "az": AZ, "el": EL}
    pipes = {}
    for name, on in (("off", False), ("on", True)):
        p = FramePipeline(cm, F, SHAPE, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5), az_antenna_idxs=AZ, el_antenna_idxs=EL,
                          det_capacity=2048, ctx=ctx, tdm_compensation=on)
        p.synth(F, seed0=4_000_000)
        pipes[name] = p
        rec = {"point_clouds_device": timed(ctx, p.point_clouds_device, a.reps),
               "argmax_families_ms": families(ctx, p.point_clouds_device, a.reps)}
        p.point_clouds_device()
        n_det = int(np.clip(p.counts, 0, p.cap).sum())
        rec["detections"] = n_det
        rec["evaluations"] = 2 * n_det
        rec["n_refined"] = int(p.n_refined)
        rec["refined_share"] = p.n_refined / max(2 * n_det, 1)
        report[f"tdm_{name}"] = rec
        print(name, json.dumps(rec), flush=True)
    # the two entries alone over the detection lists the compensated pipeline has left on the device
    p = pipes["on"]
    p.point_clouds_device()
    n_det = int(np.clip(p.counts, 0, p.cap).sum())
    lib, h = ctx.lib, ctx.handle
    d_idx = p.bufs.get("probe_idx", F * p.cap * 4)
    entries = {}
    for label, ants, shift in (("az", AZ, 1), ("el", EL, 0)):
        arr, n_ant = _lib.int_array(ants)
        table = tdm_phase_table(ants, p.tdm_slots[0], p.tdm_slots[1], C)
        n_ref = _lib.C.c_int(0)
        common = (h, p.d_in.ptr, p.d_l1.ptr, p.d_rd.ptr, p.d_dets.ptr, p.d_cnt.ptr, d_idx.ptr, F, V, S, C, p.cap, arr, n_ant, p.A, shift)
        exact = lambda: _lib.check(lib.mmw_angle_argmax_exact(*common, _lib.C.byref(n_ref)))                       # noqa: E731
        tdm = lambda: _lib.check(lib.mmw_angle_argmax_tdm(*common, table.ctypes.data, _lib.C.byref(n_ref)))          # noqa: E731
        rec = {"detections": n_det}
        for name, fn in (("exact", exact), ("tdm", tdm)):
            rec[name] = dict(timed(ctx, fn, a.reps), families_ms=families(ctx, fn, a.reps))
            fn()
            rec[name]["n_refined"] = int(n_ref.value)
            rec[name]["refined_share"] = n_ref.value / max(n_det, 1)
        entries[label] = rec
        print(label, json.dumps(rec), flush=True)
    report["entries"] = entries
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
