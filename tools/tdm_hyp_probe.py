#!/usr/bin/env python3
"""TDM-MIMO velocity unwrapping on a resident CA-CFAR batch of 12x256x128 frames, the scenes and settings of
tools/tdm_argmax_probe.py:

* ``FramePipeline.point_clouds_device()`` with ``tdm_compensation=True`` alone and with ``tdm_velocity_unwrap=True`` on top -- the
  whole call (host clock between two syncs) and the device time of the argmax stage by profile family (``argmax_tdm_hyp``: the
  float32 pass over every hypothesis, ``argmax_tdm_hyp64``: its float64 stage, ``tdm_unwrap``: the velocity kernel, ``argmax`` /
  ``argmax_tdm`` / ``argmax_tdm64``: the entries the single-hypothesis lists are handed to);
* ``mmw_angle_argmax_tdm_hyp`` alone on the azimuth list against ``mmw_angle_argmax_tdm`` over the same detection lists;
* the share of evaluations re-evaluated in float64, and how often each hypothesis wins.

``--parent FILE``: the report tools/tdm_argmax_probe.py wrote when run from a checkout of the parent commit; its ``tdm_on`` call is
recorded beside this tree's numbers as the baseline.  One warm-up call, ``--reps`` timed calls, median / min / max.

    python tools/tdm_hyp_probe.py [--frames 1250] [--reps 7] [--parent parent.json] [--out profiles/tdm_hyp.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mmwave_radar_processing_amd import _lib, synth  # noqa: E402
from mmwave_radar_processing_amd.batch import FramePipeline, tdm_hypothesis_table, tdm_phase_table  # noqa: E402
from mmwave_radar_processing_amd.config_managers import ConfigManager  # noqa: E402
from mmwave_radar_processing_amd.detectors import CaCFAR2D  # noqa: E402
from tdm_argmax_probe import AZ, EL, SHAPE, timed  # noqa: E402

FAMILIES = ("argmax", "argmax_tdm", "argmax_tdm64", "argmax_refine", "argmax_tdm_hyp", "argmax_tdm_hyp64", "tdm_unwrap")


def families(ctx, fn, reps):
    """Device ms per call of each profile family of the argmax stage."""
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
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F = a.frames
    V, S, C = SHAPE
    ctx = _lib.default_context()
    cm = ConfigManager()
    cm.load_cfg_text(synth.SYNTH_CFG_256x128x12)
    report = {"device": _lib.device_info(0)["name"], "frames": F, "shape": list(SHAPE), "az": AZ, "el": EL}
    if a.parent:
        with open(a.parent) as fh:
            parent = json.load(fh)
        report["parent_tdm_compensation_alone"] = parent["tdm_on"]
    pipes = {}
    for name, unwrap in (("compensation_alone", False), ("unwrap", True)):
        p = FramePipeline(cm, F, SHAPE, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5), az_antenna_idxs=AZ, el_antenna_idxs=EL,
                          det_capacity=2048, ctx=ctx, tdm_compensation=True, tdm_velocity_unwrap=unwrap)
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
        if unwrap:
            live = np.arange(p.cap)[None, :] < np.clip(p.counts, 0, p.cap)[:, None]
            rec["hypothesis_wins"] = np.bincount(p.tdm_hypotheses()[live], minlength=p.tdm_slots[1]).tolist()
        report[name] = rec
        print(name, json.dumps(rec), flush=True)
    # the two entries alone over the azimuth list and the detection lists the pipeline has left on the device
    p = pipes["unwrap"]
    p.point_clouds_device()
    n_det = int(np.clip(p.counts, 0, p.cap).sum())
    lib, h = ctx.lib, ctx.handle
    d_idx = p.bufs.get("probe_idx", F * p.cap * 4)
    d_hyp = p.bufs.get("probe_hyp", F * p.cap * 4)
    arr, n_ant = _lib.int_array(AZ)
    slots, n_slots = p.tdm_slots
    table = tdm_phase_table(AZ, slots, n_slots, C)
    tables = tdm_hypothesis_table(AZ, slots, n_slots, C)
    n_ref = _lib.C.c_int(0)
    head = (h, p.d_in.ptr, p.d_l1.ptr, p.d_rd.ptr, p.d_dets.ptr, p.d_cnt.ptr, d_idx.ptr)
    shape = (F, V, S, C, p.cap, arr, n_ant, p.A, 1)
    calls = {
        "tdm": lambda: _lib.check(lib.mmw_angle_argmax_tdm(*head, *shape, table.ctypes.data, _lib.C.byref(n_ref))),
        "tdm_hyp": lambda: _lib.check(lib.mmw_angle_argmax_tdm_hyp(*head, d_hyp.ptr, 0, *shape, tables.ctypes.data, n_slots,
                                                                   _lib.C.byref(n_ref))),
        "tdm_hyp_given": lambda: _lib.check(lib.mmw_angle_argmax_tdm_hyp(*head, d_hyp.ptr, 1, *shape, tables.ctypes.data, n_slots,
                                                                         _lib.C.byref(n_ref))),
    }
    entries = {"detections": n_det}
    for name, fn in calls.items():
        rec = dict(timed(ctx, fn, a.reps), families_ms=families(ctx, fn, a.reps))
        fn()
        rec["n_refined"] = int(n_ref.value)
        rec["refined_share"] = n_ref.value / max(n_det, 1)
        entries[name] = rec
        print(name, json.dumps(rec), flush=True)
    report["entries_az"] = entries
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
