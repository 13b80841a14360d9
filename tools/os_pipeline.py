#!/usr/bin/env python3
"""OS-CFAR point-cloud pipeline on resident cubes -- mmw_detect_batch (float64 CFAR plane, GUI parameters (5,5)/(3,2), rho 0.7,
alpha 2: ~470 mostly noise-level detections per 256 x 128 frame) + mmw_angle_argmax_exact for both antenna lists -- in
us/frame (HIP events): with the worst-case argmax bound through the dense float64 refinement (mmw_cells64.h), with the
worst-case bound through the direct sums only, and with round 3's empirical eighth of the bound.

    python tools/os_pipeline.py [--frames 256] [--reps 5]

With --shape V,S,C for a plane without 128 chirps (V >= 12) the variants are the worst-case bound with MMW_ARGMAX_DENSE_MIXED = 1
(k_cells64_mixed<C> where the plan has it) and = 0 (the direct sums), timed --repeats times each in alternation in one
process; per variant the median, minimum and maximum of the whole pipeline and of the argmax stage in us/frame:

    python tools/os_pipeline.py --shape 12,63,100 --frames 1250 --repeats 5

MMWGPU_LIB=<another build's libmmwgpu.so> runs the same measurement on that build (profiles/os_pipeline_np2.json: the parent
commit's library, processes alternated on one device).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib  # noqa: E402

V, S, C, A = 12, 256, 128, 64


def main():
    global V, S, C
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-default", action="store_true", help="the default variant only (for a kernel trace)")
    ap.add_argument("--shape", default="12,256,128", help="V,S,C of the cubes (V >= 12: antennas 0 .. 7 and 8 .. 11 are used)")
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats per variant (planes without 128 chirps)")
    args = ap.parse_args()
    V, S, C = (int(x) for x in args.shape.split(","))
    if V < 12:
        ap.error("--shape: V >= 12")
    F, cap = args.frames, 2048
    ctx = _lib.Context(0)
    L = ctx.lib
    n = S * C
    d_in, d_rd = ctx.alloc(F * V * n * 8), ctx.alloc(F * V * n * 8)
    _lib.check(L.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 880000, 8, 30.0))
    d_mag, d_mask, d_l1 = ctx.alloc(F * n * 8), ctx.alloc(F * n), ctx.alloc(F * V * 4)
    d_dets, d_cnt = ctx.alloc(F * cap * 8), ctx.alloc(F * 4)
    d_az, d_el = ctx.alloc(F * cap * 4), ctx.alloc(F * cap * 4)
    az, n_az = _lib.int_array(range(8))
    el, n_el = _lib.int_array(range(8, 12))
    k_rank = max(1, min(int(0.7 * 220), 220))
    refined = [_lib.C.c_int(0), _lib.C.c_int(0)]

    def run(count=False):
        _lib.check(L.mmw_detect_batch(ctx.handle, d_in.ptr, d_rd.ptr, d_mag.ptr, d_mask.ptr, d_dets.ptr, d_cnt.ptr, d_l1.ptr, F, V, S, C,
                                      1, 5, 5, 3, 2, 2.0, k_rank, cap))
        for i, (ant, na, d_idx, shift) in enumerate(((az, n_az, d_az, 1), (el, n_el, d_el, 0))):
            _lib.check(L.mmw_angle_argmax_exact(ctx.handle, d_in.ptr, d_l1.ptr, d_rd.ptr, d_dets.ptr, d_cnt.ptr, d_idx.ptr, F, V, S, C,
                                                cap, ant, na, A, shift, _lib.C.byref(refined[i]) if count else None))

    if C != 128:
        print(json.dumps(np2(args, ctx, run, refined, d_az, d_el, d_cnt, F, cap)))
        return
    out = {"frames": F}
    ref = None
    for tag, opts in (("worst_case_bound_dense", {}),
                      ("worst_case_bound_direct_sums", {"MMW_ARGMAX_DENSE_MIN": 1 << 30}),
                      ("eighth_of_the_bound_direct_sums", {"MMW_ARGMAX_DENSE_MIN": 1 << 30, "MMW_ARGMAX_BOUND_DIV": 8}))[:1 if args.only_default else 3]:
        for k in ("MMW_ARGMAX_DENSE_MIN", "MMW_ARGMAX_BOUND_DIV"):
            ctx.set_option(k, opts.get(k))
        run(count=True)
        ctx.sync()
        ctx.profile_reset()
        ctx.profile_enable(1)
        run()
        ctx.sync()
        stages = {}
        for fam in ("rd", "rd64", "cfar", "compact", "plane_l1", "argmax"):
            t, k = ctx.profile_get(fam)
            if k:
                stages[fam + "_us_per_frame"] = round(1e3 * t / F, 2)
        ctx.profile_enable(False)
        ctx.timer_start()
        for _ in range(args.reps):
            run()
        ms = ctx.timer_stop() / args.reps
        idx = (d_az.download((F, cap), np.int32), d_el.download((F, cap), np.int32))
        cnt = d_cnt.download((F,), np.int32)
        if ref is None:
            ref = idx
        same = all(np.array_equal(x[f, :cnt[f]], y[f, :cnt[f]]) for x, y in zip(idx, ref) for f in range(F))
        out[tag] = {"us_per_frame": round(1e3 * ms / F, 2), "evaluations_refined": [refined[0].value, refined[1].value],
                    "detections": int(cnt.sum()), "indices_equal_to_first_variant": bool(same), "stages": stages}
    print(json.dumps(out))


def np2(args, ctx, run, refined, d_az, d_el, d_cnt, F, cap):
    """Planes without 128 chirps: MMW_ARGMAX_DENSE_MIXED 1 against 0 under the worst-case bound, repeats alternated."""
    plan = (_lib.C.c_int * 8)()
    has_plan = hasattr(ctx.lib, "mmw_diag_cells64_plan") and ctx.lib.mmw_diag_cells64_plan(S, C, plan) == _lib.MMW_OK
    variants = (("dense_mixed_1", 1), ("dense_mixed_0", 0))
    out = {"frames": F, "shape": [V, S, C], "library": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
           "cells64_plan": list(plan) if has_plan else None, "repeats": args.repeats, "runs_per_repeat": args.reps}
    ctx.set_option("MMW_ARGMAX_BOUND_DIV", 1)
    times = {tag: {"pipeline": [], "argmax": []} for tag, _ in variants}
    ref = None
    for tag, value in variants:                   # warm-up, refined counts, indices
        ctx.set_option("MMW_ARGMAX_DENSE_MIXED", value)
        run(count=True)
        ctx.sync()
        idx = (d_az.download((F, cap), np.int32), d_el.download((F, cap), np.int32))
        cnt = d_cnt.download((F,), np.int32)
        if ref is None:
            ref = idx
        same = all(np.array_equal(x[f, :cnt[f]], y[f, :cnt[f]]) for x, y in zip(idx, ref) for f in range(F))
        out[tag] = {"evaluations_refined": [refined[0].value, refined[1].value], "detections": int(cnt.sum()),
                    "indices_equal_to_first_variant": bool(same)}
    for _ in range(args.repeats):
        for tag, value in variants:
            ctx.set_option("MMW_ARGMAX_DENSE_MIXED", value)
            ctx.profile_reset()
            ctx.profile_enable(1)
            run()
            ctx.sync()
            t, k = ctx.profile_get("argmax")
            ctx.profile_enable(False)
            times[tag]["argmax"].append(1e3 * t / F)
            ctx.timer_start()
            for _ in range(args.reps):
                run()
            times[tag]["pipeline"].append(1e3 * ctx.timer_stop() / args.reps / F)
    for tag, _ in variants:
        for what, v in times[tag].items():
            out[tag][what + "_us_per_frame"] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    return out


if __name__ == "__main__":
    main()
