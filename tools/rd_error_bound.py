#!/usr/bin/env python3
"""Measured share of the rounding-error budget of the float32 range-Doppler kernels on the adversarial planes of
tests/rd_bound_cases.py: for every kernel family of its CASES list, max_cell |rd32 - rd64| / (rd_error_ulps 2^-24 l1_dev) per
input kind, with the device l1's relative error against the float64 sum.  Writes one JSON document (default
profiles/rd_error_bound.json); tests/test_gpu_rd_error_bound.py asserts the same quantities stay <= 1."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rd_bound_cases as rb  # noqa: E402
from mmwave_radar_processing_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rd_error_bound.json"))
    args = ap.parse_args()
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    plan = (ctypes.c_int * 8)()
    cases, families = [], {}
    for c in rb.CASES:
        names, cube, rd64, l1_64 = rb.planes_and_reference(c.S, c.C)
        V = cube.shape[0]
        for name in rb.ENV_SWITCHES:
            os.environ.pop(name, None)
        os.environ.update(c.env)
        for name, value in c.options.items():
            ctx.set_option(name, value)
        d_in, d_rd, d_l1 = ctx.alloc(cube.nbytes), ctx.alloc(cube.nbytes), ctx.alloc(V * 4)
        try:
            _lib.check(L.mmw_diag_detect_plan(c.S, c.C, _lib.CFAR_CA, 4, 4, 2, 2, 0, 0, 64, plan))
            ulps = plan[7]
            d_in.upload(cube)
            _lib.check(L.mmw_range_doppler(h, d_in.ptr, d_rd.ptr, None, 1, V, c.S, c.C))
            _lib.check(L.mmw_plane_l1(h, d_in.ptr, d_l1.ptr, 1, V, c.S, c.C))
            rd32 = d_rd.download((V, c.S, c.C), np.complex64).copy()
            l1_dev = d_l1.download((V,), np.float32).astype(np.float64)
        finally:
            for b in (d_in, d_rd, d_l1):
                b.free()
            for name in c.options:
                ctx.set_option(name, None)
            for name in c.env:
                os.environ.pop(name, None)
        ratios, cells = rb.check(rd32, rd64, l1_dev, ulps)
        w = int(np.argmax(ratios))
        cases.append({"case": rb.case_id(c), "family": c.family, "shape": [c.S, c.C], "budget_ulps": ulps,
                      "worst_ratio": round(float(ratios[w]), 5), "worst_input": names[w], "worst_cell": list(cells[w]),
                      "worst_error_ulps_of_l1": round(float(ratios[w]) * ulps, 3),
                      "l1_rel_err_max": float(np.max(np.abs(l1_dev - l1_64) / l1_64)),
                      "ratio_by_input": {n: round(float(r), 5) for n, r in zip(names, ratios)}})
        fam = families.setdefault(c.family, {"worst_ratio": 0.0})
        if ratios[w] > fam["worst_ratio"]:
            fam.update(worst_ratio=round(float(ratios[w]), 5), case=rb.case_id(c), input=names[w], budget_ulps=ulps,
                       worst_error_ulps_of_l1=round(float(ratios[w]) * ulps, 3))
        print(f"{rb.case_id(c):28s} budget {ulps:4d}  worst {ratios[w]:.4f}  {names[w]} {cells[w]}")
    info = _lib.device_info(0)
    doc = {"what": "max_cell |rd32 - rd64| / (rd_error_ulps * 2^-24 * l1_dev) on the planes of tests/rd_bound_cases.py (F = 1, one "
                   "input kind per antenna plane); rd64 = oracle_np.range_doppler in complex128",
           "device": info.get("arch"), "families": families, "cases": cases}
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
