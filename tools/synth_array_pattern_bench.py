#!/usr/bin/env python3
"""Synthetic-array beam patterns of a whole drive (``batch.array_patterns`` on ``mmw_synth_array_pattern``) against the reference's
host loop.  Two shapes: 1250 frames x E = 256 elements x 60 directions (the configuration of ``tools/synth_array_bench.py``), and
1250 x E = 640 x 60 azimuth x 16 elevation bins.  Per shape:

* ``synth_pattern``: device time of one ``mmw_synth_array_pattern`` call on a geometry table already in HBM (profile family
  ``synth_pattern``: the copy of the directions, the magnitude kernel and the normalisation) and the sine/cosine pairs per second
  that is (n E T pairs per call);
* ``call_host_clock``: ``batch.array_patterns`` end to end (upload of the table, the call, download of the patterns);
* ``numpy_loop``: the reference's double loop over azimuth x elevation (one ``exp`` over all elements per direction, in numpy on
  the host) on the first ``--loop-frames`` frames, scaled to all frames.

    python tools/synth_array_pattern_bench.py [--frames 1250] [--reps 9] [--loop-frames 20] [--out profiles/synth_array_pattern.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmwave_radar_processing_amd import _lib  # noqa: E402
from mmwave_radar_processing_amd.batch import array_patterns, array_patterns_on  # noqa: E402
from mmwave_radar_processing_amd.processors.steering_beamformers import SyntheticArrayBeamformerCore  # noqa: E402
from synth_array_bench import family, stats, timed  # noqa: E402

LAMBDA = 299792458.0 / 60.25e9
SHAPES = {"1250x256x60": (256, 60, 1), "1250x640x960": (640, 60, 16)}


def numpy_loop(core, P):
    """The reference's compute_synthetic_array_pattern, frame by frame."""
    n_az, n_el = core.d.shape[1:]
    out = np.zeros((len(P), n_az, n_el), dtype=np.float32)
    for i, geo in enumerate(P):
        for a in range(n_az):
            for e in range(n_el):
                out[i, a, e] = np.abs(core.compute_array_factor_at_angle(geo, core.d[:, a, e]))
        out[i] /= np.max(out[i])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    ctx = _lib.default_context()
    report = {"device": _lib.device_info(0)["name"], "frames": n}
    rng = np.random.default_rng(5)
    for name, (E, n_az, n_el) in SHAPES.items():
        core = SyntheticArrayBeamformerCore(np.deg2rad(np.linspace(-30, 30, n_az)), np.deg2rad(np.linspace(0, 15, n_el)), LAMBDA, ctx=ctx)
        # a track of elements 0.4 wavelengths apart, every frame with its own speed and a jitter of a twentieth of a wavelength
        P = np.zeros((n, 3, E))
        P[:, 0] = (np.arange(E) - (E - 1.0))[None, :] * 0.4 * LAMBDA * rng.uniform(0.9, 1.1, (n, 1))
        P += 0.05 * LAMBDA * rng.standard_normal(P.shape)
        T = n_az * n_el
        d_P, d_pat = ctx.alloc(P.nbytes), ctx.alloc(n * T * 4)
        d_P.upload(P)
        rec = {"E": E, "T": T}
        rec["synth_pattern"] = family(ctx, lambda: array_patterns_on(ctx, d_P.ptr, n, E, core.d, LAMBDA, d_pat), a.reps, "synth_pattern")
        rec["sincos_pairs_per_s"] = n * E * T / (rec["synth_pattern"]["ms"] * 1e-3)
        rec["call_host_clock"] = timed(ctx, lambda: array_patterns(P, core.d, LAMBDA, ctx=ctx), max(a.reps // 3, 2))
        n_loop = min(a.loop_frames, n)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            want = numpy_loop(core, P[:n_loop])
            walls.append(time.perf_counter() - t0)
        rec["numpy_loop"] = dict(stats(walls), frames=n_loop, ms_scaled_to_all_frames=float(np.median(walls)) * 1e3 * n / n_loop)
        got = d_pat.download((n, n_az, n_el), np.float32)[:n_loop]
        rec["worst_abs_difference_to_numpy_loop"] = float(np.abs(got - want).max())
        for b in (d_P, d_pat):
            b.free()
        report[name] = rec
        print(name, json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
