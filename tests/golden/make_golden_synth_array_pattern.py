#!/usr/bin/env python3
"""Generate ``synth_array_pattern.npz`` from the IMPORTED reference ``SyntheticArrayBeamformerProcessor``: its
``compute_synthetic_array_pattern`` (float32, normalised) and, per direction, the complex sum of its
``compute_array_factor_at_angle`` (build container only: the reference never has to exist where the tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth_array_pattern.py

As in ``make_golden_synth_array.py`` the Cartesian ``griddata`` step is replaced ON THE INSTANCE with a no-op (the pattern functions
do not call it; the replacement keeps the instance from ever raising there).  Nothing else of the reference is touched.

Three sets, each stored as geometry ``[n, H, 3, Cv]`` (the reference's ``array_geometry`` layout), azimuth and elevation bins, the
steering directions ``d [3, n_az, n_el]``, ``pattern [n, n_az, n_el]`` float32 and ``af [n, n_az, n_el]`` complex128:

  a  all eight geometries of ``synth_array.npz`` (gate open or shut), E = 3 x 34 = 102, 7 azimuth x 2 elevation bins
  b  three geometries of E = 5 x 13 = 65 elements along a jittered track, 257 azimuth bins x 1 elevation
  c  one geometry with positions of +-5 m (about 1300 wavelengths), E = 3 x 11 = 33, 5 azimuth x 3 elevation bins
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.config_managers.cfgManager import ConfigManager                                      # noqa: E402
from mmwave_radar_processing.processors.simple_synthetic_array_beamformer_processor_multiFrame import (            # noqa: E402
    SyntheticArrayBeamformerProcessor)

CFG = "6843_RadVel_ods_10Hz.cfg"


def processor(cm, az_rad, el_rad):
    p = SyntheticArrayBeamformerProcessor(cm, receiver_idx=1, chirp_cfg_idx=2, num_frames=3, stride=3, az_angle_bins_rad=az_rad,
                                          el_angle_bins_rad=el_rad)
    p.get_interpolated_response_cart = lambda *a, **k: None
    return p


def patterns(p, geometries):
    """The reference's pattern and its un-normalised array factor for every geometry ``[H, 3, Cv]``."""
    n_az, n_el = p.d.shape[1:]
    pat = np.zeros((len(geometries), n_az, n_el), dtype=np.float32)
    af = np.zeros((len(geometries), n_az, n_el), dtype=np.complex128)
    for i, g in enumerate(geometries):
        out = p.compute_synthetic_array_pattern(g)
        assert out.dtype == np.float32 and out.shape == (n_az, n_el)
        pat[i] = out
        flat = g.transpose((1, 0, 2)).reshape(3, -1)
        for a in range(n_az):
            for e in range(n_el):
                af[i, a, e] = p.compute_array_factor_at_angle(array_geometry=flat, steering_vector=p.d[:, a, e])
    return pat, af


def main():
    cm = ConfigManager()
    cm.load_cfg(os.path.join(REF, "configs", CFG))
    g = np.load(os.path.join(HERE, "synth_array.npz"))
    rng = np.random.default_rng(20261020)
    sets = {}
    # a: the fixture's own geometries, after every frame
    sets["a"] = (g["az_rad"], g["el_rad"], np.array(g["array_geometry"], dtype=np.float64))
    # b: a track of 65 elements 0.45 wavelengths apart, jittered in all three axes, three times
    lam = processor(cm, g["az_rad"], g["el_rad"]).lambda_m
    geo_b = np.zeros((3, 5, 3, 13))
    for i in range(3):
        x = (np.arange(65) - 64.0) * 0.45 * lam * (1 + 0.1 * i)
        flat = np.stack([x, np.zeros(65), np.zeros(65)]) + 0.05 * lam * rng.standard_normal((3, 65))
        geo_b[i] = flat.reshape(3, 5, 13).transpose(1, 0, 2)
    sets["b"] = (np.deg2rad(np.linspace(-60, 60, 257)), np.array([0.0]), geo_b)
    # c: positions of metres
    sets["c"] = (np.deg2rad(np.linspace(-40, 40, 5)), np.deg2rad(np.array([-10.0, 0.0, 10.0])), rng.uniform(-5.0, 5.0, (1, 3, 3, 11)))
    out = dict(cfg=CFG, lambda_m=lam)
    for name, (az, el, geo) in sets.items():
        p = processor(cm, az, el)
        assert p.lambda_m == lam
        pat, af = patterns(p, geo)
        out.update({f"{name}_az_rad": az, f"{name}_el_rad": el, f"{name}_geometry": geo, f"{name}_d": p.d, f"{name}_pattern": pat,
                    f"{name}_af": af})
        print(name, "geometry", geo.shape, "pattern", pat.shape, pat.dtype, "min", pat.min(), "max", pat.max())
    path = os.path.join(HERE, "synth_array_pattern.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
