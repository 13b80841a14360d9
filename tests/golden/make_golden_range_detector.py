#!/usr/bin/env python3
"""Generate ``range_detector.npz`` from the IMPORTED reference ``RangeDetector`` (build container only: the reference never has
to exist where the tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_range_detector.py

Two configurations out of ``tests/golden/cfg_scalars.json``: ``6843_RadVel_ods_20Hz.cfg`` (S = 63) and the synthetic one
(S = 256).  ``RangeDetector.process`` does not reformat a raw cube, so each case holds a small ``[V, S, C]`` complex64 cube of
its own (V = 2, C = 3).  Per case: the registry key, the CFAR parameters, the reference's ``dets``, ``thresholds`` and
``range_resp``.  All four 1-D kinds at both sizes; one further case takes chirp 2 (the class itself is fixed to chirp 0, so its
expectation is the class's two steps on ``RangeProcessor.process(cube, chirp_idx=2)``).  The default construction --
``os_cfar_1d`` with ``{}`` -- is recorded as what it is in the reference: a ``TypeError`` of the detector's constructor.

A case is accepted only when no cell lies within 1e-9 (relative) of its threshold; the cube is drawn again until none does.
That is a condition on the input: the recorded indices are the reference's own decisions and nothing else.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.config_managers.cfgManager import ConfigManager                # noqa: E402
from mmwave_radar_processing.processors.range_detector import RangeDetector                  # noqa: E402

CFGS = {63: "6843_RadVel_ods_20Hz.cfg", 256: "__synth_256x128x12__"}
KINDS = {
    "ca_cfar_1d": dict(num_train=6, num_guard=2, pfa=1e-2),
    "os_cfar_1d": dict(num_train=8, num_guard=2, rho=0.75, alpha=3.0),
    "go_cfar_1d": dict(num_train=5, num_guard=1, pfa=5e-2),
    "so_cfar_1d": dict(num_train=7, num_guard=3, pfa=1e-2),
}
V, C = 2, 3
MARGIN = 1e-9


def load_cm(lines):
    with tempfile.NamedTemporaryFile("w", suffix=".cfg", delete=False) as fh:
        fh.write("\n".join(lines) + "\n")
        path = fh.name
    cm = ConfigManager()
    cm.load_cfg(path)
    os.unlink(path)
    return cm


def cube(rng, S):
    """Integer-valued I/Q: a few range tones of different strength on every antenna and chirp, plus noise."""
    s = np.arange(S)[None, :, None]
    x = 8.0 * (rng.standard_normal((V, S, C)) + 1j * rng.standard_normal((V, S, C)))
    for row, amp in ((S * 0.2, 90.0), (S * 0.45 + 0.4, 60.0), (S * 0.7, 30.0), (S * 0.71 + 2, 25.0)):
        x = x + amp * np.exp(2j * np.pi * (row * s / S + rng.uniform(0, 1, size=(V, 1, C))))
    return (np.round(x.real) + 1j * np.round(x.imag)).astype(np.complex64)


def run(det, x, chirp):
    """The class's process(), with the chirp it hard-wires to 0 as a parameter."""
    if chirp == 0:
        dets = det.process(x)
    else:
        det.range_resp = super(RangeDetector, det).process(x, chirp_idx=chirp)
        idxs = det.cfar_detector.detect(det.range_resp)
        det.thresholds = det.cfar_detector.thresholds
        dets = det.dets = np.array(idxs) if len(idxs) > 0 else np.array([])
    thr = det.thresholds
    ok = np.isfinite(thr)
    clear = np.all(np.abs(det.range_resp[ok] - thr[ok]) > MARGIN * np.abs(thr[ok]))
    return clear, dets


def main():
    with open(os.path.join(HERE, "cfg_scalars.json")) as fh:
        table = json.load(fh)
    rng = np.random.default_rng(20261020)
    d, names = {}, []
    for S, cfg in CFGS.items():
        cm = load_cm(table[cfg]["lines"])
        assert cm.get_num_adc_samples(0) == S
        cases = [(key, 0) for key in KINDS] + ([("os_cfar_1d", 2)] if S == 63 else [("ca_cfar_1d", -1)])
        for key, chirp in cases:
            det = RangeDetector(cm, cfar_type=key, cfar_params=dict(KINDS[key]))
            for draws in range(1, 100):
                x = cube(rng, S)
                clear, dets = run(det, x, chirp)
                if clear and len(dets) > 0:
                    break
            else:
                raise AssertionError("no clear draw")
            name = f"{key}_S{S}_chirp{chirp}"
            names.append(name)
            d[f"{name}_cube"], d[f"{name}_dets"] = x, np.asarray(dets, dtype=np.int64)
            d[f"{name}_thresholds"], d[f"{name}_range_resp"] = det.thresholds, det.range_resp
            d[f"{name}_bins"] = det._map_detections_to_bins(np.asarray(dets, dtype=np.int64))
            d[f"{name}_params"] = np.array(json.dumps(KINDS[key]))
            print(f"{name}: {len(dets)} detections after {draws} draw(s)")
        d[f"cfg_S{S}"] = np.array(cfg)
        d[f"range_bins_S{S}"] = det.range_bins
    d["cases"] = np.array(names)
    cm = load_cm(table[CFGS[63]]["lines"])
    try:
        RangeDetector(cm)
        d["default_error"] = np.array("")
    except TypeError:
        d["default_error"] = np.array("TypeError")
    try:
        RangeDetector(cm, cfar_type="nope")
        raise AssertionError("expected ValueError")
    except ValueError as e:
        d["unknown_key_message"] = np.array(str(e))
    path = os.path.join(HERE, "range_detector.npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print(f"wrote {path}: {size / 1024:.0f} KiB, default construction: {d['default_error']!s}")
    assert size <= os.path.getsize(os.path.join(HERE, "micro_doppler.npz"))


if __name__ == "__main__":
    main()
