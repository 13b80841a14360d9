#!/usr/bin/env python3
"""Generate ``synth_array_calib.npz`` from the IMPORTED reference ``SyntheticArrayBeamformerProcessor(enable_calibration=True)``
with the reference's own ``ConfigManager`` on ``configs/6843_RadVel_ods_10Hz.cfg`` (build container only: the reference never has to
exist where the tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth_array_calib.py

As in ``make_golden_synth_array.py``, ``get_interpolated_response_cart`` is replaced ON THE INSTANCE with a no-op (presentation; it
raises for more than one elevation bin).  ``_find_calibration_targets`` is wrapped on the instance to RECORD the inputs of every
discrete decision (the wrapper calls the reference's method and returns its result unchanged).

Scene: receiver 1, chirp configuration 2 (virtual antenna 9), 3 frames of history, every 3rd chirp (E = 102).  Eight frames, the
gate open at frames 2, 3 and 7.  Four point reflectors (range row, azimuth, amplitude) over noise of sigma 2, integer-valued I/Q.
The phase of a reflector across chirps follows the TRUE track of the platform, whose velocity differs from the reported one by
``TRUE_VEL_ERROR`` -- that is what the calibration has to find.  Cases: (a) 13 azimuth bins x {0, 10} degrees, 1 iteration; (b)
the same, 2 iterations; (c) 2 azimuth bins (no local maximum can exist along azimuth: "no suitable targets" as the reference runs
it).  The margins of every decision the reference took are asserted: >= 0.5 dB between ranked range peaks and to the fourth,
>= 0.5 dB between an azimuth pick and its runner-up, every phase step, modulo 2 pi, <= pi / 2 (so no raw step lies near the unwrap threshold).
"""
import os
import sys

import numpy as np
from scipy.signal import find_peaks

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from mmwave_radar_processing.config_managers.cfgManager import ConfigManager                                      # noqa: E402
from mmwave_radar_processing.processors.simple_synthetic_array_beamformer_processor_multiFrame import (            # noqa: E402
    SyntheticArrayBeamformerProcessor)

CFG = "6843_RadVel_ods_10Hz.cfg"
PARAMS = dict(receiver_idx=1, chirp_cfg_idx=2, num_frames=3, stride=3)
EL_DEG = np.array([0.0, 10.0])
CASES = {"a": (np.linspace(5, 65, 13), 1), "b": (np.linspace(5, 65, 13), 2), "c": (np.array([20.0, 40.0]), 1)}
VELS = np.array([[.2, .01, 0]] * 3 + [[.21, 0, .01], [.3, 0, 0]] + [[.2, 0, 0]] * 3)
TRUE_VEL_ERROR = np.array([0.0012, 0.0005, 0.0])
REFLECTORS = [(12, 20.0, 90.0), (27, 40.0, 70.0), (41, 55.0, 55.0), (52, 30.0, 30.0)]      # range row, azimuth (deg), amplitude
LIVE = (9, 5)                # the antenna of the array, a decoy
NUM_RX, NUM_TX = 4, 3


def raw_of(virt):
    V, S, L = virt.shape
    raw = np.zeros((NUM_RX, S, NUM_TX * L), dtype=np.complex64)
    for tx in range(NUM_TX):
        raw[:, :, tx::NUM_TX] = virt[tx * NUM_RX:(tx + 1) * NUM_RX]
    return raw


def slabs_of(cm, lambda_m, rng):
    """[n, 2, S, loops]: antenna 9 sees the reflectors along the true track, the decoy another scene."""
    S, L = cm.get_num_adc_samples(profile_idx=0), cm.frameCfg_loops
    prof = cm.profile_cfgs[0]
    period_us, frame_s = prof["idleTime_us"] + prof["rampEndTime_us"], cm.frameCfg_periodicity_ms * 1e-3
    raw_idx = NUM_TX * np.arange(L) + PARAMS["chirp_cfg_idx"]                 # raw chirp of loop c
    t_s = -(NUM_TX * L - 1 - raw_idx) * period_us * 1e-6                      # start time relative to the frame's last chirp
    n = len(VELS)
    out = np.zeros((n, 2, S, L), dtype=np.complex64)
    s = np.arange(S)[:, None]
    start = np.zeros(3)
    for f in range(n):
        v_true = VELS[f] + TRUE_VEL_ERROR
        start = start + 2 * v_true * frame_s
        pos = start[:, None] + 2 * t_s[None, :] * v_true[:, None]              # [3, L]
        x = 2.0 * (rng.standard_normal((S, L)) + 1j * rng.standard_normal((S, L)))
        for row, az_deg, amp in REFLECTORS:
            d = np.array([np.cos(np.deg2rad(az_deg)), np.sin(np.deg2rad(az_deg)), 0.0])
            x = x + amp * np.exp(2j * np.pi * row * s / S) * np.exp(-2j * np.pi * (d @ pos) / lambda_m)[None, :]
        out[f, 0] = np.round(x.real) + 1j * np.round(x.imag)
        y = 2.0 * (rng.standard_normal((S, L)) + 1j * rng.standard_normal((S, L)))
        y = y + 80.0 * np.exp(2j * np.pi * ((50 - f) * s / S + 11.2 * np.arange(L)[None, :] / L))
        out[f, 1] = np.round(y.real) + 1j * np.round(y.imag)
    return out


def margins_of(avg, image, targets, d, P, Fq, lambda_m):
    """Assert the margins of the decisions behind `targets`; returns (range dB margin, azimuth dB margin, largest raw step)."""
    peaks, _ = find_peaks(avg, height=0)
    vals = np.sort(avg[peaks])[::-1]
    assert len(peaks) >= 4, len(peaks)
    m_rng = float(np.min(vals[:3] - vals[1:4]))
    assert m_rng >= 0.5, m_rng
    m_az, step = np.inf, 0.0
    for row, a in targets:
        u = np.abs(10 * np.log10(np.abs(image[row, :, 0])))
        pk, _ = find_peaks(u, height=0)
        others = [u[q] for q in pk if q != a]
        if others:
            m_az = min(m_az, float(u[a] - max(others)))
        z = Fq[row] * np.exp(2j * np.pi * (d[:, a, 0] @ P) / lambda_m)
        step = max(step, float(np.abs(np.angle(z[1:] * np.conj(z[:-1]))).max()))      # (the step modulo 2 pi: its distance from +-pi decides)
    assert m_az >= 0.5, m_az
    assert step <= np.pi / 2, step
    return m_rng, m_az, step


def run_case(cm, slabs, az_deg, iters):
    p = SyntheticArrayBeamformerProcessor(cm, az_angle_bins_rad=np.deg2rad(az_deg), el_angle_bins_rad=np.deg2rad(EL_DEG),
                                          min_vel=np.array([0.17, 0.0, 0.0]), max_vel=np.array([0.25, 0.05, 0.05]),
                                          max_vel_stdev=np.array([0.1, 0.1, 0.1]), enable_calibration=True,
                                          num_calibration_iters=iters, **PARAMS)
    p.get_interpolated_response_cart = lambda *a, **k: None
    find, record = p._find_calibration_targets, []

    def recording_find(freq_resps, num_targets=3):
        got = find(freq_resps, num_targets=num_targets)
        record.append((np.array(freq_resps), np.array(p.beamformed_resp), list(got)))
        return got

    p._find_calibration_targets = recording_find
    S, L = slabs.shape[2:]
    out = dict(frames=[], geom=[], geom_cal=[], targets=[], status=[], resp=[], margins=[])
    for f in range(len(VELS)):
        virt = np.zeros((NUM_RX * NUM_TX, S, L), dtype=np.complex64)
        virt[list(LIVE)] = slabs[f]
        del record[:]
        resp = p.process(raw_of(virt), VELS[f])
        if not p.array_geometry_valid:
            assert resp.size == 0
            continue
        P = p.array_geometry.transpose(1, 0, 2).reshape(3, -1)
        tg, status = np.full((3, 2), -1, dtype=np.int32), 0
        for Fq, image, got in record:
            if len(got) < 3:
                break
            with np.errstate(divide="ignore"):
                avg = np.mean(20 * np.log10(np.abs(Fq)), axis=1)
            out["margins"].append(margins_of(avg, image, got, p.d, P, Fq, p.lambda_m))
            tg, status = np.array(got, dtype=np.int32), status + 1
        out["frames"].append(f)
        out["geom"].append(p.array_geometry.copy())
        out["geom_cal"].append(np.array(p.array_geometry_calibrated, dtype=float).copy())
        out["targets"].append(tg)
        out["status"].append(status)
        out["resp"].append(np.array(resp, dtype=np.complex128))
    return p, out


def main():
    cm = ConfigManager()
    cm.load_cfg(os.path.join(REF, "configs", CFG))
    lam = 299792458.0 / (float(cm.profile_cfgs[0]["startFreq_GHz"]) * 1e9)
    slabs = slabs_of(cm, lam, np.random.default_rng(20261020))
    store = dict(cfg=CFG, params=np.array([PARAMS[k] for k in ("receiver_idx", "chirp_cfg_idx", "num_frames", "stride")]),
                 el_rad=np.deg2rad(EL_DEG), velocities=VELS, live=np.array(LIVE), slabs=slabs, lambda_m=lam)
    for name, (az_deg, iters) in CASES.items():
        p, out = run_case(cm, slabs, az_deg, iters)
        assert out["frames"] == [2, 3, 7], out["frames"]
        if name == "c":
            assert out["status"] == [0, 0, 0]
        else:
            assert out["status"] == [iters] * 3, out["status"]
        resps = np.stack(out["resp"])
        store.update({f"{name}_az_rad": np.deg2rad(az_deg), f"{name}_iters": iters, f"{name}_frames": np.array(out["frames"]),
                      f"{name}_geometry": np.stack(out["geom"]), f"{name}_geometry_calibrated": np.stack(out["geom_cal"]),
                      f"{name}_targets": np.stack(out["targets"]), f"{name}_status": np.array(out["status"], dtype=np.int32),
                      f"{name}_responses": resps, f"{name}_peaks": np.abs(resps).reshape(len(resps), -1).max(1)})
        store["min_vel"], store["max_vel"], store["max_vel_stdev"] = p.min_vel, p.max_vel, p.max_vel_stdev
        corr = np.abs(np.stack(out["geom_cal"]) - np.stack(out["geom"])).max(axis=(0, 1, 3))
        print(name, "status", out["status"], "targets", [t.tolist() for t in out["targets"]], "max |correction| x/y/z", corr,
              "margins (range dB, azimuth dB, raw step)", np.array(out["margins"]).round(3).tolist())
    path = os.path.join(HERE, "synth_array_calib.npz")
    np.savez_compressed(path, **store)
    biggest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != "synth_array_calib.npz")
    print(path, os.path.getsize(path), "bytes (largest other fixture:", biggest, ")")
    assert os.path.getsize(path) <= biggest


if __name__ == "__main__":
    main()
