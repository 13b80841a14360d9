"""Host side of the self-calibrating synthetic-array beamformer (no device): the entries in the header and the ctypes table, the
class ``SelfCalibratingSyntheticArrayProcessor`` stepped over the reference-generated fixture (cases a, b, c of
``tests/golden/make_golden_synth_array_calib.py``; the contraction replaced by numpy), the host-only twin of the kernels' decision
and solve code against the class and on inputs constructed for each rule, the argument refusals of the pipeline, and a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.processors import SelfCalibratingSyntheticArrayProcessor, SyntheticArrayBeamformerProcessor
from mmwave_radar_processing_amd.processors import synthetic_array_beamformer as sab
from test_synth_array_host import config

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
CSRC = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
LAMBDA = 299792458.0 / 60.25e9
# float64 against float64: measured worst |geometry - reference| over cases a and b is 4.2e-17 m (printed below; three ulps of the
# 0.1 m aperture); the bar is 100 x that, because the summation order of the prefix sum and of lstsq legitimately differs
GEOMETRY_TOL = 4.2e-15


def numpy_contract(X, P, d, lam):
    """[S, n_az, n_el] in float64: FFT_S(hann(S) . (X hamming(E)) exp(2 pi i d.P / lambda))."""
    S, E = X.shape
    W = np.hamming(E)[:, None] * np.exp(2j * np.pi * np.tensordot(P.T, d.reshape(3, -1), axes=1) / lam)
    return np.fft.fft(np.hanning(S)[:, None] * (X @ W), axis=0).reshape(S, *d.shape[1:])


def case_processor(g, case, cls=SelfCalibratingSyntheticArrayProcessor, **over):
    rx, cfg_idx, H, stride = (int(x) for x in g["params"])
    kw = dict(receiver_idx=rx, chirp_cfg_idx=cfg_idx, num_frames=H, stride=stride, az_angle_bins_rad=g[f"{case}_az_rad"],
              el_angle_bins_rad=g["el_rad"], min_vel=g["min_vel"], max_vel=g["max_vel"], max_vel_stdev=g["max_vel_stdev"])
    if cls is SelfCalibratingSyntheticArrayProcessor:
        kw["num_calibration_iters"] = int(g[f"{case}_iters"])
    kw.update(over)
    return cls(config(str(g["cfg"])), **kw)


def raw_cube(g, f):
    S, L = g["slabs"].shape[2:]
    raw = np.zeros((4, S, 3 * L), dtype=np.complex64)
    raw[1, :, 2::3] = g["slabs"][f, 0]
    raw[1, :, 1::3] = g["slabs"][f, 1]
    return raw


def test_entries_are_declared_bound_and_leave_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+mmw_synth_array_calibrate\s*\(([^)]*)\)\s*;", text)
    assert m, "mmw_synth_array_calibrate is not declared in include/mmwgpu.h"
    names = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names == ["ctx", "d_cubes", "n_resident", "V", "S", "C", "v", "k", "H", "h_frames", "n_out", "h_P", "h_dirs", "n_az", "n_el",
                     "lambda_m", "n_iters", "d_out", "d_Pcal", "d_status", "d_targets"]
    assert len(_lib._SIGNATURES["mmw_synth_array_calibrate"]) == len(names)
    m = re.search(r"\bint\s+mmw_diag_synth_array_calib_host\s*\(([^)]*)\)\s*;", text)
    assert m and len(_lib._SIGNATURES["mmw_diag_synth_array_calib_host"]) == len(m.group(1).split(","))
    assert {"mmw_synth_array_calibrate", "mmw_diag_synth_array_calib_host"} <= set(_lib.EXPORTED)
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_synth_calib\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_synth_calib\.o:.*-ffp-contract=off", make, flags=re.M)
    lib = _lib.load_library()
    assert lib.mmw_synth_array_calibrate and lib.mmw_diag_synth_array_calib_host


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_stepped_class_reproduces_the_reference(golden, monkeypatch, case):
    g = golden("synth_array_calib.npz")
    p = case_processor(g, case)
    monkeypatch.setattr(p._core, "contract", lambda X, P: numpy_contract(X, P, p.d, p.lambda_m))
    frames, worst_g, worst_r = g[f"{case}_frames"].tolist(), 0.0, 0.0
    seen = 0
    for f, vel in enumerate(g["velocities"]):
        out = p.process(raw_cube(g, f), vel)
        assert (out.size > 0) == (f in frames)
        if f not in frames:
            continue
        i = frames.index(f)
        tg = np.full((3, 2), -1)
        tg[:len(p.calibration_targets)] = np.array(p.calibration_targets).reshape(-1, 2)
        assert np.array_equal(tg, g[f"{case}_targets"][i]) and p.calibration_status == int(g[f"{case}_status"][i])
        worst_g = max(worst_g, np.abs(p.array_geometry_calibrated - g[f"{case}_geometry_calibrated"][i]).max())
        worst_r = max(worst_r, np.abs(out - g[f"{case}_responses"][i]).max() / g[f"{case}_peaks"][i])
        if case == "c":
            assert np.array_equal(p.array_geometry_calibrated, p.array_geometry)
        else:
            assert np.abs(p.array_geometry_calibrated - p.array_geometry).max() > 1e-4      # there was something to correct
        seen += 1
    print(f"case {case}: worst geometry difference {worst_g:.3g} m, worst response difference {worst_r:.3g} of the peak")
    assert seen == 3 and worst_g <= GEOMETRY_TOL and worst_r <= 1e-12


def test_plain_class_and_pipeline_keep_refusing_calibration(golden):
    g = golden("synth_array_calib.npz")
    with pytest.raises(NotImplementedError):
        case_processor(g, "a", cls=SyntheticArrayBeamformerProcessor, enable_calibration=True)
    with pytest.raises(ValueError):
        case_processor(g, "a", num_calibration_iters=0)


# ------------------------------------------------------------------------------------------------------------------- the host twin
def twin(avg, mag, Fq, P, d, lam=LAMBDA, avg_err=None, mag_band=0.0, l1=None):
    lib = _lib.load_library()
    S, n_az = mag.shape
    n_el, E = d.shape[2], P.shape[1]
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)          # noqa: E731
    avg, mag, P, dirs, avg_err, l1 = c(avg), c(mag), c(P), c(d.reshape(3, -1)), c(avg_err), c(l1)
    Fq = np.ascontiguousarray(Fq, dtype=np.complex128)
    Pcal, tg, info = np.full((3, E), np.nan), np.full((3, 2), -7, np.int32), np.zeros(4, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                                     # noqa: E731
    _lib.check(lib.mmw_diag_synth_array_calib_host(ptr(avg), ptr(avg_err), S, ptr(mag), mag_band, n_az, n_el, ptr(Fq), ptr(l1), E, ptr(P),
                                                   ptr(dirs), lam, ptr(Pcal), ptr(tg), ptr(info)))
    return Pcal, tg, info


def directions(n_az, n_el=1, lo=5, hi=65):
    th, ph = np.meshgrid(np.deg2rad(np.linspace(lo, hi, n_az)), np.deg2rad(np.linspace(0, 10, n_el)), indexing="ij")
    return np.array([np.cos(th) * np.cos(ph), np.sin(th) * np.cos(ph), np.sin(ph)])


def strong_scene(rng, S, E, d, n_t=3):
    """A window [S, E] with n_t strong reflectors on distinct rows and azimuth bins, a geometry and its perturbed truth."""
    n_az = d.shape[1]
    P = np.zeros((3, E))
    P[0] = np.linspace(-0.1, 0.0, E)
    true = P.copy()
    true[0] += np.linspace(0, 4e-4, E)
    true[1] += np.linspace(0, 2e-4, E) ** 1
    rows = rng.choice(np.arange(3, S - 3, 4), n_t, replace=False)
    azs = rng.choice(np.arange(1, n_az - 1), n_t, replace=False)
    s = np.arange(S)[:, None]
    X = 2.0 * (rng.standard_normal((S, E)) + 1j * rng.standard_normal((S, E)))
    for t, (r, a) in enumerate(zip(rows, azs)):
        X = X + (90 - 15 * t) * np.exp(2j * np.pi * r * s / S) * np.exp(-2j * np.pi * (d[:, a, 0] @ true) / LAMBDA)[None, :]
    return np.round(X.real) + 1j * np.round(X.imag), P


@pytest.mark.parametrize("S,E,n_az,n_el,seed", [(63, 102, 13, 2, 1), (64, 32, 9, 1, 2), (32, 17, 7, 1, 3), (128, 256, 21, 1, 4)])
def test_twin_equals_the_class_functions_on_strong_scenes(S, E, n_az, n_el, seed):
    rng = np.random.default_rng(seed)
    d = directions(n_az, n_el)
    X, P = strong_scene(rng, S, E, d)
    Fq = sab.calibration_spectra(X)
    img = numpy_contract(X, P, d, LAMBDA)
    want_t = sab.calibration_targets(Fq, img)
    assert len(want_t) == 3
    want_P = sab.calibrated_geometry(Fq, P, want_t, d, LAMBDA)
    avg = np.mean(20 * np.log10(np.abs(Fq)), axis=1)
    Pcal, tg, info = twin(avg, np.abs(img[:, :, 0]), Fq, P, d)
    assert info[0] == 1 and info[1] == 0 and np.array_equal(tg, np.array(want_t))
    diff = np.abs(Pcal - want_P).max()
    print(f"S {S} E {E}: twin against numpy {diff:.3g} m, correction {np.abs(want_P - P).max():.3g} m")
    assert diff <= GEOMETRY_TOL and np.array_equal(Pcal[2], P[2]) and np.array_equal(Pcal[:, 0], P[:, 0])
    # with the error bounds of the device on: nothing is flagged on such a scene
    l1 = np.abs(X.real).sum(0) + np.abs(X.imag).sum(0)
    _, tg2, info2 = twin(avg, np.abs(img[:, :, 0]), Fq, P, d, avg_err=np.full(S, 1e-9), mag_band=1e-6 * np.abs(img).max(), l1=l1)
    assert info2[0] == 1 and np.array_equal(tg2, tg)


def flat_inputs(S=16, E=6, n_az=7):
    """avg with three clear peaks (rows 3, 8, 12), a magnitude image with one clear azimuth peak per row, flat phases."""
    d = directions(n_az)
    avg = 1.0 + 0.01 * np.arange(S)            # (ramps: no ties and no peaks besides the spikes)
    avg[[3, 8, 12]] = [30.0, 20.0, 10.0]
    mag = np.tile(2.0 + 0.1 * np.arange(n_az), (S, 1))
    mag[3, 2], mag[8, 4], mag[12, 5] = 9.0, 8.0, 7.0
    P = np.zeros((3, E))
    P[0] = np.arange(E) * 1e-3
    Fq = np.ones((S, E), dtype=complex)
    return avg, mag, Fq, P, d


def steered(Fq, P, d, rows_az, phases):
    """Fq whose rows, steered to their targets, have the given phase histories."""
    Fq = Fq.copy()
    for (r, a), ph in zip(rows_az, phases):
        Fq[r] = np.exp(1j * np.asarray(ph)) * np.exp(-2j * np.pi * (d[:, a, 0] @ P) / LAMBDA)
    return Fq


def test_twin_rules_on_constructed_inputs():
    avg, mag, Fq, P, d = flat_inputs()
    Pcal, tg, info = twin(avg, mag, Fq, P, d)
    assert info.tolist()[:3] == [1, 0, 3] and tg.tolist() == [[3, 2], [8, 4], [12, 5]]
    # a plateau peak reports its middle sample (rows 7..9 equal -> 8), along range and along azimuth (bins 3..5 -> 4)
    a2, m2 = avg.copy(), mag.copy()
    a2[[7, 9]] = 20.0
    m2[8, [3, 5]] = 8.0
    assert twin(a2, m2, Fq, P, d)[1].tolist() == [[3, 2], [8, 4], [12, 5]]
    # the first maximum on ties along azimuth
    m3 = mag.copy()
    m3[3, [2, 5]] = 9.0
    assert twin(avg, m3, Fq, P, d)[1][0].tolist() == [3, 2]
    # |dB| with magnitudes on both sides of 1: 0.05 (26 dB below) beats 9 (19 dB above); 0.5 does not beat 9
    m4 = mag.copy()
    m4[3] = [2.0, 1.5, 9.0, 1.2, 0.5, 0.05, 0.3]
    want = sab.calibration_targets(np.power(10.0, avg / 20)[:, None] * np.ones((1, 4)), m4[:, :, None])
    got = twin(avg, m4, Fq, P, d)[1]
    assert got[0].tolist() == [3, 5] and [tuple(t) for t in got.tolist()] == want
    # a negative avg peak does not count (height = 0): fewer than three range peaks, like a non-finite avg: no suitable targets
    below = avg - 4.0
    below[[3, 8, 12]] = [30.0, 20.0, -0.5]
    for bad in (below, np.where(avg == 1.0, -np.inf, avg), np.where(avg == 30.0, np.nan, avg)):
        Pcal, tg, info = twin(bad, mag, Fq, P, d)
        assert info.tolist() == [0, 0, 0, 0] and (tg == -1).all() and np.array_equal(Pcal, P)
    # a row without an azimuth peak drops its target: no correction
    m5 = mag.copy()
    m5[12] = np.linspace(2, 8, 7)
    Pcal, tg, info = twin(avg, m5, Fq, P, d)
    assert info.tolist() == [0, 0, 3, 0] and np.array_equal(Pcal, P)


def test_twin_phase_wrap_and_rank_deficiency():
    avg, mag, Fq, P, d = flat_inputs()
    targets = [(3, 2), (8, 4), (12, 5)]
    E = P.shape[1]
    # a step of exactly +pi stays +pi (numpy: -pi becomes +pi for a positive raw step), a step of -pi stays -pi
    ph = np.zeros((3, E))
    ph[0, 1:] = np.pi                 # one raw step of +pi in the first target's history
    ph[1, 3:] = -np.pi
    F2 = np.empty_like(Fq)
    F2[:] = Fq
    for (r, a), h in zip(targets, ph):
        F2[r] = np.exp(1j * h)
    Praw = np.zeros_like(P)           # no steering phase at all: angle(z) is exactly 0 or +-pi
    Pcal, tg, info = twin(avg, mag, F2, Praw, d)
    want = sab.calibrated_geometry(F2, Praw, targets, d, LAMBDA)
    steps = np.diff(np.unwrap(np.angle(F2[[3, 8, 12]])), axis=1)
    assert steps[0, 0] == np.pi and abs(steps[1, 2]) == np.pi
    assert info[0] == 1 and np.abs(Pcal - want).max() <= 1e-15 and np.abs(want).max() > 1e-4
    # with an error bound on the phases the same input is flagged: wrap
    _, _, info = twin(avg, mag, F2, Praw, d, l1=np.full(E, 1.0))
    assert info[0] == -1 and info[1] == 4
    # two targets on one azimuth: rank 2 still; all three on one azimuth: rank 1 -- flagged (condition) and solved minimum-norm
    m2 = mag.copy()
    m2[[3, 8, 12]] = mag[0]
    m2[3, 4] = m2[8, 4] = m2[12, 4] = 9.0
    tg1 = [(3, 4), (8, 4), (12, 4)]
    F3 = steered(Fq, P, d, tg1, [np.linspace(0, 0.3, E)] * 3)
    Pcal, tg, info = twin(avg, m2, F3, P, d)
    want = sab.calibrated_geometry(F3, P, tg1, d, LAMBDA)
    assert info.tolist() == [-1, 8, 3, 1] and np.abs(Pcal - want).max() <= 1e-15 and np.abs(want - P).max() > 1e-6
    m2[8, 4], m2[8, 2] = mag[0, 4], 9.0
    Pcal, tg, info = twin(avg, m2, F3, P, d)
    assert info[0] == 1 and tg.tolist() == [[3, 4], [8, 2], [12, 4]]


def test_twin_flags_each_reason_alone():
    avg, mag, Fq, P, d = flat_inputs()
    S = len(avg)
    assert twin(avg, mag, Fq, P, d, avg_err=np.full(S, 1e-3), mag_band=1e-3, l1=np.full(P.shape[1], 1.0))[2][0] == 1
    # range: the third and fourth peak inside the band; two neighbours inside the band; a peak inside the band of height 0
    a2 = avg.copy()
    a2[5] = 10.0 + 1e-4
    assert twin(a2, mag, Fq, P, d, avg_err=np.full(S, 1e-3))[2].tolist()[:2] == [-1, 1]
    assert twin(a2, mag, Fq, P, d)[2].tolist()[:3] == [0, 0, 3]       # decided: rows 3, 8, 5, and row 5 has no azimuth peak
    a3 = avg.copy()
    a3[14] = a3[13] + 1e-4
    assert twin(a3, mag, Fq, P, d, avg_err=np.full(S, 1e-3))[2].tolist()[:2] == [-1, 1]
    # azimuth: the pick and a rival inside the band; a magnitude inside the band of 1; a zero magnitude
    m2 = mag.copy()
    m2[3, 5] = 9.0 - 1e-4
    assert twin(avg, m2, Fq, P, d, mag_band=1e-3)[2].tolist()[:2] == [-1, 2]
    assert twin(avg, m2, Fq, P, d)[1][0].tolist() == [3, 2]
    m3 = mag.copy()
    m3[8, 3] = 1.0 + 1e-5               # (next to the pick; the same value at the far end of the row would not matter)
    assert twin(avg, m3, Fq, P, d, mag_band=1e-3)[2].tolist()[:2] == [-1, 2]
    m4 = mag.copy()
    m4[12, 1] = 0.0
    assert twin(avg, m4, Fq, P, d)[2].tolist()[:2] == [-1, 2]


def test_pipeline_refuses_bad_arguments_before_any_device_use(golden):
    g = golden("synth_array_calib.npz")
    proc = case_processor(g, "a", cls=SyntheticArrayBeamformerProcessor)
    pipe = FramePipeline.__new__(FramePipeline)          # no context, no buffers: a device use would raise AttributeError
    pipe.V, pipe.S, pipe.C, pipe.n_frames = 12, 63, 100, 8
    vel = g["velocities"]
    for kw, match in ((dict(num_calibration_iters=0), "num_calibration_iters"), (dict(num_calibration_iters=9), "num_calibration_iters")):
        with pytest.raises(ValueError, match=match):
            pipe.synthetic_array_calibrated(proc, vel, **kw)
    with pytest.raises(ValueError, match="velocities"):
        pipe.synthetic_array_calibrated(proc, vel[:5])
    pipe.S = 64
    with pytest.raises(ValueError, match="do not match"):
        pipe.synthetic_array_calibrated_device(proc, vel)
    pipe.S = 63
    proc.enable_calibration = True
    with pytest.raises(ValueError, match="calibration"):
        pipe.synthetic_array_calibrated(proc, vel)
    proc.enable_calibration = False
    proc.receiver_idx = 4
    with pytest.raises(ValueError, match="receiver"):
        pipe.synthetic_array_calibrated(proc, vel)


def test_argument_checks_and_host_twin_under_address_and_ub_sanitizers(tmp_path):
    """mmw_tu_synth_calib.hip compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/synth_array_calib_sanitize.cpp, a program of its own that launches nothing (the recipe of the Doppler-azimuth peak
    pickers' test): every refused argument of both entries with the outputs untouched, n_out == 0, and the host twin over a sweep
    of shapes.  (No GPU sanitizer is involved; the kernels are launch stubs that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_synth_calib.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(CSRC, "mmw_tu_synth_calib.hip")], check=True)
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "synth_array_calib_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "synth_array_calib_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
