"""Host side of the synthetic-array beam patterns (no device): the entries in the header, the ctypes table and the Makefile; the
host-only twin ``mmw_diag_synth_array_pattern_host`` -- the accumulation the kernel runs -- against the reference-generated fixture
under both bounds of ``synth_pattern_cases``; exact ones, the NaN frame; ``compute_array_factor_at_angle``; every argument check
of the Python layer on a pipeline whose context is never touched; the argument checks of ``mmw_synth_array_pattern`` and the host
twin over a sweep of sizes under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mmwave_radar_processing_amd import _lib, batch
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.processors import SelfCalibratingSyntheticArrayProcessor, SyntheticArrayBeamformerProcessor
from mmwave_radar_processing_amd.processors.steering_beamformers import SyntheticArrayBeamformerCore
from synth_pattern_cases import SETS, af_bound, check, directions, fixture_set, host_patterns, nan_case
from test_synth_array_host import _NoDevice, fixture_processor

CSRC = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")


def test_entries_are_declared_bound_built_and_leave_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmwgpu.h")).read(), flags=re.S)
    want = {"mmw_synth_array_pattern": ["ctx", "d_P", "n", "E", "h_dirs", "T", "lambda_m", "d_pattern", "d_af"],
            "mmw_diag_synth_array_pattern_host": ["h_P", "n", "E", "h_dirs", "T", "lambda_m", "h_pattern", "h_af"]}
    for name, names in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/mmwgpu.h"
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == names
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == len(names)
        assert hasattr(_lib.load_library(), name)
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7
    assert _lib.load_library().mmw_abi_version() == 7
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_synth_pattern\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_synth_pattern\.o:.*-ffp-contract=off", make, flags=re.M)
    assert os.path.exists(os.path.join(CSRC, "mmw_tu_synth_pattern.hip")) and os.path.exists(os.path.join(CSRC, "mmw_synth_pattern.h"))


@pytest.mark.parametrize("name", SETS)
def test_host_entry_against_the_reference_fixture(golden, name):
    P, d, lam, want_pattern, want_af = fixture_set(golden("synth_array_pattern.npz"), name)
    pat, af = host_patterns(P, d, lam)
    check(f"host entry, set {name}", pat, af, want_pattern, want_af, af_bound(P, d, lam))
    # without the array factor: the same patterns
    assert np.array_equal(host_patterns(P, d, lam, with_factor=False)[0].view(np.uint32), pat.view(np.uint32))


def test_fixture_holds_what_the_issue_lists(golden):
    g = golden("synth_array_pattern.npz")
    shapes = {name: (fixture_set(g, name)[0].shape, g[f"{name}_pattern"].shape) for name in SETS}
    assert shapes == {"a": ((8, 3, 102), (8, 7, 2)), "b": ((3, 3, 65), (3, 257, 1)), "c": ((1, 3, 33), (1, 5, 3))}
    s = golden("synth_array.npz")
    assert np.array_equal(g["a_geometry"], s["array_geometry"]) and np.array_equal(g["a_d"], s["d"]) and float(g["lambda_m"]) == float(s["lambda_m"])
    assert 4.5 < np.abs(g["c_geometry"]).max() <= 5.0
    for name in SETS:
        assert g[f"{name}_pattern"].dtype == np.float32 and g[f"{name}_af"].dtype == np.complex128
        assert (g[f"{name}_pattern"].reshape(len(g[f"{name}_pattern"]), -1).max(1) == 1.0).all()


def test_zero_geometry_and_one_element_give_exact_ones():
    d = directions(67, 3)
    pat, af = host_patterns(np.zeros((2, 3, 130)), d, 0.0039)
    assert (pat == 1.0).all() and (af == 130.0).all()
    rng = np.random.default_rng(3)
    pat, af = host_patterns(rng.uniform(-2, 2, (4, 3, 1)), d, 0.0039)
    assert (pat == 1.0).all() and np.abs(np.abs(af) - 1.0).max() <= 2.0 ** -51


def test_nan_frame_is_all_nan_and_leaves_the_others_alone():
    P, bad, d, lam = nan_case()
    clean, clean_af = host_patterns(P, d, lam)
    got, got_af = host_patterns(bad, d, lam)
    assert np.isnan(got[1]).all() and np.isnan(got_af[1]).all()
    for i in (0, 2):
        assert np.array_equal(got[i].view(np.uint32), clean[i].view(np.uint32)) and np.array_equal(got_af[i].view(np.float64), clean_af[i].view(np.float64))
    assert np.isfinite(clean).all()
    inf = P.copy()
    inf[2, 0, 0] = np.inf
    assert np.isnan(host_patterns(inf, d, lam)[0][2]).all()


def test_array_factor_at_angle_equals_the_fixture(golden):
    g = golden("synth_array_pattern.npz")
    for name in SETS:
        P, d, lam, _, want_af = fixture_set(g, name)
        core = SyntheticArrayBeamformerCore(g[f"{name}_az_rad"], g[f"{name}_el_rad"], lam, ctx=_NoDevice())
        assert np.array_equal(core.d, d)
        got = np.array([[[core.compute_array_factor_at_angle(P[i], d[:, a, e]) for e in range(d.shape[2])] for a in range(d.shape[1])]
                        for i in range(len(P))])
        assert got.dtype == np.complex128 and np.array_equal(got.view(np.float64), want_af.view(np.float64)), name      # the same expression
    p = fixture_processor(golden("synth_array.npz"))
    P, d, lam, _, want_af = fixture_set(g, "a")
    assert p.compute_array_factor_at_angle(P[2], p.d[:, 3, 1]) == want_af[2, 3, 1]
    for cls in (SyntheticArrayBeamformerProcessor, SelfCalibratingSyntheticArrayProcessor):
        assert callable(getattr(cls, "compute_array_factor_at_angle")) and callable(getattr(cls, "compute_synthetic_array_pattern"))


def test_every_argument_check_comes_before_any_device_use(golden):
    g = golden("synth_array.npz")
    p = fixture_processor(g)
    nodev = _NoDevice()
    fp = FramePipeline.__new__(FramePipeline)
    fp.ctx = fp.bufs = fp.d_in = nodev
    fp.n_frames = 8
    fp.V, fp.S, fp.C = 12, 63, 100
    # the shape of velocities: the module function, the pipeline with and without calibration, the device twin
    for vel in (np.zeros((8, 2)), np.zeros(8), np.zeros((2, 8, 3))):
        with pytest.raises(ValueError, match="velocities"):
            batch.synthetic_array_patterns(p, vel, ctx=nodev)
        for calibrated in (False, True):
            with pytest.raises(ValueError, match="velocities"):
                fp.synthetic_array_patterns(p, vel, calibrated=calibrated)
            with pytest.raises(ValueError, match="velocities"):
                fp.synthetic_array_patterns_device(p, vel, calibrated=calibrated)
    with pytest.raises(ValueError, match="velocities"):
        fp.synthetic_array_patterns(p, g["velocities"][:7], calibrated=True)            # one row per resident frame
    for n_it in (0, 9):
        with pytest.raises(ValueError, match="num_calibration_iters"):
            fp.synthetic_array_patterns(p, g["velocities"], calibrated=True, num_calibration_iters=n_it)
    # P, d and lambda_m of array_patterns
    d, P = directions(5, 2), np.zeros((2, 3, 9))
    for bad in (np.zeros((3, 9)), np.zeros((2, 2, 9)), np.zeros((2, 3, 0)), np.zeros((2, 9, 3)), np.zeros((1, 2, 3, 9))):
        with pytest.raises(ValueError, match=r"array_patterns: P must be \[n, 3, E\]"):
            batch.array_patterns(bad, d, 0.0039, ctx=nodev)
    for bad in (np.zeros((3, 10)), np.zeros((2, 5, 2)), np.zeros((3, 0, 2)), np.zeros((5, 2, 3))):
        with pytest.raises(ValueError, match=r"array_patterns: d must be \[3, n_az, n_el\]"):
            batch.array_patterns(P, bad, 0.0039, ctx=nodev)
    for bad in (0.0, -0.0039, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_m"):
            batch.array_patterns(P, d, bad, ctx=nodev, with_factor=True)
    # the mirrored class: the geometry's shape, and a wavelength or a direction table that was overwritten
    with pytest.raises(ValueError, match="array_geometry"):
        SyntheticArrayBeamformerCore([0.0, 0.1], [0.0], 0.0039, ctx=nodev).compute_synthetic_array_pattern(np.zeros((3, 34)))
    p.lambda_m = 0.0
    with pytest.raises(ValueError, match="lambda_m"):
        fp.synthetic_array_patterns(p, g["velocities"])
    p = fixture_processor(g)
    p.d = np.zeros((3, 14))
    with pytest.raises(ValueError, match="d must be"):
        fp.synthetic_array_patterns(p, g["velocities"])
    # no frames: empty results of the right shape, still without a device
    out, af = batch.array_patterns(np.zeros((0, 3, 9)), d, 0.0039, ctx=nodev, with_factor=True)
    assert out.shape == (0, 5, 2) and out.dtype == np.float32 and af.shape == (0, 5, 2) and af.dtype == np.complex128


def test_argument_checks_and_host_sweep_under_address_and_ub_sanitizers(tmp_path):
    """mmw_tu_synth_pattern.hip's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/synth_array_pattern_sanitize.cpp, a program of its own that launches nothing: every class of refused argument and
    n == 0 through mmw_synth_array_pattern, and the host-only twin over a sweep of (n, E, T) with exactly sized arrays.  (No GPU
    sanitizer is involved; the kernels are launch stubs that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_synth_pattern.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(CSRC, "mmw_tu_synth_pattern.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "synth_array_pattern_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "synth_array_pattern_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
