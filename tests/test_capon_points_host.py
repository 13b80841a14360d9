"""Capon point clouds without a GPU: the host twin of the kernel (mmw_diag_capon_doppler_host: the kernel's own arithmetic, in its
order) against the float64 NumPy restatement of tests/capon_points_cases.py, the argument checks, the exports and the sanitizer
program.

Tolerances are the issue's.  Spectra: |z| within 1e-9 of the detection's peak -- for delta = 1e-3 and n <= 16, cond(R) <=
(1 + delta) n / delta ~ 1.6e4, so the solve errs by about cond n eps ~ 6e-11 and a 512-term float64 sum by 1e-13.  Doppler bin:
identical wherever the restatement's two largest |z| differ by more than 1e-8 relatively; no detection of the chosen seeds falls
inside that band (checked here on the restatement alone), so none is excluded.  For K = 2 the Hann window is all zero: dop 0, peak 0.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import capon_points_cases as cc
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.detectors import CaCFAR1D, CaCFAR2D, OsCFAR2D
from mmwave_radar_processing_amd.processors.steering_beamformers import capon_points_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
HOST_IDS = ["x".join(map(str, c[:3])) for c in cc.HOST_SHAPES]


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_entry(X, dets, counts, thetas, cap, delta=cc.DELTA, windowing=1, rows=None, vel=None, spec=True, points=True, fill=7):
    """mmw_diag_capon_doppler_host on poisoned outputs: (status, dop, peak, spec, points)."""
    lib = _lib.load_library()
    F, n, R, K = X.shape
    r, v = cc.tables(R, K)
    rows = r if rows is None else rows
    vel = v if vel is None else vel
    dop, peak = np.full((F, cap), fill, np.int32), np.full((F, cap), float(fill))
    sp, pt = np.full((F, cap, K), float(fill)), np.full((F, cap, 4), float(fill))
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    rc = lib.mmw_diag_capon_doppler_host(X.ctypes.data, dets.ctypes.data, counts.ctypes.data, dptr(th), dop.ctypes.data,
                                         peak.ctypes.data, sp.ctypes.data if spec else None, pt.ctypes.data if points else None,
                                         rows.ctypes.data if points else None, vel.ctypes.data if points else None, F, n, R, K,
                                         len(th), cap, delta, windowing)
    return rc, dop, peak, sp, pt


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_the_new_entries_and_keeps_abi_7():
    lib = _lib.load_library()
    assert hasattr(lib, "mmw_capon_doppler") and hasattr(lib, "mmw_diag_capon_doppler_host")
    assert lib.mmw_abi_version() == 7 == _lib.ABI_VERSION
    assert "mmw_capon_doppler" in _lib.EXPORTED and "mmw_diag_capon_doppler_host" in _lib.EXPORTED


# ------------------------------------------------------------------------------------------------ seeds (restatement alone)
@pytest.mark.parametrize("case", cc.HOST_SHAPES, ids=HOST_IDS)
def test_no_detection_of_the_seeds_lies_in_the_doppler_band(case):
    n, R, K, seed = case
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    for windowing in (True, False):
        if K == 2 and windowing:
            continue                    # an all-zero window: the rule there is dop 0, peak 0
        for f in range(len(X)):
            _, _, spec = cc.doppler_reference(X[f], dets[f, :counts[f]], cc.THETAS, cc.DELTA, windowing)
            assert min(cc.top_two_gap(s) for s in spec) > cc.DOP_BAND


# ------------------------------------------------------------------------------------------------ host twin vs restatement
@pytest.mark.parametrize("windowing", [1, 0])
@pytest.mark.parametrize("case", cc.HOST_SHAPES, ids=HOST_IDS)
def test_host_twin_against_restatement(case, windowing):
    n, R, K, seed = case
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    cap = dets.shape[1]
    rows, vel = cc.tables(R, K)
    rc, dop, peak, spec, pts = host_entry(X, dets, counts, cc.THETAS, cap, windowing=windowing)
    assert rc == _lib.MMW_OK
    for f in range(len(X)):
        m = counts[f]
        assert {(0, 0), (0, cc.T_ANGLES - 1), (R - 1, 1)} <= {tuple(d) for d in dets[f, :m]}        # first and last row, several each
        rd, rp, rs = cc.doppler_reference(X[f], dets[f, :m], cc.THETAS, cc.DELTA, bool(windowing))
        if K == 2 and windowing:
            assert np.all(dop[f, :m] == 0) and np.all(peak[f, :m] == 0) and np.all(spec[f, :m] == 0)
        else:
            assert np.array_equal(dop[f, :m], rd)
            err = np.max(np.abs(spec[f, :m] - rs) / rp[:, None])
            print(f"{case} windowing {windowing} frame {f}: spectrum error {err:.2e} of the peak")
            assert err <= cc.SPEC_TOL and np.max(np.abs(peak[f, :m] - rp) / rp) <= cc.SPEC_TOL
            assert np.array_equal(peak[f, :m], spec[f, np.arange(m), dop[f, :m]])
        want = cc.points_reference(dets[f, :m], dop[f, :m], cc.THETAS, rows, vel)
        assert np.array_equal(pts[f, :m], want)             # one rounding per product on host-made tables
        assert np.all(dop[f, m:] == 0) and np.all(peak[f, m:] == 0) and np.all(spec[f, m:] == 0) and np.all(pts[f, m:] == 0)


def test_optional_outputs_may_be_null():
    n, R, K, seed = cc.HOST_SHAPES[0]
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    full = host_entry(X, dets, counts, cc.THETAS, dets.shape[1])
    bare = host_entry(X, dets, counts, cc.THETAS, dets.shape[1], spec=False, points=False)
    assert bare[0] == _lib.MMW_OK and np.array_equal(bare[1], full[1]) and np.array_equal(bare[2], full[2])
    assert np.all(bare[3] == 7) and np.all(bare[4] == 7)


# ------------------------------------------------------------------------------------------------ degenerate inputs
def test_degenerate_rows_bad_indices_and_clamped_counts():
    n, R, K, seed = cc.HOST_SHAPES[0]
    X = np.array(cc.host_snapshots(n, R, K, seed))
    X[0, :, 2, :] = 0                                       # an all-zero row
    X[1, 3, 4, 5] = np.nan                                  # a NaN in a row
    cap = 10
    dets = np.zeros((2, cap, 2), np.int32)
    dets[0, :6] = [(0, 4), (2, 0), (2, 9), (2, 32), (5, 1), (5, 2)]
    dets[1] = [(1, 1), (4, 0), (4, 31), (R, 0), (-1, 3), (0, cc.T_ANGLES), (0, -1), (2**31 - 1, 0), (3, 3), (5, 32)]
    counts = np.array([6, cap + 50], np.int32)              # frame 1: above cap, clamped
    rc, dop, peak, spec, pts = host_entry(X, dets, counts, cc.THETAS, cap)
    assert rc == _lib.MMW_OK
    for j in (1, 2, 3):                                     # the zero row: -1 / NaN, the position stays
        assert dop[0, j] == -1 and np.isnan(peak[0, j]) and np.all(np.isnan(spec[0, j]))
        assert np.all(np.isfinite(pts[0, j, :3])) and np.isnan(pts[0, j, 3])
    for j in (0, 4, 5):
        assert dop[0, j] >= 0 and np.isfinite(peak[0, j])
    assert np.all(dop[0, 6:] == 0) and np.all(peak[0, 6:] == 0) and np.all(spec[0, 6:] == 0) and np.all(pts[0, 6:] == 0)
    for j in (1, 2):                                        # the NaN row
        assert dop[1, j] == -1 and np.isnan(peak[1, j]) and np.isnan(pts[1, j, 3])
    for j in (3, 4, 5, 6, 7):                               # q or t out of range
        assert dop[1, j] == -1 and np.isnan(peak[1, j]) and np.all(np.isnan(spec[1, j]))
        assert np.all(np.isnan(pts[1, j, [0, 1, 3]])) and pts[1, j, 2] == 0
    for j in (0, 8, 9):                                     # every slot up to cap is served, none beyond
        assert dop[1, j] >= 0 and np.isfinite(peak[1, j])
    rd, rp, _ = cc.doppler_reference(X[1], dets[1], cc.THETAS, cc.DELTA, True)
    assert np.array_equal(dop[1], rd)
    neg = host_entry(X, dets, np.array([-3, 0], np.int32), cc.THETAS, cap)
    assert neg[0] == _lib.MMW_OK and np.all(neg[1] == 0) and np.all(neg[2] == 0) and np.all(neg[4] == 0)


def test_unordered_lists_give_the_same_cells():
    n, R, K, seed = cc.HOST_SHAPES[1]
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    _, dop, peak, spec, _ = host_entry(X, dets, counts, cc.THETAS, dets.shape[1])
    perm = np.random.default_rng(1).permutation(counts[0])
    shuffled = dets.copy()
    shuffled[0, :counts[0]] = dets[0, perm]
    _, dop2, peak2, spec2, _ = host_entry(X, shuffled, counts, cc.THETAS, dets.shape[1])
    assert np.array_equal(dop2[0, :counts[0]], dop[0, perm]) and np.array_equal(peak2[0, :counts[0]], peak[0, perm])
    assert np.array_equal(spec2[0, :counts[0]], spec[0, perm])


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refused_argument_class_leaves_the_outputs_untouched():
    lib = _lib.load_library()
    n, R, K, seed = cc.HOST_SHAPES[0]
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    cap, F, T = dets.shape[1], len(X), cc.T_ANGLES
    th = cc.THETAS.copy()
    rows, vel = cc.tables(R, K)
    outs = [np.full((F, cap), 7, np.int32), np.full((F, cap), 7.0), np.full((F, cap, K), 7.0), np.full((F, cap, 4), 7.0)]
    good = dict(X=X.ctypes.data, dets=dets.ctypes.data, counts=counts.ctypes.data, th=dptr(th), dop=outs[0].ctypes.data,
                peak=outs[1].ctypes.data, spec=outs[2].ctypes.data, pts=outs[3].ctypes.data, rows=rows.ctypes.data,
                vel=vel.ctypes.data, F=F, n=n, R=R, K=K, T=T, cap=cap, delta=cc.DELTA, win=1)
    bad_th = th.copy()
    bad_th[5] = np.inf
    nan_th = th.copy()
    nan_th[0] = np.nan
    refusals = [dict(X=None), dict(dets=None), dict(counts=None), dict(th=None), dict(dop=None), dict(peak=None), dict(rows=None),
                dict(vel=None), dict(n=0), dict(n=17), dict(n=-1), dict(K=0), dict(K=513), dict(R=0), dict(R=-1), dict(T=0),
                dict(cap=0), dict(cap=-5), dict(F=-1), dict(delta=-1e-9), dict(delta=float("nan")), dict(delta=float("inf")),
                dict(th=dptr(bad_th)), dict(th=dptr(nan_th))]
    for change in refusals:
        a = dict(good, **change)
        rc = lib.mmw_diag_capon_doppler_host(*a.values())
        assert rc == _lib.MMW_ERR_INVALID and lib.mmw_last_error(), change
        # the device entry judges the same arguments before it touches its context: a null context is refused too, nothing runs
        assert lib.mmw_capon_doppler(None, *a.values()) == _lib.MMW_ERR_INVALID
        for o in outs:
            assert np.all(o == 7), change
    assert lib.mmw_diag_capon_doppler_host(*dict(good, F=0).values()) == _lib.MMW_OK
    assert all(np.all(o == 7) for o in outs)
    assert lib.mmw_diag_capon_doppler_host(*dict(good, spec=None, pts=None, rows=None, vel=None).values()) == _lib.MMW_OK


def test_capon_points_args_every_refusal():
    V, S, K = 12, 32, 16
    det = CaCFAR2D((2, 3), (1, 1), 1e-3)
    th, rx, window, delta, fpp, cfar, cap = capon_points_args(V, S, K, cc.THETAS, range(8), det, (2, 30), 1e-3, 4, 99)
    assert (rx, window, delta, fpp, cap) == (list(range(8)), (2, 30), 1e-3, 4, 99) and np.array_equal(th, cc.THETAS)
    assert cfar == (_lib.CFAR_CA, 2, 3, 1, 1, float(det._scale()), int(det._k_rank()))
    os_det = OsCFAR2D([2, 3], [1, 1], 0.7, 6.0)            # YAML lists are accepted as FramePipeline(cfar=...) accepts them
    assert capon_points_args(V, S, K, cc.THETAS, [0, 1], os_det)[5] == (_lib.CFAR_OS, 2, 3, 1, 1, float(os_det._scale()),
                                                                       int(os_det._k_rank()))

    class OwnThresholds(CaCFAR2D):
        def _compute_thresholds(self, X):
            return X, X

    class Duck:
        kind, num_train, num_guard = 0, (1, 1), (1, 1)

    for bad in (None, "ca_cfar_2d", CaCFAR1D(4, 2, 1e-3), OwnThresholds((2, 2), (1, 1), 1e-3), Duck()):
        with pytest.raises(ValueError, match="stock CaCFAR2D or OsCFAR2D"):
            capon_points_args(V, S, K, cc.THETAS, range(8), bad)
    for train, guard in (((2,), (1, 1)), ((2, 3), 1), ((2, -1), (1, 1)), ((2.5, 3), (1, 1)), ((2, 3), (1, "x"))):
        with pytest.raises(ValueError, match="pair of non-negative integers"):
            capon_points_args(V, S, K, cc.THETAS, range(8), CaCFAR2D(train, guard, 1e-3))
    for chirps in (0, 513):
        with pytest.raises(ValueError, match="chirps per frame"):
            capon_points_args(V, S, chirps, cc.THETAS, range(8), det)
    for capacity in (0, -1, 2.5):
        with pytest.raises(ValueError, match="det_capacity"):
            capon_points_args(V, S, K, cc.THETAS, range(8), det, det_capacity=capacity)
    # everything capon_cube_args refuses is refused here as well
    with pytest.raises(ValueError, match="thetas_rad"):
        capon_points_args(V, S, K, [], range(8), det)
    with pytest.raises(ValueError, match="not finite"):
        capon_points_args(V, S, K, [0.0, np.nan], range(8), det)
    with pytest.raises(ValueError, match="rx_antennas"):
        capon_points_args(V, S, K, cc.THETAS, range(17), det)
    with pytest.raises(IndexError):
        capon_points_args(V, S, K, cc.THETAS, [0, V], det)
    with pytest.raises(ValueError, match="range_bins"):
        capon_points_args(V, S, K, cc.THETAS, range(8), det, range_bins=(5, 5))
    with pytest.raises(ValueError, match="delta"):
        capon_points_args(V, S, K, cc.THETAS, range(8), det, delta=-1.0)
    with pytest.raises(ValueError, match="frames_per_pass"):
        capon_points_args(V, S, K, cc.THETAS, range(8), det, frames_per_pass=0)


# ------------------------------------------------------------------------------------------------ sanitizer
def test_host_twin_and_refusals_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/capon_doppler_sanitize.cpp, a program of its own that launches nothing: the host twin on exactly sized buffers at
    every shape extreme, and every class of refused argument of the device entry.  (No GPU sanitizer is involved; the kernels are
    launch stubs never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_capon_doppler.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(CSRC, "mmw_tu_capon_doppler.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "capon_doppler_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "capon_doppler_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
