"""Host side of the Doppler-azimuth peak pickers (no device): the entries in the header and the ctypes table, the shared rule
through ``mmw_diag_doppler_azimuth_peaks_host`` against ``DopplerAzimuthProcessor.detect_peaks_rows`` / ``detect_peak_zero_az`` on
crafted maps, the band of undecided comparisons, ``precise_ranges_from_zero_az``, the arguments ``doppler_azimuth_peaks`` refuses
before it touches a device, the join of the multi-device form, and the entries' argument checks under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dopaz_peaks_cases as K
from conftest import ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, precise_ranges_from_zero_az

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
TAIL = ["n_sets", "F", "n_rows", "A", "h_groups", "G", "h_m", "a_lo", "a_hi", "a_zero", "min_threshold_dB", "prominence_dB"]


@pytest.fixture(scope="module")
def proc():
    return K.make_proc()


def test_entries_are_declared_bound_and_export_the_band():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in (("mmw_doppler_azimuth_peaks", ["ctx", "d_maps"] + TAIL + ["d_row_peak", "d_zero"]),
                       ("mmw_diag_doppler_azimuth_peaks_host", ["h_maps"] + TAIL + ["h_row_peak", "h_zero"])):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/mmwgpu.h"
        assert [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")] == want
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == len(want)
    band = re.search(r"#define\s+MMW_DOPAZ_PEAK_BAND\s+(\S+)", text)
    assert band and float(band.group(1)) == _lib.DOPAZ_PEAK_BAND == 1e-10
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7
    make = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_dopaz_peaks\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_dopaz_peaks\.o:.*-ffp-contract=off", make, flags=re.M)


def test_rule_equals_the_host_pickers_on_crafted_maps_and_leaves_no_line_undecided(proc):
    """Every entry of every case equals what find_peaks decides in dB; the cap on undecided lines is zero."""
    cases = K.random_cases()
    assert {c.n_rows for c in cases} == {1, 2, 33, 70} and {c.a_hi - c.a_lo for c in cases} >= {1, 2, 3, 64}
    lines = peaks = 0
    for case in cases:
        row, zero = K.run_host_entry(case)
        want_row, want_zero = K.host_tables(proc, case)
        assert not np.any(row == K.UNDECIDED) and not np.any(zero == K.UNDECIDED), case.label
        assert np.array_equal(row, want_row), case.label
        assert np.array_equal(zero, want_zero), case.label
        lines += row.size + zero.size
        peaks += int(np.count_nonzero(row >= 0)) + int(np.count_nonzero(zero >= 0))
    print(f"{len(cases)} cases, {lines} lines, {peaks} peaks, 0 differences, 0 undecided")
    assert peaks > 2000                                                       # the maps do hold peaks to disagree about


def test_rows_behind_m_make_no_peak_and_do_not_lift_the_floor(proc):
    case = K.random_case(5, 33, width=40)
    m1 = int(case.m[1])
    assert 0 < m1 < 33 and np.all(case.maps[:, 1, m1:] >= 50.0) and case.maps[:, 1, :m1].max() < 50.0
    row, zero = K.run_host_entry(case)
    assert np.all(row[:, 1, m1:] == K.NONE) and np.all(zero[:, 1] < m1 - 1)   # row m - 1 is the end of the column: never a peak
    assert np.any(row[:, 1, :m1] >= 0)                                         # a floor from behind m would have swallowed these
    assert np.array_equal(row, K.host_tables(proc, case)[0])


def test_comparisons_inside_the_band_are_undecided_and_outside_equal_the_host(proc):
    """Each kind of comparison -- neighbour / neighbour, cell / floor, peak / base x ratio, candidate / candidate -- a quarter of
    the band and four bands apart, above and below; the second map of the pair supplies the offset."""
    for case, notes in K.band_cases(0.25):
        row, zero = K.run_host_entry(case)
        for f, (kind, rows, in_zero) in enumerate(notes):
            for r in rows:
                assert row[0, f, r] == K.UNDECIDED, (kind, f, r, row[0, f])
            if in_zero:
                assert zero[0, f] == K.UNDECIDED, (kind, f)
    seen = set()
    for case, notes in K.band_cases(4.0):
        row, zero = K.run_host_entry(case)
        want_row, want_zero = K.host_tables(proc, case)
        assert not np.any(row == K.UNDECIDED) and not np.any(zero == K.UNDECIDED), case.label
        assert np.array_equal(row, want_row) and np.array_equal(zero, want_zero), case.label
        for f, (kind, rows, in_zero) in enumerate(notes):
            seen.add((kind, tuple(int(row[0, f, r]) for r in rows), int(zero[0, f]) if in_zero else None))
    # above and below the comparison the decision differs: the placement does steer it
    for kind in ("neighbour", "floor", "prominence", "candidate"):
        assert len({s for s in seen if s[0] == kind}) == 2, (kind, seen)


def test_a_frame_with_a_nan_or_an_inf_is_undecided_throughout(proc):
    case = K.nonfinite_case()
    row, zero = K.run_host_entry(case)
    m = case.m
    # groups: (0, 1), (2,), (1,).  Frame 0: NaN in set 0; frame 1: Inf in set 1; frame 2: only behind m / outside the columns
    for g, f, bad in ((0, 0, True), (1, 0, False), (2, 0, False), (0, 1, True), (1, 1, False), (2, 1, True),
                      (0, 2, False), (1, 2, False), (2, 2, False)):
        if bad:
            assert np.all(row[g, f, :m[f]] == K.UNDECIDED) and np.all(row[g, f, m[f]:] == K.NONE) and zero[g, f] == K.UNDECIDED
        else:
            want_row, want_zero = K.host_pickers(proc, case, g, f)
            assert np.array_equal(row[g, f], want_row) and zero[g, f] == want_zero, (g, f)


def test_zero_threshold_and_zero_prominence_are_decided(proc):
    """Ratios of exactly 1: the floor is the frame maximum (everything is floored: no peak anywhere), and a prominence of 0 dB
    takes every local maximum -- bit-equal operands are decided there."""
    case = K.random_case(11, 9, width=30, thr=0.0)
    row, zero = K.run_host_entry(case)
    assert np.all(row == K.NONE) and np.all(zero == K.NONE)
    assert np.array_equal(row, K.host_tables(proc, case)[0])
    case = K.random_case(12, 9, width=30)
    row, _ = K.run_host_entry(case, prominence_dB=0.0)
    assert not np.any(row == K.UNDECIDED) and np.count_nonzero(row >= 0) >= np.count_nonzero(K.run_host_entry(case)[0] >= 0)


def _peak(v):
    return np.array([0.0, v])


def test_precise_ranges_follow_the_four_branches_of_estimate_ego_vx_velocity():
    none = np.empty(shape=(0, 2))
    az = [_peak(0.4), _peak(-0.3), none, none, _peak(0.1)]
    el = [_peak(0.2), none, _peak(0.7), none, _peak(-0.1)]
    bound = 0.25
    got = precise_ranges_from_zero_az(az, el, bound)
    assert got.shape == (5, 2) and got.dtype == np.float64
    for f in range(5):                                     # velocity_estimator.py:640-661, then :163-166 around -1 * ego_vx
        if az[f].shape[0] > 0 and el[f].shape[0] > 0:
            ego = -1 * (az[f][1] + el[f][1]) / 2.0
        elif az[f].shape[0] > 0:
            ego = -1 * az[f][1]
        elif el[f].shape[0] > 0:
            ego = -1 * el[f][1]
        else:
            ego = 0.0
        centre = -1 * ego
        assert np.array_equal(got[f], np.array([centre - bound, centre + bound])), f
    only_az = precise_ranges_from_zero_az(az, None, 0.5)
    assert np.array_equal(only_az[:, 0], np.array([0.4, -0.3, 0.0, 0.0, 0.1]) - 0.5)
    assert precise_ranges_from_zero_az([], [], 0.25).shape == (0, 2)
    with pytest.raises(ValueError):
        precise_ranges_from_zero_az(az, el[:3])


def bare_pipeline(n_frames=3, shape=(12, 63, 70)):
    """A FramePipeline without a device behind it: enough for the checks that come before any buffer is touched."""
    p = FramePipeline.__new__(FramePipeline)
    p.n_frames = n_frames
    p.V, p.S, p.C = shape
    return p


def test_doppler_azimuth_peaks_refuses_bad_arguments_before_any_device_use(proc):
    p = bare_pipeline()
    sets, win = [[0, 3, 4, 7], [1, 2, 5, 6], [0, 1, 2, 3]], [0.9, 2.0]
    shifts = [True, True, False]
    for method in (p.doppler_azimuth_peaks, p.doppler_azimuth_peaks_device):
        with pytest.raises(ValueError, match="outside the 3"):
            method(proc, sets, [(0, 3)], win, shifts)
        with pytest.raises(ValueError, match="outside the 3"):
            method(proc, sets, [-1], win, shifts)
        with pytest.raises(ValueError, match="twice"):
            method(proc, sets, [(1, 1)], win, shifts)
        with pytest.raises(ValueError, match="one set or two"):
            method(proc, sets, [(0, 1, 2)], win, shifts)
        with pytest.raises(ValueError, match="share shift_angle"):
            method(proc, sets, [(0, 1), (1, 2)], win, shifts)
        with pytest.raises(ValueError, match="shift_angle"):
            method(proc, sets, [(0, 1)], win, [True, False])
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="min_threshold_dB"):
                method(proc, sets, [(0, 1)], win, shifts, min_threshold_dB=bad)
        with pytest.raises(ValueError, match="DopplerAzimuthProcessor"):
            method(object(), sets, [(0, 1)], win, shifts)
        with pytest.raises(ValueError, match="range_windows"):
            method(proc, sets, [(0, 1)], np.zeros((2, 2)), shifts)              # 3 frames are resident
        with pytest.raises(ValueError, match="precise_vel_ranges"):
            method(proc, sets, [(0, 1)], win, shifts, precise_vel_ranges=np.zeros((4, 2)))
        with pytest.raises(ValueError, match="repeats"):
            method(proc, [[0, 3, 3, 7]], [0], win)
        with pytest.raises(ValueError, match="num_angle_bins == 64"):
            method(K.make_proc(num_angle_bins=32), sets, [(0, 1)], win, shifts)
        gap = K.make_proc()
        gap.valid_angle_mask = gap.valid_angle_mask.copy()
        gap.valid_angle_mask[30] = False
        with pytest.raises(ValueError, match="one non-empty run"):
            method(gap, sets, [(0, 1)], win, shifts)
    assert not hasattr(p, "ctx") and not hasattr(p, "bufs") and not hasattr(p, "n_peaks_undecided")


class _FakePart:
    """Host-only stand-in for a per-device FramePipeline: per group and frame, one row peak (global frame, device) and a zero
    peak at the frame's window end; odd global frames count as undecided."""

    def __init__(self, device):
        self.device = device
        self.frames = np.empty(0)

    def load(self, cubes):
        self.frames = cubes[:, 0, 0, 0].real.copy()

    def doppler_azimuth_peaks(self, proc, rx_sets, groups, range_windows, shift_angle=True, precise_vel_ranges=None,
                              min_threshold_dB=30.0):
        n = len(self.frames)
        assert range_windows.shape == (n, 2) and (precise_vel_ranges is None or precise_vel_ranges.shape == (n, 2))
        rows = [[np.array([[self.frames[f] + 100 * g, self.device]]) for f in range(n)] for g in range(len(groups))]
        zero = [[np.array([0.0, range_windows[f, 1]]) for f in range(n)] for g in range(len(groups))]
        self.n_peaks_undecided = int(np.count_nonzero(self.frames % 2))
        return rows, zero


@pytest.mark.parametrize("world,n_frames", [(1, 5), (2, 7), (4, 10), (8, 3)])
def test_multi_device_peaks_come_back_in_frame_order(world, n_frames):
    shape = (2, 2, 4)
    mp = MultiDeviceFramePipeline(None, max_frames=16, shape=shape, devices=list(range(world)), part_factory=lambda d, n: _FakePart(d))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    wins = np.stack([np.zeros(n_frames), 10.0 + np.arange(n_frames)], axis=1)
    rows, zero = mp.doppler_azimuth_peaks(None, [[0], [1]], [(0, 1), 1], wins)
    assert len(rows) == len(zero) == 2 and all(len(x) == n_frames for x in rows + zero)
    owners = [f * world // n_frames for f in range(n_frames)]
    for g in range(2):
        assert [int(rows[g][f][0, 0]) for f in range(n_frames)] == [f + 100 * g for f in range(n_frames)]
        assert [int(rows[g][f][0, 1]) for f in range(n_frames)] == owners
        assert [zero[g][f][1] for f in range(n_frames)] == wins[:, 1].tolist()     # each shard got ITS rows of the table
    assert mp.n_peaks_undecided == n_frames // 2
    mp.close()


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/doppler_azimuth_peaks_sanitize.cpp, a program of its own that launches nothing: every class of refused argument with
    the outputs left untouched, F == 0 and G == 0, through both entries, and the shared rule on small maps through the host-only
    one.  (No GPU sanitizer is involved; the kernel is a launch stub that is never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_dopaz_peaks.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_dopaz_peaks.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "doppler_azimuth_peaks_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "doppler_azimuth_peaks_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
