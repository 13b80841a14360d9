"""Host side of the batched synthetic-array beamformer (no device): the C entry in the header and the ctypes table, the processor's
tables against the reference's expressions on every shipped cfg, the velocity gate and the backward pose accumulation against the
reference-generated fixture (stepped class and ``batch.synthetic_array_geometry``), the gate's edges one at a time, the window
arithmetic of ``mmw_synth_array.h`` against brute force, and the entry's argument checks under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, synthetic_array_geometry
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import SyntheticArrayBeamformerProcessor
from mmwave_radar_processing_amd.processors.synthetic_array_beamformer import gate, window_geometry

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")


def shipped_cfgs():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        return json.load(fh)


def config(name):
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(shipped_cfgs()[name]["lines"]) + "\n")
    return cm


def fixture_processor(g, **over):
    rx, cfg_idx, H, stride = (int(x) for x in g["params"])
    kw = dict(receiver_idx=rx, chirp_cfg_idx=cfg_idx, num_frames=H, stride=stride, az_angle_bins_rad=g["az_rad"].tolist(),
              el_angle_bins_rad=g["el_rad"], min_vel=g["min_vel"].tolist(), max_vel=g["max_vel"], max_vel_stdev=g["max_vel_stdev"],
              some_gui_parameter=3)
    kw.update(over)
    return SyntheticArrayBeamformerProcessor(config(str(g["cfg"])), **kw)


def test_entry_is_declared_bound_and_leaves_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+mmw_synth_array\s*\(([^)]*)\)\s*;", text)
    assert m, "mmw_synth_array is not declared in include/mmwgpu.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "d_cubes", "n_resident", "V", "S", "C", "v", "k", "H", "h_frames",
                                                           "n_out", "h_P", "h_dirs", "T", "lambda_m", "d_out"]
    assert "mmw_synth_array" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_synth_array"]) == len(params)
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7


@pytest.mark.parametrize("pick,stride", [(0, 1), (-1, 3)])
def test_tables_equal_the_reference_expressions_on_every_shipped_cfg(pick, stride):
    table = shipped_cfgs()
    assert len(table) == 26
    for name in table:
        cm = config(name)
        cfgs = np.arange(start=cm.frameCfg_start_index, stop=cm.frameCfg_end_index + 1)
        chirp_cfg_idx = int(cfgs[pick])
        az, el = np.deg2rad(np.linspace(-20, 20, 5)), np.deg2rad(np.array([0.0, 5.0]))
        p = SyntheticArrayBeamformerProcessor(cm, receiver_idx=0, chirp_cfg_idx=chirp_cfg_idx, num_frames=2, stride=stride,
                                              az_angle_bins_rad=az, el_angle_bins_rad=el)
        # the reference's expressions (simple_synthetic_array_beamformer_processor_multiFrame.py:175-246, 474-488)
        chirps_per_frame = cm.frameCfg_loops * (cm.frameCfg_end_index - cm.frameCfg_start_index + 1)
        idxs = np.tile(A=cfgs, reps=cm.frameCfg_loops).flatten()
        mask0 = (idxs == chirp_cfg_idx)
        mask = np.zeros_like(mask0, dtype=bool)
        mask[np.where(mask0)[0][::stride]] = True
        period_us = cm.profile_cfgs[0]["idleTime_us"] + cm.profile_cfgs[0]["rampEndTime_us"]
        times = (np.arange(start=chirps_per_frame - 1, stop=-1, step=-1) * -period_us)[mask]
        lam = 299792458.0 / (float(cm.profile_cfgs[0]["startFreq_GHz"]) * 1e9)
        thetas, phis = np.meshgrid(az, el, indexing="ij")
        d = np.array([np.cos(thetas) * np.cos(phis), np.sin(thetas) * np.cos(phis), np.sin(phis)])
        for got, want in ((p.valid_chirps_mask, mask), (p.chirp_start_times_us, times), (p.d, d)):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
        assert p.lambda_m == lam and p.chirps_per_frame == chirps_per_frame, name
        Cv = -(-cm.frameCfg_loops // stride)
        assert mask.sum() == Cv and p.history_acd_cube_valid_chirps.shape == (2, cm.get_num_adc_samples(profile_idx=0), Cv)
        assert p.history_acd_cube_valid_chirps.dtype == np.complex128 and p.history_avg_vel.shape == (2, 3)
        assert np.array_equal(p.range_bins, np.linspace(start=0, stop=cm.range_max_m, num=p.num_range_bins))
        assert p.array_geometry.shape == (0,) and p.array_geometry_valid is False and p.beamformed_resp is None


def test_calibration_is_refused():
    with pytest.raises(NotImplementedError):
        SyntheticArrayBeamformerProcessor(config("6843_RadVel_ods_10Hz.cfg"), enable_calibration=True)


def test_stepped_class_reproduces_the_fixture_flags_and_geometry(golden, monkeypatch):
    g = golden("synth_array.npz")
    p = fixture_processor(g)
    assert np.array_equal(p.valid_chirps_mask, g["valid_chirps_mask"]) and np.array_equal(p.chirp_start_times_us, g["chirp_start_times_us"])
    assert np.array_equal(p.d, g["d"]) and p.lambda_m == float(g["lambda_m"])
    assert np.flatnonzero(p.valid_chirps_mask)[:3].tolist() == [2, 11, 20]
    calls = []
    monkeypatch.setattr(p._core, "contract", lambda X, P: calls.append((X.copy(), P.copy())) or np.zeros((X.shape[0], 7, 2), complex))
    S, L = g["slabs"].shape[2:]
    worst = 0.0
    for f, vel in enumerate(g["velocities"]):
        raw = np.zeros((4, S, 3 * L), dtype=np.complex64)
        raw[1, :, 2::3] = g["slabs"][f, 0]                  # receiver 1, transmitter 2: virtual antenna 9
        raw[1, :, 1::3] = g["slabs"][f, 1]                  # the decoy (virtual antenna 5)
        out = p.process(raw, vel.tolist())
        assert p.array_geometry_valid == bool(g["valid"][f]) and (out.size > 0) == bool(g["valid"][f]), f
        worst = max(worst, np.abs(p.array_geometry - g["array_geometry"][f]).max())
        assert np.array_equal(p.history_acd_cube_valid_chirps[-1], g["slabs"][f, 0][:, ::3])
    print(f"geometry: worst deviation {worst:.3g} m")
    assert worst <= 1e-15
    assert np.flatnonzero(g["valid"]).tolist() == g["frames"].tolist() == [2, 3, 7] and len(calls) == 3
    # what the contraction is handed: the window stacked oldest first, [S, E] and [3, E]
    X, P = calls[-1]
    assert X.shape == (S, 102) and P.shape == (3, 102)
    assert np.array_equal(X[:, 68:], g["slabs"][7, 0][:, ::3]) and np.array_equal(X[:, :34], g["slabs"][5, 0][:, ::3])
    assert np.array_equal(P, p.array_geometry.transpose(1, 0, 2).reshape(3, -1))
    p.reset()
    assert not p.history_avg_vel.any() and not p.history_acd_cube_valid_chirps.any() and p.array_geometry_valid is False


def test_geometry_scan_equals_the_fixture_and_leaves_the_processor_alone(golden):
    g = golden("synth_array.npz")
    p = fixture_processor(g)
    p.history_avg_vel[:] = 7.0                              # state the scan must neither read nor write
    before = (p.history_avg_vel.copy(), p.history_acd_cube_valid_chirps.copy(), p.array_geometry.copy(), p.array_geometry_valid)
    valid, P = synthetic_array_geometry(p, g["velocities"])
    assert valid.dtype == np.bool_ and np.array_equal(valid, g["valid"])
    assert P.dtype == np.float64 and P.shape == (3, 3, 102)
    want = g["array_geometry"][g["frames"]].transpose(0, 2, 1, 3).reshape(3, 3, 102)
    assert np.abs(P - want).max() <= 1e-15
    assert np.array_equal(p.history_avg_vel, before[0]) and np.array_equal(p.history_acd_cube_valid_chirps, before[1])
    assert np.array_equal(p.array_geometry, before[2]) and p.array_geometry_valid is before[3]
    valid0, P0 = synthetic_array_geometry(p, np.zeros((0, 3)))
    assert valid0.shape == (0,) and P0.shape == (0, 3, 102)
    with pytest.raises(ValueError):
        synthetic_array_geometry(p, np.zeros((4, 2)))


def test_gate_edges_each_flipped_alone():
    lo, hi, sd = np.array([0.17, 0.0, 0.0]), np.array([0.25, 0.05, 0.05]), np.array([0.1, 0.1, 0.1])
    good = np.array([[.2, .01, 0], [.21, 0, .01], [.2, 0, 0]])
    assert gate(good, lo, hi, sd)
    for row, col, val in ((0, 0, 0.16), (2, 0, 0.26), (1, 1, 0.06), (1, 2, -0.06)):       # one entry outside [min, max]
        bad = good.copy()
        bad[row, col] = val
        assert not gate(bad, lo, hi, sd), (row, col, val)
    edge = good.copy()
    edge[0, 0], edge[2, 0] = 0.17, 0.25                     # the bounds themselves are inside
    assert gate(edge, lo, hi, sd)
    # the spread: just over / exactly on the bound, everything else wide open
    wide_lo, wide_hi = np.zeros(3), np.full(3, 10.0)
    pair = np.array([[1.0, 0, 0], [1.5, 0, 0]])             # std of the x column: 0.25 exactly
    assert gate(pair, wide_lo, wide_hi, np.array([0.25, 0.1, 0.1]))
    assert not gate(pair, wide_lo, wide_hi, np.array([np.nextafter(0.25, 0), 0.1, 0.1]))
    # a reversed direction: |v| and the spread pass (|.| is taken per component), the cosine is -1
    rev = np.array([[.2, 0, 0], [-.2, 0, 0]])
    assert gate(np.abs(rev), lo, hi, np.full(3, 1.0)) and not gate(rev, lo, hi, np.full(3, 1.0))
    # 18.2 degrees apart: cosine just below 0.95
    a = np.deg2rad(18.3)
    assert not gate(np.array([[1.0, 0, 0], [np.cos(a), np.sin(a), 0]]), wide_lo, wide_hi, np.full(3, 1.0))
    a = np.deg2rad(18.0)
    assert gate(np.array([[1.0, 0, 0], [np.cos(a), np.sin(a), 0]]), wide_lo, wide_hi, np.full(3, 1.0))


def test_min_vel_zero_opens_the_gate_on_a_zero_history(golden):
    g = golden("synth_array.npz")
    p = fixture_processor(g, min_vel=[0.0, 0.0, 0.0])
    vel = np.array([[.2, .01, 0]] * 4)
    valid, P = synthetic_array_geometry(p, vel)
    # zero rows have direction 0 (the +1e-6 keeps the division finite), so their cosines are 0: the gate stays shut until the
    # history holds no zero row -- with min_vel = 0 it is the direction test alone that shuts it
    assert valid.tolist() == [False, False, True, True]
    still = np.zeros((3, 3))
    assert not gate(still, np.zeros(3), p.max_vel, p.max_vel_stdev)
    # one frame of history: a single non-zero velocity is its own direction
    p1 = fixture_processor(g, min_vel=[0.0, 0.0, 0.0], num_frames=1)
    valid1, P1 = synthetic_array_geometry(p1, vel)
    assert valid1.all() and P1.shape == (4, 3, 34)
    assert np.array_equal(P1[0], window_geometry(vel[:1], p1.chirp_start_times_us, p1.frame_period_ms)[0])


def test_window_geometry_is_the_backward_accumulation():
    t = np.array([-300.0, -200.0, -100.0, 0.0])
    hist = np.array([[0.1, 0, 0], [0.2, 0.01, 0], [0.3, 0, -0.02]])
    P = window_geometry(hist, t, 100.0)
    assert P.shape == (3, 3, 4)
    start = np.array([0, 0, 0])
    for f in (2, 1, 0):                                      # the reference's loop, newest frame first, from the origin
        for axis in range(3):
            want = 2 * t * 1e-6 * hist[f][axis] + start[axis]
            assert np.abs(P[f, axis] - want).max() <= 1e-18
        start = start + 2 * hist[f] * (-1 * 100.0 * 1e-3)
    assert P[2, 0, -1] == 0.0 and np.all(np.diff(P[:, 0, :].ravel()) > 0)      # the aperture runs forward in time along x


# ---------------------------------------------------------------- the window arithmetic (mmw_synth_array.h)
def window_plan(lib, C, k, H, frame, e0, n, cap=16):
    segs = (ctypes.c_int * (4 * cap))()
    info = (ctypes.c_int * 4)()
    assert lib.mmw_diag_synth_array_window(C, k, H, frame, e0, n, segs, cap, info) == 0
    return [tuple(segs[4 * i:4 * i + 4]) for i in range(min(info[0], cap))], info[1], bool(info[2]), bool(info[3])


@pytest.mark.parametrize("k", [1, 3])
def test_window_segments_against_brute_force(k):
    lib = _lib.load_library()
    for C in (1, 7, 8, 16, 20, 21, 32, 34):
        Cv = -(-C // k)
        for H in (1, 2, 3, 4):
            E = H * Cv
            for n in (8, 16, 32):
                fast_brute = E % 32 == 0
                for frame in (0, 1, H - 1, H + 2):
                    for e0 in range(0, E, n):
                        segs, first, vec16, fast = window_plan(lib, C, k, H, frame, e0, n)
                        # brute force: element by element
                        elems = [(e // Cv, frame - H + 1 + e // Cv, e % Cv) for e in range(e0, min(e0 + n, E))]
                        want = []
                        for h, fr, j in elems:
                            if want and want[-1][0] == h:
                                want[-1][3] += 1
                            else:
                                want.append([h, fr, j, 1])
                        assert segs == [tuple(w) for w in want], (C, k, H, frame, e0, n)
                        live = [fr for _, fr, _ in elems if fr >= 0]
                        assert first == (live[0] if live else -1)
                        # 16-byte loads: every element pair of every row at an address that is a multiple of 16 bytes, the
                        # run in one frame, unit stride
                        addr_ok = all((row * C + j * k) % 2 == 0 for row in range(3) for _, _, j in elems[::2])
                        contiguous = k == 1 and len(want) == 1 and len(elems) % 2 == 0
                        assert vec16 == (contiguous and addr_ok), (C, k, H, frame, e0, n)
                        fast_brute = fast_brute and vec16 and len(elems) == n
                    assert fast == fast_brute, (C, k, H, n)
    # the case the old "whole chunks" rule got wrong: E = 32, but a lane's run of 16 crosses frames
    segs, first, vec16, fast = window_plan(lib, 8, 1, 4, 1, 0, 32)
    assert [s[1] for s in segs] == [-2, -1, 0, 1] and first == 0 and not vec16 and not fast
    assert lib.mmw_diag_synth_array_window(8, 0, 4, 1, 0, 32, (ctypes.c_int * 64)(), 16, (ctypes.c_int * 4)()) == _lib.MMW_ERR_INVALID


class _NoDevice:
    """Stands in for the context and the buffer set of a FramePipeline: any use is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"device touched ({name}) before the arguments were checked")


def test_pipeline_refuses_bad_arguments_before_any_device_use(golden):
    g = golden("synth_array.npz")
    p = fixture_processor(g)
    fp = FramePipeline.__new__(FramePipeline)
    fp.ctx = fp.bufs = fp.d_in = _NoDevice()
    fp.n_frames = 8
    for shape in ((12, 63, 99), (12, 64, 100), (8, 63, 100), (4, 63, 100)):
        fp.V, fp.S, fp.C = shape
        with pytest.raises(ValueError, match="do not match"):
            fp.synthetic_array(p, g["velocities"])
    fp.V, fp.S, fp.C = 12, 63, 100
    for vel in (g["velocities"][:7], np.zeros((8, 2)), np.zeros(8)):
        with pytest.raises(ValueError, match="velocities"):
            fp.synthetic_array(p, vel)
    p.enable_calibration = True
    with pytest.raises(ValueError, match="calibration"):
        fp.synthetic_array_device(p, g["velocities"])


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/synth_array_sanitize.cpp, a program of its own that launches nothing: every class of refused argument and n_out == 0
    through mmw_synth_array, and the window arithmetic over a sweep.  (No GPU sanitizer is involved; the kernels are launch stubs
    that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=fast", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_synth_array.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_synth_array.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "synth_array_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "synth_array_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
