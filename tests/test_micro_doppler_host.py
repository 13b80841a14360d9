"""Host side of the micro-Doppler path (no device): the new C entry in the header and the ctypes table, the processor's bin tables
and window against the reference's expressions on every shipped cfg, the fftshift index formula, the roll of the spectrogram
(``MicroDopplerProcessor.push`` and ``batch.micro_doppler_history``) against the reference-generated fixture, the join order of
the multi-device form, and the entry's argument checks under AddressSanitizer + UndefinedBehaviorSanitizer."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import MultiDeviceFramePipeline, micro_doppler_history, shard_bounds
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import MicroDopplerProcessor
from mmwave_radar_processing_amd.processors.micro_doppler_resp import shifted_bin, window_rows

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")


class GridConfig:
    """The five scalars the processor reads, chosen so that S range bins sit at 0, 1, ... and C velocity bins 1 apart."""

    def __init__(self, S, C, period_ms=50.0):
        self.range_res_m, self.range_max_m = 1.0, float(S)
        self.vel_res_m_s, self.vel_max_m_s = 1.0, C / 2
        self.frameCfg_periodicity_ms = period_ms


def shipped_cfgs():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        return json.load(fh)


def test_entry_is_declared_bound_and_leaves_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+mmw_micro_doppler\s*\(([^)]*)\)\s*;", text)
    assert m, "mmw_micro_doppler is not declared in include/mmwgpu.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "d_cubes", "d_out", "n_frames", "V", "S", "C", "rx_idx", "row_lo",
                                                           "row_hi"]
    assert "mmw_micro_doppler" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_micro_doppler"]) == 10
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7


@pytest.mark.parametrize("target_ranges", [[0, 1.0], [0.5, 2.0]])
def test_bin_tables_and_window_equal_the_reference_expressions_on_every_shipped_cfg(target_ranges):
    table = shipped_cfgs()
    assert len(table) == 26
    for name, ent in table.items():
        cm = ConfigManager()
        cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
        H = 20
        p = MicroDopplerProcessor(cm, target_ranges=target_ranges, num_frames_history=H)
        # the reference's expressions (processors/micro_doppler_resp.py:59-87), on the same scalars
        vel = np.arange(start=-1 * cm.vel_max_m_s, stop=cm.vel_max_m_s - cm.vel_res_m_s + 1e-3, step=cm.vel_res_m_s)
        rng = np.arange(start=0, step=cm.range_res_m, stop=cm.range_max_m - cm.range_res_m / 2 + 1e-3)
        keep = np.logical_and(rng >= target_ranges[0], rng <= target_ranges[1]).astype(np.bool_)
        frame_period = cm.frameCfg_periodicity_ms * 1e-3
        t = np.linspace(start=0, stop=H * frame_period, num=H)
        for got, want in ((p.vel_bins, vel), (p.range_bins, rng), (p.range_bin_idxs_to_keep, keep), (p.time_bins, t)):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
        rows = np.flatnonzero(keep)
        assert p.rows == (rows[0], rows[-1]) and np.array_equal(rows, np.arange(rows[0], rows[-1] + 1)), name
        assert isinstance(p.target_ranges, np.ndarray) and p.num_frames_history == H
        assert p.micro_doppler_resp.shape == (len(vel), H) and p.micro_doppler_resp.dtype == np.float64
        assert not p.micro_doppler_resp.any()
        assert len(vel) == ent["expect"]["loops"], name


def test_fixture_tables_are_the_reference_arrays_bit_for_bit(golden):
    g = golden("micro_doppler.npz")
    ent = shipped_cfgs()[str(g["cfg"])]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    assert [cm.vel_max_m_s, cm.vel_res_m_s, cm.range_res_m, cm.range_max_m, cm.frameCfg_periodicity_ms] == g["scalars"].tolist()
    p = MicroDopplerProcessor(cm, target_ranges=g["target_ranges"].tolist(), num_frames_history=int(g["num_frames_history"]))
    for got, key in ((p.vel_bins, "vel_bins"), (p.range_bins, "range_bins"), (p.time_bins, "time_bins"),
                     (p.range_bin_idxs_to_keep, "mask")):
        assert got.dtype == g[key].dtype and np.array_equal(got, g[key]), key
    assert list(p.rows) == g["rows"].tolist()


def test_a_window_between_two_bins_is_refused_at_configure():
    for name, ent in shipped_cfgs().items():
        cm = ConfigManager()
        cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
        res = cm.range_res_m
        with pytest.raises(ValueError, match="no range bin"):
            MicroDopplerProcessor(cm, target_ranges=[2.3 * res, 2.7 * res])
    with pytest.raises(ValueError, match="no range bin"):
        MicroDopplerProcessor(GridConfig(16, 8), target_ranges=[5.0, 3.0])       # reversed
    with pytest.raises(ValueError, match="no range bin"):
        window_rows(np.arange(16.0), (16.5, 40.0))                                # past the last bin
    mask, lo, hi = window_rows(np.arange(16.0), (3.0, 3.0))                       # both ends on one bin: that row
    assert (lo, hi) == (3, 3) and mask.sum() == 1


@pytest.mark.parametrize("C", [1, 2, 23, 32, 127])
def test_shifted_index_formula_is_numpy_fftshift(C):
    bins = np.arange(C)
    assert np.array_equal(np.fft.fftshift(bins), shifted_bin(bins, C))
    assert np.array_equal(np.fft.fftshift(bins), [(c + C - C // 2) % C for c in range(C)])
    # the kernel stores FFT bin k at column (k + C/2) mod C: the inverse permutation
    col = (bins + C // 2) % C
    assert np.array_equal(shifted_bin(col, C), bins)


def test_push_and_history_roll_newest_first():
    C, H = 6, 4
    p = MicroDopplerProcessor(GridConfig(16, C), target_ranges=[0, 3], num_frames_history=H)
    rows = np.arange(1, 8)[:, None] * 10.0 + np.arange(C)[None, :]             # frame n holds 10 (n + 1) + c
    assert not micro_doppler_history(rows[:0], H).any() and micro_doppler_history(rows[:0], H).shape == (C, H)
    for n in range(len(rows)):
        out = p.push(rows[n])
        assert out is p.micro_doppler_resp and out.shape == (C, H) and out.dtype == np.float64
        assert np.array_equal(out[:, 0], rows[n])                               # newest first
        for age in range(H):
            want = rows[n - age] if n - age >= 0 else np.zeros(C)               # zeros beyond the frames seen, H frames kept
            assert np.array_equal(out[:, age], want), (n, age)
        assert np.array_equal(micro_doppler_history(rows[:n + 1], H), out)
    p.reset()
    assert p.micro_doppler_resp.shape == (C, H) and not p.micro_doppler_resp.any()
    assert p.history_estimated == [] and p.history_gt == []
    assert np.array_equal(p.push(rows[2]), micro_doppler_history(rows[2:3], H))
    with pytest.raises(ValueError):
        p.push(np.zeros(C + 1))
    with pytest.raises(ValueError):
        micro_doppler_history(np.zeros(C), H)
    # concatenated stream() chunks are one sequence
    assert np.array_equal(micro_doppler_history(np.concatenate([rows[:3], rows[3:]]), H), micro_doppler_history(rows, H))
    assert micro_doppler_history(rows, 0).shape == (C, 0)


def test_fixture_buffers_are_the_history_of_the_fixture_rows(golden):
    g = golden("micro_doppler.npz")
    H = int(g["num_frames_history"])
    rows, buffers = g["out_rows"], g["buffers"]
    assert rows.shape[1] > H                                                   # the oldest row has left the buffer at the end
    for i in range(len(g["rx"])):
        p = MicroDopplerProcessor(GridConfig(g["cubes"].shape[2], rows.shape[2]), target_ranges=[0, 1], num_frames_history=H)
        for f in range(rows.shape[1]):
            assert np.array_equal(micro_doppler_history(rows[i, :f + 1], H), buffers[i, f])
            assert np.array_equal(p.push(rows[i, f]), buffers[i, f])
    # the recorded rows are the inline definition, on the recorded complex64 cubes
    lo, hi = g["rows"]
    for i, rx in enumerate(g["rx"]):
        for f, cube in enumerate(g["cubes"]):
            want = np.abs(np.fft.fftshift(np.fft.fft2(cube[rx]), axes=1))[lo:hi + 1].max(0)
            assert np.array_equal(want, rows[i, f])


def test_process_refuses_a_cube_of_another_shape_before_any_device_call():
    p = MicroDopplerProcessor(GridConfig(16, 8), target_ranges=[0, 3])
    for shape in ((2, 15, 8), (2, 16, 9)):
        with pytest.raises(ValueError, match="does not match"):
            p.process(np.zeros(shape, dtype=np.complex64))
    with pytest.raises(IndexError):
        p.process(np.zeros((2, 16, 8), dtype=np.complex64), rx_idx=2)
    assert p._ctx is None and not p.micro_doppler_resp.any()


class _FakePart:
    """Host-only stand-in for a per-device FramePipeline: row f of its micro_doppler() is [global frame, device, rx, window]."""

    def __init__(self, device, max_frames, shape):
        self.device, self.max_frames, self.shape = device, max_frames, shape
        self.frames = np.empty(0)

    def load(self, cubes):
        self.frames = cubes[:, 0, 0, 0].real.copy()

    def micro_doppler(self, target_ranges, rx_idx):
        out = np.zeros((len(self.frames), self.shape[2]))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = self.frames, self.device, rx_idx, target_ranges[1]
        return out


@pytest.mark.parametrize("world,n_frames", [(1, 5), (2, 7), (4, 10), (8, 3), (3, 0)])
def test_multi_device_rows_come_back_in_frame_order(world, n_frames):
    shape = (2, 2, 4)
    mp = MultiDeviceFramePipeline(None, max_frames=16, shape=shape, devices=list(range(world)),
                                  part_factory=lambda d, n: _FakePart(d, n, shape))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    assert mp.bounds == [shard_bounds(n_frames, r, world) for r in range(world)]
    rows = mp.micro_doppler(target_ranges=(0, 2.5), rx_idx=1)
    assert rows.shape == (n_frames, shape[2]) and rows.dtype == np.float64
    assert rows[:, 0].tolist() == list(range(n_frames))                                       # frame order
    assert rows[:, 1].tolist() == [f * world // n_frames for f in range(n_frames)]            # owner = floor(f W / F)
    assert np.all(rows[:, 2] == 1) and np.all(rows[:, 3] == 2.5)
    mp.close()


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/micro_doppler_sanitize.cpp, a program of its own that launches nothing: every class of refused argument and
    n_frames == 0 through mmw_micro_doppler.  (No GPU sanitizer is involved; the kernels are launch stubs that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=fast", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_micro_doppler.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_micro_doppler.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "micro_doppler_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "micro_doppler_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
