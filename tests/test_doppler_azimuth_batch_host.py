"""Host side of the batched Doppler-azimuth maps (no device): the two new C entries in the header and the ctypes table, the per-frame
tables of ``batch.doppler_azimuth_tables`` against the processor's own expressions on every shipped cfg, the arguments
``FramePipeline.doppler_azimuth`` refuses before it touches a device, the join order of the multi-device form, and the entries'
argument checks under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, doppler_azimuth_tables, shard_bounds
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
COARSE = ["ctx", "d_cubes", "d_out", "n_frames", "V", "S", "C", "A", "h_rx", "n_sets", "n_rx", "h_set_flags", "h_rows", "flags"]
VEL_RANGES = [[-0.25, 0.25], [0.3, 1.2], [-0.05, 0.02], [-500.0, 500.0]]       # both halves, positive only, a NaN half, beyond vel_max


def shipped_cfgs():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        return json.load(fh)


def make_proc(ent, **kw):
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    return DopplerAzimuthProcessor(cm, **kw)


def test_entries_are_declared_bound_and_leave_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in (("mmw_doppler_azimuth_batch", COARSE), ("mmw_doppler_azimuth_zoom_batch", COARSE + ["n_used", "h_freq", "M"])):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/mmwgpu.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == want
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == len(want)
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7


def test_row_tables_equal_the_keep_expression_of_process_on_every_shipped_cfg():
    table = shipped_cfgs()
    assert len(table) == 26
    for name, ent in table.items():
        p = make_proc(ent)
        res, top = p.config_manager.range_res_m, p.config_manager.range_max_m
        wins = np.array([[3.2 * res, 9.7 * res],            # inside the range
                         [-1.0, 2.5 * res],                 # clipped at 0
                         [top - 3 * res, top + 5.0],        # clipped at range_max_m
                         [2.3 * res, 2.7 * res],            # between two bins: empty
                         [3.6 * res, 4.4 * res],            # a single bin
                         [0.0, top]])                       # what process takes for range_window=[]
        before = wins.copy()
        rows = doppler_azimuth_tables(p, wins)
        assert rows.dtype == np.int32 and rows.shape == (len(wins), 2) and np.array_equal(wins, before), name
        for f, rw in enumerate(wins):
            keep = np.where((p.range_bins >= rw[0]) & (p.range_bins <= rw[1]))[0]          # process, doppler_azimuth_resp.py
            if keep.size:
                assert tuple(rows[f]) == (keep[0], keep[-1] + 1), (name, f)
                assert np.array_equal(keep, np.arange(keep[0], keep[-1] + 1))
            else:
                assert rows[f, 0] == rows[f, 1] and 0 <= rows[f, 0] <= len(p.range_bins), (name, f)
        assert rows[3, 0] == rows[3, 1] and rows[4, 1] - rows[4, 0] == 1 and rows[1, 0] == 0, name
        assert rows[2, 1] == len(p.range_bins) and tuple(rows[5]) == (0, len(p.range_bins)), name
        assert np.array_equal(doppler_azimuth_tables(p, wins[0]), rows[:1])                  # one pair: one frame


def test_zoom_tables_equal_the_zoom_plan_of_every_frame_on_every_shipped_cfg():
    for name, ent in shipped_cfgs().items():
        p = make_proc(ent)
        sentinel = np.array([123.0])
        p.zoomed_vel_bins = sentinel
        res = p.config_manager.range_res_m
        wins = np.tile([0.0, 5 * res], (len(VEL_RANGES), 1))
        vrs = np.array(VEL_RANGES)
        before = vrs.copy()
        rows, freq, m, bins = doppler_azimuth_tables(p, wins, vrs)
        assert p.zoomed_vel_bins is sentinel and np.array_equal(vrs, before), name             # proc and the caller's arrays: only read
        assert rows.shape == (4, 2) and freq.dtype == np.float64 and freq.shape == (4, int(m.max())) and len(bins) == 4, name
        n = p.vel_bins.size
        for f, vr in enumerate(VEL_RANGES):
            q = make_proc(ent)
            want = q._zoom_plan(np.array(vr))
            assert m[f] == len(want) == len(bins[f]), (name, f)
            assert np.array_equal(freq[f, :m[f]], want, equal_nan=True), (name, f)
            assert np.array_equal(bins[f], q.zoomed_vel_bins), (name, f)
            assert np.all(np.isnan(freq[f, m[f]:])), (name, f)                                  # the padding
        assert m[0] == 2 * n and freq.shape[1] == 2 * n and m[3] == 2 * n, name
        if p.config_manager.vel_max_m_s > 0.3:
            assert m[1] == n and np.all(bins[1] > 0), name                                      # positive only: half of M
        # [-0.05, 0.02] is widened to 0.2 m/s at one end; a half that still spans less than the minimum is NaN
        assert np.array_equal(np.isnan(freq[2, :m[2]]), np.isnan(make_proc(ent)._zoom_plan(np.array(VEL_RANGES[2])))), name
    with pytest.raises(ValueError):
        doppler_azimuth_tables(p, wins, vrs[:2])
    with pytest.raises(ValueError):
        doppler_azimuth_tables(p, np.zeros((3, 3)))


def bare_pipeline(n_frames=3, shape=(12, 63, 70)):
    """A FramePipeline without a device behind it: enough for the checks that come before any buffer is touched."""
    p = FramePipeline.__new__(FramePipeline)
    p.n_frames = n_frames
    p.V, p.S, p.C = shape
    return p


def test_doppler_azimuth_refuses_bad_arguments_before_any_device_use():
    ent = shipped_cfgs()["6843_RadVel_ods_20Hz.cfg"]
    proc = make_proc(ent)
    assert len(proc.range_bins) == 63 and proc.vel_bins.size == 70
    p = bare_pipeline()
    sets, win = [[0, 3, 4, 7], [1, 2, 5, 6]], [0.9, 2.0]
    for method in (p.doppler_azimuth, p.doppler_azimuth_device):
        with pytest.raises(ValueError, match="DopplerAzimuthProcessor"):
            method(object(), sets, win)
        with pytest.raises(ValueError, match="range_windows"):
            method(proc, sets, np.zeros((2, 2)))                        # 3 frames are resident
        with pytest.raises(ValueError, match="range_windows"):
            method(proc, sets, np.zeros((3, 3)))
        with pytest.raises(ValueError, match="precise_vel_ranges"):
            method(proc, sets, win, precise_vel_ranges=np.zeros((4, 2)))
        with pytest.raises(ValueError, match="one length"):
            method(proc, [[0, 3, 4, 7], [1, 2, 5]], win)
        with pytest.raises(ValueError, match="outside the 12 antennas"):
            method(proc, [[0, 3, 4, 12]], win)
        with pytest.raises(ValueError, match="repeats"):
            method(proc, [[0, 3, 3, 7]], win)
        with pytest.raises(ValueError, match="at most 16"):
            bare_pipeline(shape=(20, 63, 70)).doppler_azimuth(proc, (), win)
        with pytest.raises(ValueError, match="shift_angle"):
            method(proc, sets, win, shift_angle=[True, False, True])
        with pytest.raises(ValueError, match="num_angle_bins == 64"):
            method(make_proc(ent, num_angle_bins=32), sets, win)
        with pytest.raises(ValueError, match="range bins"):
            bare_pipeline(shape=(12, 64, 70)).doppler_azimuth(proc, sets, win)
        with pytest.raises(ValueError, match="CZT defined for length 70"):
            bare_pipeline(shape=(12, 63, 69)).doppler_azimuth(proc, sets, win, precise_vel_ranges=[-0.25, 0.25])
    assert not hasattr(p, "ctx") and not hasattr(p, "bufs") and proc.zoomed_vel_bins is None


class _FakePart:
    """Host-only stand-in for a per-device FramePipeline: its doppler_azimuth() writes, per frame, the global frame number, the
    device, the frame's window end and (precise) its velocity range start, with m_f = 2 + (global frame % 2) * ``ragged`` bins."""

    def __init__(self, device, max_frames, shape, ragged):
        self.device, self.max_frames, self.shape, self.ragged = device, max_frames, shape, ragged
        self.frames = np.empty(0)

    def load(self, cubes):
        self.frames = cubes[:, 0, 0, 0].real.copy()

    def doppler_azimuth(self, proc, rx_sets, range_windows, shift_angle=True, precise_vel_ranges=None):
        n, k = len(self.frames), len(rx_sets)
        assert range_windows.shape == (n, 2) and (precise_vel_ranges is None or precise_vel_ranges.shape == (n, 2))
        if precise_vel_ranges is None:
            out = np.zeros((k, n, self.shape[2], 4))
            out[..., 0], out[..., 1], out[..., 2] = self.frames[None, :, None], self.device, range_windows[None, :, 1, None]
            return out
        maps, bins = [], []
        for f in range(n):
            m = 2 + (int(self.frames[f]) % 2) * self.ragged
            x = np.zeros((k, m, 4))
            x[..., 0], x[..., 1], x[..., 2], x[..., 3] = self.frames[f], self.device, range_windows[f, 1], precise_vel_ranges[f, 0]
            maps.append(x)
            bins.append(np.full(m, self.frames[f]))
        return (np.stack(maps, axis=1) if not self.ragged else maps), bins


@pytest.mark.parametrize("world,n_frames", [(1, 5), (2, 7), (4, 10), (8, 3)])
@pytest.mark.parametrize("ragged", [0, 1])
def test_multi_device_maps_come_back_in_frame_order(world, n_frames, ragged):
    shape = (2, 2, 4)
    mp = MultiDeviceFramePipeline(None, max_frames=16, shape=shape, devices=list(range(world)),
                                  part_factory=lambda d, n: _FakePart(d, n, shape, ragged))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    assert mp.bounds == [shard_bounds(n_frames, r, world) for r in range(world)]
    wins = np.stack([np.zeros(n_frames), 10.0 + np.arange(n_frames)], axis=1)
    vrs = np.stack([-1.0 - np.arange(n_frames), np.ones(n_frames)], axis=1)
    owners = [f * world // n_frames for f in range(n_frames)]
    coarse = mp.doppler_azimuth(None, [[0], [1], [0]], wins)
    assert coarse.shape == (3, n_frames, shape[2], 4)
    assert coarse[1, :, 0, 0].tolist() == list(range(n_frames)) and coarse[2, :, 1, 1].tolist() == owners
    assert coarse[0, :, 0, 2].tolist() == wins[:, 1].tolist()                    # each shard got ITS rows of the table
    one = mp.doppler_azimuth(None, [[0]], [0.0, 3.5])                            # one pair for all frames
    assert one.shape == (1, n_frames, shape[2], 4) and np.all(one[..., 2] == 3.5)
    maps, bins = mp.doppler_azimuth(None, [[0], [1]], wins, precise_vel_ranges=vrs)
    assert len(bins) == n_frames and [b[0] for b in bins] == list(range(n_frames))
    if ragged and n_frames > 1:
        assert isinstance(maps, list) and [x.shape for x in maps] == [(2, 2 + f % 2, 4) for f in range(n_frames)]
    else:
        assert isinstance(maps, np.ndarray) and maps.shape == (2, n_frames, 2, 4)
        maps = [maps[:, f] for f in range(n_frames)]
    for f in range(n_frames):
        assert np.all(maps[f][..., 0] == f) and np.all(maps[f][..., 1] == owners[f])
        assert np.all(maps[f][..., 2] == wins[f, 1]) and np.all(maps[f][..., 3] == vrs[f, 0])
    mp.close()


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/doppler_azimuth_batch_sanitize.cpp, a program of its own that launches nothing: every class of refused argument and
    n_frames == 0 through both entries.  (No GPU sanitizer is involved; the kernels are launch stubs that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=fast", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_dopaz_batch.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_dopaz_batch.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "doppler_azimuth_batch_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "doppler_azimuth_batch_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
