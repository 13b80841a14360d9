"""Host side of the Capon range-azimuth path (no device): the float64 chain's peak on every point-target case (the condition
the GPU argmax test relies on), the pass sizing, the argument checks of ``FramePipeline.capon_range_angle_device`` before any
device call, the join order of the multi-device form, the new entry in the header / ctypes table / Makefile, and the entry's
refusals under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import capon_ra_cases as rc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib, batch
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, shard_bounds
from mmwave_radar_processing_amd.processors.steering_beamformers import CaponBeamformer
from oracle import oracle_np as O

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
CSRC = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")


def test_entry_is_declared_bound_listed_and_leaves_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+mmw_range_snapshots\s*\(([^)]*)\)\s*;", text)
    assert m, "mmw_range_snapshots is not declared in include/mmwgpu.h"
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["ctx", "d_cubes", "d_out", "n_frames", "V", "S", "C", "h_rx", "n_rx", "r_lo", "r_hi", "perform_windowing"]
    assert "mmw_range_snapshots" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_range_snapshots"]) == 12
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = re.search(r"^UNITS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "mmw_tu_range_snapshots" in units
    assert sorted(units) == sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert os.path.exists(os.path.join(CSRC, "mmw_range_snapshots.h"))


# ---------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_transform_is_the_definition(shape):
    """The DFT-matrix / np.fft reference against the defining sum on a few entries, and np.fft against the matrix on a
    power-of-two shape: the two reference forms are one definition."""
    V, S, C = shape
    x = rc.cubes(shape).astype(np.complex128)
    assert rc.cubes(shape).dtype == np.complex64 and x.shape == (rc.F, V, S, C)
    rng = np.random.default_rng(1)
    for windowing in (True, False):
        ref = rc.full_reference(shape, windowing)
        w = np.hanning(S) if windowing else np.ones(S)
        scale = np.abs(ref).max()
        for _ in range(6):
            f, v, r, c = rng.integers(rc.F), rng.integers(V), rng.integers(S), rng.integers(C)
            want = np.sum(w * x[f, v, :, c] * np.exp(-2j * np.pi * ((r * np.arange(S)) % S) / S))
            assert abs(ref[f, v, r, c] - want) <= 1e-12 * scale
    snaps = rc.reference_snapshots(shape, [V - 1, 0], (0, 1), True)
    assert snaps.shape == (rc.F, 2, 1, C) and np.array_equal(snaps[:, 1, 0], rc.full_reference(shape, True)[:, 0, 0])
    assert rc.reference_snapshots(shape, [], (0, S), False).shape == (rc.F, V, S, C)
    assert len(rc.snapshot_cases(shape)) == len(rc.windows(S)) * 4 * 2 and len(rc.windows(S)) == 4


def test_shape_list_covers_both_paths_and_the_tails():
    assert [rc.is_fft_path(s[1]) for s in rc.SHAPES] == [True, True, True, True, False, False, False]
    assert any(s[2] < 16 for s in rc.SHAPES) and any(s[2] % 16 == 1 for s in rc.SHAPES) and any(s[0] == 16 for s in rc.SHAPES)
    assert any(s[1] == 1024 for s in rc.SHAPES) and any(s[2] % 32 for s in rc.SHAPES)
    for V, S, C in rc.SHAPES:
        lists = rc.antenna_lists(V)
        assert lists[0] == [] and len(lists[1]) == 1 and len(set(lists[3])) < len(lists[3])
        assert lists[2] != sorted(lists[2]) or len(lists[2]) < 3, lists[2]           # permuted, not an ordered subset
        assert all(0 <= i < V for l in lists for i in l)
        for lo, hi in rc.windows(S):
            assert 0 <= lo < hi <= S
        lo, hi = rc.interior_window(S)
        assert lo <= rc.target_of((V, S, C))[0] < hi and (lo, hi) != (0, S)


@pytest.mark.parametrize("case", rc.point_target_cases(), ids=lambda c: "x".join(map(str, c[0])))
def test_float64_chain_peaks_at_the_target_with_margin(case):
    """Reference snapshots -> oracle_np.capon_spectrum: in row r0 of every frame the maximum sits at the grid angle nearest the
    target's and exceeds every value that is not its grid neighbour by more than 1 %.  The GPU argmax test (device argmax == this
    argmax or a grid neighbour) rests on exactly this; a case that does not meet it is changed, not excused."""
    shape, rx, window, row = case
    snaps = rc.reference_snapshots(shape, rx, window, True)
    for f in range(rc.F):
        r0, th0 = rc.target_of(shape, f)
        assert r0 - window[0] == row
        P = O.capon_spectrum(snaps[f], rc.THETAS, rc.DELTA)[row]
        t = int(np.argmax(P))
        assert t == int(np.argmin(np.abs(rc.THETAS - th0))), (shape, f, t)
        others = np.delete(P, [i for i in (t - 1, t, t + 1) if 0 <= i < len(P)])
        print(f"{shape} frame {f}: peak {P[t]:.4g} at {np.rad2deg(rc.THETAS[t]):.0f} deg, largest non-neighbour {others.max():.4g}")
        assert P[t] > 1.01 * others.max(), (shape, f)


# -------------------------------------------------------------------------------------------------------- pass sizing
def test_capon_pass_frames_at_the_budget_boundaries():
    per_frame = 8 * 256 * 128 * 8
    assert batch.capon_pass_frames(8, 256, 128, budget_bytes=64 << 20) == (64 << 20) // per_frame == 32
    assert batch.capon_pass_frames(8, 256, 128) == batch.CAPON_PASS_BUDGET // per_frame == 512        # the measured default: 1 GiB
    assert batch.capon_pass_frames(8, 256, 128, budget_bytes=per_frame) == 1
    assert batch.capon_pass_frames(8, 256, 128, budget_bytes=2 * per_frame - 1) == 1
    assert batch.capon_pass_frames(8, 256, 128, budget_bytes=2 * per_frame) == 2
    assert batch.capon_pass_frames(8, 256, 128, budget_bytes=per_frame - 1) == 1          # never below one frame
    assert batch.capon_pass_frames(16, 1024, 4096, budget_bytes=0) == 1
    assert batch.capon_pass_frames(12, 512, 128, 64 << 20) == (64 << 20) // (12 * 512 * 128 * 8) == 10
    assert batch.capon_pass_frames(1, 1, 1, budget_bytes=80) == 10
    with pytest.raises(ValueError):
        batch.capon_pass_frames(0, 4, 4)
    assert batch.capon_passes(3, 2) == [(0, 2), (2, 3)] == rc.pass_list(3, 2)
    assert batch.capon_passes(3, 1) == [(0, 1), (1, 2), (2, 3)] and batch.capon_passes(3, 3) == [(0, 3)] == batch.capon_passes(3, 7)
    assert batch.capon_passes(0, 4) == []
    with pytest.raises(ValueError):
        batch.capon_passes(3, 0)


# ---------------------------------------------------------------------------------------------------- argument checks
class _NoDevice:
    """Stands where the context and the buffers would: any use fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"device touched ({name}) before the arguments were checked")


def bare_pipeline(n_frames=3, shape=(12, 64, 32)):
    p = FramePipeline.__new__(FramePipeline)
    p.n_frames = n_frames
    p.V, p.S, p.C = shape
    p.ctx = p.bufs = p.d_in = _NoDevice()
    return p


def test_capon_range_angle_refuses_bad_arguments_before_any_device_call():
    p = bare_pipeline()
    th, rx = rc.THETAS, list(range(8))
    for method in (p.capon_range_angle_device, p.capon_range_angle):
        with pytest.raises(ValueError, match="1..16 antennas.*got 0"):
            method(th, [])
        with pytest.raises(ValueError, match="1..16 antennas.*got 17"):
            method(th, [0] * 17)
        with pytest.raises(IndexError, match="index 12 is out of bounds for 12 antennas"):
            method(th, [0, 12])
        with pytest.raises(IndexError, match="index -13 is out of bounds"):
            method(th, [-13])
        for bad in ((5, 5), (6, 5), (-1, 4), (0, 65), (64, 65)):
            with pytest.raises(ValueError, match=re.escape(f"range_bins ({bad[0]}, {bad[1]}) is not 0 <= r_lo < r_hi <= 64")):
                method(th, rx, range_bins=bad)
        with pytest.raises(ValueError, match="range_bins must be a pair"):
            method(th, rx, range_bins=(1, 2, 3))
        with pytest.raises(ValueError, match="delta -0.001 is not a finite number >= 0"):
            method(th, rx, delta=-1e-3)
        with pytest.raises(ValueError, match="delta nan"):
            method(th, rx, delta=float("nan"))
        with pytest.raises(ValueError, match="delta inf"):
            method(th, rx, delta=float("inf"))
        for bad in (0, -2, 1.5):
            with pytest.raises(ValueError, match=f"frames_per_pass must be a positive integer, got {bad}"):
                method(th, rx, frames_per_pass=bad)
        with pytest.raises(ValueError, match="non-empty 1-D grid"):
            method([], rx)
        with pytest.raises(ValueError, match="non-empty 1-D grid"):
            method(np.zeros((2, 2)), rx)
        with pytest.raises(ValueError, match="not finite"):
            method([0.0, np.nan], rx)
        with pytest.raises(ValueError, match="not finite"):
            method([np.inf], rx)
    # good arguments get as far as the device
    with pytest.raises(AssertionError, match="device touched"):
        p.capon_range_angle_device(th, rx, range_bins=(0, 64), delta=0.0, frames_per_pass=2)


def test_process_cube_refuses_bad_arguments_before_any_device_call():
    bf = CaponBeamformer(rc.THETAS)
    cube = np.zeros((4, 16, 8), dtype=np.complex64)
    with pytest.raises(ValueError, match="expected a"):
        bf.process_cube(cube[0], [0])
    with pytest.raises(IndexError, match="index 4 is out of bounds for 4 antennas"):
        bf.process_cube(cube, [0, 4])
    with pytest.raises(ValueError, match="range_bins"):
        bf.process_cube(cube, [0, 1], range_bins=(3, 17))
    with pytest.raises(ValueError, match="1..16 antennas"):
        bf.process_cube(np.zeros((2, 20, 16, 8), dtype=np.complex64), list(range(17)))
    assert bf._ctx is None and bf._bufs is None
    assert bf.process_cube(np.zeros((0, 4, 16, 8), dtype=np.complex64), [0, 1], range_bins=(2, 5)).shape == (0, 3, len(rc.THETAS))
    assert bf._ctx is None


# ------------------------------------------------------------------------------------------------------------ sharding
class _FakePart:
    """Host-only stand-in for a per-device FramePipeline: map f of its capon_range_angle() holds [global frame, device, ...]."""

    def __init__(self, device):
        self.device = device
        self.frames = np.empty(0)
        self.calls = 0

    def load(self, cubes):
        self.frames = cubes[:, 0, 0, 0].real.copy()

    def capon_range_angle(self, thetas_rad, rx_antennas, range_bins=None, delta=1e-3, perform_windowing=True, frames_per_pass=None):
        self.calls += 1
        out = np.zeros((len(self.frames), range_bins[1] - range_bins[0], len(thetas_rad)))
        out[:, 0, 0], out[:, 0, 1], out[:, 0, 2], out[:, 0, 3] = self.frames, self.device, len(rx_antennas), delta
        out[:, 1, 0], out[:, 1, 1] = perform_windowing, -1 if frames_per_pass is None else frames_per_pass
        return out


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_multi_device_maps_come_back_in_frame_order(world):
    shape, n_frames = (4, 8, 4), 3
    mp = MultiDeviceFramePipeline(None, max_frames=16, shape=shape, devices=list(range(world)), part_factory=lambda d, n: _FakePart(d))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    assert mp.bounds == [shard_bounds(n_frames, r, world) for r in range(world)]
    maps = mp.capon_range_angle(np.linspace(-1, 1, 5), [2, 1, 0], range_bins=(1, 4), delta=0.5, perform_windowing=False,
                                frames_per_pass=2)
    assert maps.shape == (n_frames, 3, 5) and maps.dtype == np.float64
    assert maps[:, 0, 0].tolist() == list(range(n_frames))                                        # frame order
    assert maps[:, 0, 1].tolist() == [f * world // n_frames for f in range(n_frames)]             # owner = floor(f W / F)
    assert np.all(maps[:, 0, 2] == 3) and np.all(maps[:, 0, 3] == 0.5) and np.all(maps[:, 1, 0] == 0) and np.all(maps[:, 1, 1] == 2)
    # ranks without frames are skipped
    assert [p.calls for p in mp.parts] == [int(hi > lo) for lo, hi in mp.bounds]
    with pytest.raises(IndexError):
        mp.capon_range_angle(np.linspace(-1, 1, 5), [4])
    mp.load(cubes[:0])
    assert mp.capon_range_angle(np.linspace(-1, 1, 5), [0, 1], range_bins=(1, 4)).shape == (0, 3, 5)
    mp.close()


# ----------------------------------------------------------------------------------------------------------- sanitizer
def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The new translation unit's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/range_snapshots_sanitize.cpp, a program of its own that launches nothing: every class of refused argument, S = 1025
    and n_frames == 0 through mmw_range_snapshots.  (No GPU sanitizer is involved; the kernels are launch stubs never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=fast", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_range_snapshots.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(CSRC, "mmw_tu_range_snapshots.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "range_snapshots_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "range_snapshots_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
