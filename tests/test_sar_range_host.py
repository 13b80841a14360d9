"""Host side of the strip-map SAR and range-detector paths (no device): the two new C entries in the header and the ctypes table,
the SAR geometry function against the reference-generated fixture (slices and bins, exactly), the window packing, the mirrored
classes' constructors, every refused argument of both entries through the built library (both judge their arguments before they
touch the context), the argument checks of the batch forms, the join order of the multi-device forms, and the entries' host code
under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors.ca_cfar import CaCFAR1D
from mmwave_radar_processing_amd.detectors.detector_registry import get_detector_registry
from mmwave_radar_processing_amd.processors import RangeDetector, RangeProcessor, StripMapSARProcessor
from mmwave_radar_processing_amd.processors.range_detector import device_cfar1d_args
from mmwave_radar_processing_amd.processors.strip_map_SAR_processor import frame_windows, pack_windows, slice_window, strip_map_geometry

HEADER = os.path.join(ROOT, "include", "mmwgpu.h")
TAGS = ("ods", "synth")


def config_of(name):
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        ent = json.load(fh)[name]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    return cm


def test_entries_are_declared_bound_and_leave_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    want = {"mmw_sar_slices": ["ctx", "d_cubes", "n_frames", "V", "S", "C", "rx_idx", "h_win", "h_off", "d_out"],
            "mmw_range_detect": ["ctx", "d_cubes", "n_frames", "V", "S", "C", "chirp_idx", "kind", "num_train", "num_guard", "scale",
                                 "k_rank", "d_profile", "d_thr", "d_dets", "d_counts", "cap"]}
    for name, names in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in include/mmwgpu.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name]) == len(names)
        assert hasattr(_lib.load_library(), name)
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text) and _lib.ABI_VERSION == 7


@pytest.mark.parametrize("tag", TAGS)
def test_geometry_equals_the_fixture_exactly(golden, tag):
    g = golden("strip_map_sar.npz")
    p = StripMapSARProcessor(config_of(str(g[f"{tag}_cfg"])))
    assert [p.lambda_m, p.chirp_period_us, p.chirps_per_frame] == g[f"{tag}_tables"].tolist()
    for got, key in ((p.phase_shifts, "phase_shifts"), (p.range_bins, "range_bins")):
        assert got.dtype == np.float64 and np.array_equal(got, g[f"{tag}_{key}"])
    assert len(p.phase_shifts) == p.config_manager.frameCfg_loops != p.chirps_per_frame       # one phase per loop, not per chirp
    assert isinstance(p.virtual_array_reformatter.config_manager, ConfigManager)
    kinds = g[f"{tag}_kinds"].tolist()
    assert {"wide and touching", "single", "empty", "negative", "custom", "geometry only"} <= set(kinds)
    S, C = len(p.range_bins), len(p.phase_shifts)
    for i, (v, h, d) in enumerate(g[f"{tag}_params"]):
        geom = strip_map_geometry(v, h, d, p.az_angle_range_rad, phase_shifts=p.phase_shifts, lambda_m=p.lambda_m,
                                  chirp_period_us=p.chirp_period_us, range_bins=p.range_bins)
        r, a = geom.valid_ranges_slice, geom.valid_angles_slice
        assert [r.start, r.stop, a.start, a.stop] == g[f"{tag}_slices"][i].tolist(), kinds[i]
        for got, key in ((geom.ground_range_bins, "ground_range"), (geom.ground_az_bins_rad, "ground_az"),
                         (geom.angle_bins_rad, "angle_bins")):
            want = g[f"{tag}_{i}_{key}"]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (kinds[i], key)
        # the meshes are the reference's expressions on those bins
        th, rh = np.meshgrid(geom.ground_az_bins_rad, geom.ground_range_bins, indexing="xy")
        assert np.array_equal(geom.thetas, th, equal_nan=True) and np.array_equal(geom.rhos, rh, equal_nan=True)
        assert np.array_equal(geom.x_s, rh * np.cos(th), equal_nan=True) and np.array_equal(geom.y_s, rh * np.sin(th), equal_nan=True)
        # the method sets the attributes the plotters read, to the same values
        assert p.configure_array_geometry(v, h, d).valid_angles_slice == a and p.valid_ranges_slice == r and p.valid_angles_slice == a
        assert np.array_equal(p.x_s, geom.x_s, equal_nan=True) and np.array_equal(p.ground_range_bins, geom.ground_range_bins,
                                                                               equal_nan=True)
        lean = p.geometry(v, h, d, meshes=False)
        assert lean.thetas is None and lean.x_s is None and lean.valid_angles_slice == a
        win = slice_window(geom, S, C)
        assert win == (r.start, r.stop, a.start, a.stop)
        if f"{tag}_{i}_out" in g.files:
            assert g[f"{tag}_{i}_out"].shape == (win[1] - win[0], win[3] - win[2])
    touching = g[f"{tag}_slices"][kinds.index("wide and touching")]
    assert touching[2] == 0 or touching[3] == C - 1
    assert np.diff(g[f"{tag}_slices"][kinds.index("single")][2:]) == 1 and np.diff(g[f"{tag}_slices"][kinds.index("empty")][2:]) == 0


def test_no_qualifying_range_bin_is_the_reference_index_error():
    p = StripMapSARProcessor(config_of("6843_RadVel_ods_20Hz.cfg"))
    for h, d in ((1e3, 1.5), (0.24, -1.0)):
        with pytest.raises(IndexError):
            p.configure_array_geometry(1.0, h, d)
    # a height beyond the distance is a reversed slice: an empty window, as NumPy slices it
    geom = p.geometry(1.0, 1.2, 0.5)
    assert geom.valid_ranges_slice.start > geom.valid_ranges_slice.stop
    win = slice_window(geom, len(p.range_bins), len(p.phase_shifts))
    assert win[0] == win[1] and np.zeros((63, 70))[geom.valid_ranges_slice, geom.valid_angles_slice].shape == (0, win[3] - win[2])
    q = StripMapSARProcessor(p.config_manager, az_angle_range_rad=[-0.2, 0.1])
    assert isinstance(q.az_angle_range_rad, np.ndarray) and q.az_angle_range_rad.tolist() == [-0.2, 0.1]


def test_windows_pack_back_to_back():
    win, off = pack_windows([(1, 3, 2, 7), (0, 0, 0, 5), (2, 4, 3, 3), (0, 4, 0, 8)])
    assert win.dtype == np.int32 and win.shape == (4, 4) and off.dtype == np.int64
    assert off.tolist() == [0, 10, 10, 10, 42]
    win, off = pack_windows(np.zeros((0, 4)))
    assert win.shape == (0, 4) and off.tolist() == [0]


def test_process_checks_come_before_any_device_call(golden):
    g = golden("strip_map_sar.npz")
    p = StripMapSARProcessor(config_of(str(g["ods_cfg"])))
    del p.virtual_array_reformatter
    p.config_manager.virtual_antennas_enabled = False
    cube = np.zeros((12, 63, 70), dtype=np.complex64)
    with pytest.raises(IndexError):
        p.process(cube, 1.0, rx_index=12)
    with pytest.raises(ValueError):
        p.process(cube[0], 1.0)
    out = p.process(cube, 0.0)                   # the platform at rest: an empty window needs no device
    assert out.shape == (19, 0) and out.dtype == np.complex128 and p._ctx is None


def test_range_detector_mirrors_the_reference_class(golden):
    g = golden("range_detector.npz")
    cm = config_of(str(g["cfg_S63"]))
    assert str(g["default_error"]) == "TypeError"
    with pytest.raises(TypeError):
        RangeDetector(cm)                         # os_cfar_1d with {}: the detector's constructor has no defaults, as in the reference
    with pytest.raises(ValueError) as e:
        RangeDetector(cm, cfar_type="nope")
    assert str(e.value) == str(g["unknown_key_message"]) and all(k in str(e.value) for k in get_detector_registry())
    for name in g["cases"].tolist():
        key, S = name.split("_S")[0], int(name.split("_S")[1].split("_")[0])
        d = RangeDetector(config_of(str(g[f"cfg_S{S}"])), cfar_type=key, cfar_params=json.loads(str(g[f"{name}_params"])))
        assert isinstance(d, RangeProcessor) and d.dets is None and d.thresholds is None and d.range_resp is None
        assert type(d.cfar_detector) is get_detector_registry()[key] and device_cfar1d_args(d.cfar_detector) is not None
        assert np.array_equal(d.range_bins, g[f"range_bins_S{S}"])
        assert np.array_equal(d._map_detections_to_bins(g[f"{name}_dets"]), g[f"{name}_bins"])
    d.range_bins = None
    with pytest.raises(ValueError, match="not configured"):
        d._map_detections_to_bins(np.array([1]))


def test_only_the_stock_detectors_run_on_the_device():
    class Mine(CaCFAR1D):
        pass

    class Own(CaCFAR1D):
        def _compute_thresholds(self, x):
            return np.full(len(x), np.inf), np.zeros(len(x))

    assert device_cfar1d_args(CaCFAR1D(4, 1, 1e-2))[:3] == (_lib.CFAR_CA, 4, 1)
    assert device_cfar1d_args(Mine(4, 1, 1e-2)) is None and device_cfar1d_args(Own(4, 1, 1e-2)) is None
    assert device_cfar1d_args(get_detector_registry()["ca_cfar_2d"]((4, 4), (1, 1), 1e-2)) is None


def _ctx_stand_in():
    """Bytes that are never dereferenced: both entries judge every argument before they touch their context."""
    return ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)


def test_sar_entry_refuses_bad_arguments_without_a_device():
    lib, ctx = _lib.load_library(), _ctx_stand_in()
    V, S, C = 2, 4, 8
    cube, out = ctypes.create_string_buffer(V * S * C * 8), ctypes.create_string_buffer(S * C * 8)
    before = out.raw

    def call(ctx=ctx, cube=cube, F=1, V=V, S=S, C=C, rx=0, win=(1, 3, 2, 7), off=(0, 10), out=out):
        w = None if win is None else (ctypes.c_int32 * len(win))(*win)
        o = None if off is None else (ctypes.c_int64 * len(off))(*off)
        return lib.mmw_sar_slices(ctx, cube, F, V, S, C, rx, w, o, out)

    assert call(F=0) == _lib.MMW_OK
    bad = [dict(ctx=None), dict(cube=None), dict(win=None), dict(off=None), dict(out=None), dict(F=-1), dict(V=0), dict(S=0), dict(C=-1),
           dict(rx=-1), dict(rx=V), dict(win=(3, 1, 2, 7)), dict(win=(1, 3, 7, 2)), dict(win=(-1, 3, 2, 7), off=(0, 20)),
           dict(win=(1, S + 1, 2, 7), off=(0, 20)), dict(win=(1, 3, 2, C + 1), off=(0, 14)), dict(win=(1, 3, -1, 7), off=(0, 16)),
           dict(off=(1, 11)), dict(off=(0, 9)), dict(off=(0, 11)), dict(off=(0, -10)), dict(F=0, off=(1, 1)), dict(F=0, rx=V),
           dict(F=2, win=(1, 3, 2, 7, 0, 1, 0, 1), off=(0, 10, 12))]
    for kw in bad:
        assert call(**kw) == _lib.MMW_ERR_INVALID, kw
        assert lib.mmw_last_error(), kw
    with pytest.raises(ValueError, match="rx_idx 7"):
        _lib.check(call(rx=7))
    assert out.raw == before


def test_range_entry_refuses_bad_arguments_without_a_device():
    lib, ctx = _lib.load_library(), _ctx_stand_in()
    V, S, C = 2, 16, 3
    cube = ctypes.create_string_buffer(V * S * C * 8)
    dets, counts = ctypes.create_string_buffer(S * 4), ctypes.create_string_buffer(4)

    def call(ctx=ctx, cube=cube, F=1, V=V, S=S, C=C, chirp=0, kind=_lib.CFAR_OS, T=3, G=1, k=4, dets=dets, counts=counts, cap=S):
        return lib.mmw_range_detect(ctx, cube, F, V, S, C, chirp, kind, T, G, 2.0, k, None, None, dets, counts, cap)

    assert call(F=0) == _lib.MMW_OK and call(F=0, chirp=-C, cap=0) == _lib.MMW_OK
    bad = [dict(ctx=None), dict(cube=None), dict(dets=None), dict(counts=None), dict(F=-1), dict(F=65536), dict(V=0), dict(S=0), dict(C=0),
           dict(chirp=C), dict(chirp=-C - 1), dict(cap=-1), dict(kind=-1), dict(kind=4), dict(T=-1), dict(G=-1), dict(T=513, kind=_lib.CFAR_CA),
           dict(k=0), dict(k=7), dict(F=0, chirp=C)]
    for kw in bad:
        assert call(**kw) == _lib.MMW_ERR_INVALID, kw
    assert call(S=49153) == _lib.MMW_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="chirp_idx 9"):
        _lib.check(call(chirp=9))


def test_batch_forms_check_their_arguments_before_the_context(golden):
    g = golden("strip_map_sar.npz")
    fp = FramePipeline.__new__(FramePipeline)        # no context, no buffers: a refused call must not need them
    fp.n_frames, fp.V, fp.S, fp.C = 3, 12, 63, 70
    p = StripMapSARProcessor(config_of(str(g["ods_cfg"])))
    with pytest.raises(ValueError, match="StripMapSARProcessor"):
        fp.strip_map_sar(object(), 1.0)
    for vel in (np.zeros(2), np.zeros((3, 1)), np.zeros(4)):
        with pytest.raises(ValueError, match="velocities"):
            fp.strip_map_sar_device(p, vel)
    for rx in (12, -13):
        with pytest.raises(IndexError):
            fp.strip_map_sar(p, np.ones(3), rx_index=rx)
    with pytest.raises(IndexError):
        fp.strip_map_sar(p, np.ones(3), sensor_height_m=1e3)
    with pytest.raises(ValueError, match="RangeDetector"):
        fp.range_detections(RangeProcessor(p.config_manager))
    det = RangeDetector(p.config_manager, "ca_cfar_1d", dict(num_train=4, num_guard=1, pfa=1e-2))
    for chirp in (70, -71):
        with pytest.raises(IndexError):
            fp.range_detections(det, chirp_idx=chirp)


@pytest.mark.parametrize("tag", TAGS)
def test_batch_windows_follow_numpy_for_non_finite_and_zero_speeds(golden, tag):
    """NaN, inf, 0.0 and -0.0 among ordinary speeds, each twice: frame f's window is the fixture's for ``velocities[f]`` (a NaN is
    not equal to itself, so a table keyed by the speed's value would never find it again)."""
    g = golden("strip_map_sar.npz")
    p = StripMapSARProcessor(config_of(str(g[f"{tag}_cfg"])))
    S, C = len(p.range_bins), len(p.phase_shifts)
    params = g[f"{tag}_params"]
    rows = [i for i, (v, h, d) in enumerate(params) if (h, d) == (0.24, 1.5)]
    order = rows + rows[::-1]
    vel = params[order, 0]
    assert np.isnan(vel).sum() == 2 and np.isinf(vel).sum() == 2 and (vel == 0).sum() == 4 and np.signbit(vel[vel == 0]).sum() == 2
    assert np.isfinite(vel[vel != 0]).sum() >= 6
    want = g[f"{tag}_slices"][order]
    win, off = frame_windows(p, vel, 0.24, 1.5, S, C)
    assert win.tolist() == want.tolist()
    assert off.tolist() == [0] + np.cumsum((want[:, 1] - want[:, 0]) * (want[:, 3] - want[:, 2])).tolist()
    assert frame_windows(p, np.zeros(0), 0.24, 1.5, S, C)[1].tolist() == [0]
    # the batch form hands exactly these windows to the entry (stand-ins for the context and its buffers record the call)
    seen = {}

    def entry(handle, d_cubes, F, V_, S_, C_, rx, h_win, h_off, d_out):
        seen.update(F=F, rx=rx, win=np.ctypeslib.as_array(h_win, (F, 4)).copy(), off=np.ctypeslib.as_array(h_off, (F + 1,)).copy())
        return _lib.MMW_OK

    fp = FramePipeline.__new__(FramePipeline)
    fp.n_frames, fp.V, fp.S, fp.C = len(vel), 12, S, C
    fp.d_in = types.SimpleNamespace(ptr=None)
    fp.bufs = types.SimpleNamespace(get=lambda name, nbytes: types.SimpleNamespace(ptr=None, nbytes=nbytes))
    fp.ctx = types.SimpleNamespace(handle=None, lib=types.SimpleNamespace(mmw_sar_slices=entry))
    d_out, off2, win2 = fp.strip_map_sar_device(p, vel, rx_index=-1)
    assert seen["F"] == len(vel) and seen["rx"] == 11 and d_out.nbytes == max(int(off[-1]), 1) * 8
    assert np.array_equal(seen["win"], win) and np.array_equal(seen["off"], off) and np.array_equal(win2, win) and np.array_equal(off2, off)


class _FakePart:
    """Host-only stand-in for a per-device FramePipeline: its results name the global frame, the device and the arguments."""

    def __init__(self, device, max_frames, shape):
        self.device, self.shape, self.frames = device, shape, np.empty(0)

    def load(self, cubes):
        self.frames = cubes[:, 0, 0, 0].real.copy()

    def strip_map_sar(self, proc, velocities, sensor_height_m, rx_index, max_SAR_distance):
        assert len(velocities) == len(self.frames)
        win = np.array([[0, 1, 0, int(f) % 3] for f in self.frames], dtype=np.int32).reshape(-1, 4)
        return [np.full((1, int(f) % 3), f + 1j * v + self.device * 100) for f, v in zip(self.frames, velocities)], win

    def range_detections(self, detector, chirp_idx, return_thresholds):
        self.asked = return_thresholds
        dets = [np.array([int(f), self.device, chirp_idx]) for f in self.frames]
        return (dets, np.tile(self.frames[:, None], (1, self.shape[1]))) if return_thresholds else dets


@pytest.mark.parametrize("world,n_frames", [(1, 5), (2, 7), (4, 10), (8, 3), (3, 0)])
def test_multi_device_results_come_back_in_frame_order(world, n_frames):
    shape = (2, 4, 4)
    mp = MultiDeviceFramePipeline(None, max_frames=16, shape=shape, devices=list(range(world)),
                                  part_factory=lambda d, n: _FakePart(d, n, shape))
    cubes = np.zeros((n_frames,) + shape, dtype=np.complex64)
    cubes[:, 0, 0, 0] = np.arange(n_frames)
    mp.load(cubes)
    owner = [f * world // n_frames for f in range(n_frames)]
    vel = np.arange(n_frames) * 0.5
    slices, win = mp.strip_map_sar(None, vel)
    assert len(slices) == n_frames and win.shape == (n_frames, 4) and win.dtype == np.int32
    for f in range(n_frames):
        assert slices[f].shape == (1, f % 3) and win[f].tolist() == [0, 1, 0, f % 3]
        assert np.all(slices[f] == f + 1j * vel[f] + owner[f] * 100)
    if n_frames:
        with pytest.raises(ValueError, match="velocities"):
            mp.strip_map_sar(None, vel[:-1])
    assert len(mp.strip_map_sar(None, 2.0)[0]) == n_frames                     # one speed for every frame
    dets = mp.range_detections(None, chirp_idx=2)
    assert [d.tolist() for d in dets] == [[f, owner[f], 2] for f in range(n_frames)]
    live = [p for p in mp.parts if len(p.frames)]
    assert all(p.asked is False for p in live)            # thresholds nobody asked for are not made on any shard
    dets2, thr = mp.range_detections(None, return_thresholds=True)
    assert all(p.asked is True for p in live)
    assert len(dets2) == n_frames and thr.shape == (n_frames, shape[1]) and thr[:, 0].tolist() == list(range(n_frames))
    mp.close()


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """The two translation units' host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/sar_range_sanitize.cpp, a program of its own that launches nothing: every class of refused argument and
    n_frames == 0 through mmw_sar_slices and mmw_range_detect, and the window / offset validation over a sweep.  (No GPU sanitizer
    is involved; the kernels are launch stubs that are never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=fast", "--cuda-host-only"]
    objs = []
    for unit in ("mmw_tu_sar", "mmw_tu_cfar"):
        objs.append(str(tmp_path / f"{unit}.o"))
        subprocess.run([hipcc, *flags, "-c", "-o", objs[-1], os.path.join(csrc, f"{unit}.hip")], check=True)
    # the host-only objects still refer to their (absent) device code objects: empty stand-ins, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", *objs], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "sar_range_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "sar_range_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", *objs, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
