"""Strip-map SAR slices (mmw_sar_slices, StripMapSARProcessor, FramePipeline.strip_map_sar) and range detections
(mmw_range_detect, RangeDetector, FramePipeline.range_detections) on the device.

SAR.  Expected values: ``np.fft.fftshift(np.fft.fft2(x[rx]), axes=1)[r0:r1, c0:c1]`` in float64 on the complex64 cube, and the
reference-generated fixture.  Bar (the project's spectra bar): every element within 1e-5 x the largest magnitude of that frame's
full plane.  Every parity test prints the worst ratio it saw.  Every call writes into a poisoned buffer with guard elements in
front of the first block and behind the last; they, and the whole buffer when every window is empty, must stay as they were.
Shapes: 2x8x7 with every window there is (1620 of them, the full plane included; odd C), three times over so that the 4860
frames pass the kernel's grid cap of 4096 workgroups; 3x63x70 (odd S, a last column block of 70 % 128 columns) on antenna 2 with
windows that end at column C, start at column 0, hold one cell, nothing, and the full plane; 2x256x128 with windows of 1, 12,
37 and 256 rows (4, 8 and 16 rows in flight, one and several passes, a last pass partly filled); 1x3x3444, the most chirps the
kernel serves (one small window), and 3445, the first it refuses.  Each of these goes through the raw entry with guards, batch
against single frame bit for bit.  The class and both pipeline forms run the reference-generated fixture (12x63x70 and
12x256x128, virtual antennas 0 and 5), and a batch whose speeds mix NaN, inf, 0.0 and -0.0 with ordinary ones.

Range detector.  Indices: identical to the fixture's (the generator kept every cell at least 1e-9 relative from its threshold).
Profile: the budget of tests/axis_fft_cases.py for mmw_range_profile_f64, ``range_profile_ulps(S) * 2^-53 * L1`` of the windowed
input.  Thresholds: bit-identical to tests/cfar_cases.py's ``ref_cfar1d`` on the device's own profile (what the CFAR tests ask
of mmw_cfar1d), and against the fixture within ``scale`` times the profile budget -- an estimate is a mean or an order statistic
of profile cells, so it moves by no more than the cells do -- plus 4 ulps of the threshold for the roundings of the sum and the
scaling (derived in DESIGN.md 4.24)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import axis_fft_cases as ac
import cfar_cases as cc
from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors.ca_cfar import CaCFAR1D
from mmwave_radar_processing_amd.processors import RangeDetector, StripMapSARProcessor
from mmwave_radar_processing_amd.processors.range_detector import device_cfar1d_args
from mmwave_radar_processing_amd.processors.strip_map_SAR_processor import pack_windows

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5
POISON = np.complex64(-7.0 - 9.0j)
GUARD = 64
GRID_CAP = 4096


def config_of(name):
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        ent = json.load(fh)[name]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    return cm


def noise_cubes(shape, F, seed):
    """Small seeded cubes: two on-bin tones per antenna (so that a wrong row, column or slab costs of the order of the peak) in noise."""
    V, S, C = shape
    rng = np.random.default_rng([seed, V, S, C])
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    x = 0.05 * (rng.standard_normal((F, V, S, C)) + 1j * rng.standard_normal((F, V, S, C)))
    for f in range(F):
        for v in range(V):
            for i in range(2):
                row, dop = rng.integers(S), rng.integers(C)
                x[f, v] += (2.0 + i + 0.3 * v) * np.exp(2j * np.pi * (row * s / S + dop * c / C))
    return x.astype(np.complex64)


def planes_of(cubes, rx):
    return np.fft.fftshift(np.fft.fft2(cubes[:, rx].astype(np.complex128), axes=(-2, -1)), axes=-1)


def run_sar(ctx, cubes, rx, windows, first=0, n_frames=None):
    """mmw_sar_slices on frames [first, first + n) into a poisoned buffer with GUARD elements on both sides: (status, blocks or
    None).  The guards are checked here."""
    F, V, S, C = cubes.shape
    n = F - first if n_frames is None else n_frames
    win, off = pack_windows(windows)
    total = int(off[-1])
    d_in, d_out = ctx.alloc(max(cubes.nbytes, 16)), ctx.alloc((total + 2 * GUARD) * 8)
    try:
        d_in.upload(cubes)
        d_out.upload(np.full(total + 2 * GUARD, POISON))
        rc = ctx.lib.mmw_sar_slices(ctx.handle, d_in.at(first * V * S * C * 8), n, V, S, C, rx,
                                    win.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    d_out.at(GUARD * 8))
        ctx.sync()
        buf = d_out.download((total + 2 * GUARD,), np.complex64)
    finally:
        d_in.free()
        d_out.free()
    assert np.all(buf[:GUARD] == POISON) and np.all(buf[GUARD + total:] == POISON), "a guard element was written"
    if rc != _lib.MMW_OK:
        assert np.all(buf == POISON), "a refused call wrote to d_out"
        return rc, None
    flat = buf[GUARD:GUARD + total]
    return rc, [flat[off[f]:off[f + 1]].reshape(win[f, 1] - win[f, 0], win[f, 3] - win[f, 2]) for f in range(len(win))]


def worst_ratio(blocks, planes, windows):
    worst = 0.0
    for blk, plane, (r0, r1, c0, c1) in zip(blocks, planes, windows):
        assert blk.shape == (r1 - r0, c1 - c0)
        if blk.size:
            assert np.all(np.isfinite(blk.view(np.float32)))
            worst = max(worst, float(np.abs(blk - plane[r0:r1, c0:c1]).max() / np.abs(plane).max()))
    return worst


@functools.lru_cache(maxsize=None)
def tiny_case():
    """2x8x7: every window of the plane, three times over (4860 frames, past the grid cap), each frame a cube of its own."""
    S, C = 8, 7
    wins = [(r0, r1, c0, c1) for r0 in range(S + 1) for r1 in range(r0, S + 1) for c0 in range(C + 1) for c1 in range(c0, C + 1)]
    assert len(wins) == 1620 and (0, S, 0, C) in wins
    wins = wins * 3
    cubes = noise_cubes((2, S, C), len(wins), seed=1)
    return cubes, wins, planes_of(cubes, 1)


def test_every_window_of_a_tiny_plane_in_a_batch_past_the_grid_cap():
    ctx = _lib.default_context()
    cubes, wins, planes = tiny_case()
    assert len(wins) > GRID_CAP
    rc, blocks = run_sar(ctx, cubes, 1, wins)
    assert rc == _lib.MMW_OK
    w = worst_ratio(blocks, planes, wins)
    print(f"sar 2x8x7, {len(wins)} frames, every window: worst error {w:.3g} of the plane's peak (bar {SPEC_TOL:g})")
    assert w <= SPEC_TOL
    # frames behind the cap (walked by a workgroup's second trip) are as good as the first
    assert worst_ratio(blocks[GRID_CAP:], planes[GRID_CAP:], wins[GRID_CAP:]) <= SPEC_TOL
    # a frame's block does not depend on the batch: single-frame calls give the same bits
    for f in list(range(0, len(wins), 211)) + [GRID_CAP - 1, GRID_CAP, len(wins) - 1]:
        rc, one = run_sar(ctx, cubes, 1, [wins[f]], first=f, n_frames=1)
        assert rc == _lib.MMW_OK and np.array_equal(one[0].view(np.float32), blocks[f].view(np.float32)), f


def test_only_empty_windows_write_nothing_and_no_frames_is_a_no_op():
    ctx = _lib.default_context()
    cubes = noise_cubes((2, 8, 7), 3, seed=2)
    rc, blocks = run_sar(ctx, cubes, 0, [(2, 2, 0, 7), (0, 8, 3, 3), (8, 8, 7, 7)])       # guards adjoin: total == 0
    assert rc == _lib.MMW_OK and all(b.size == 0 for b in blocks)
    rc, blocks = run_sar(ctx, cubes, 0, np.zeros((0, 4)), n_frames=0)
    assert rc == _lib.MMW_OK and blocks == []
    # an empty window between two full ones: its neighbours' blocks adjoin and are both right
    wins = [(0, 8, 0, 7), (3, 3, 1, 6), (0, 8, 0, 7)]
    rc, blocks = run_sar(ctx, cubes, 0, wins)
    assert rc == _lib.MMW_OK and worst_ratio(blocks, planes_of(cubes, 0), wins) <= SPEC_TOL


def test_refused_arguments_leave_the_output_untouched():
    ctx = _lib.default_context()
    cubes = noise_cubes((2, 8, 7), 2, seed=3)
    for rx, wins in ((2, [(0, 8, 0, 7)] * 2), (-1, [(0, 8, 0, 7)] * 2), (0, [(0, 8, 0, 7), (0, 9, 0, 7)]), (0, [(0, 8, 0, 7), (0, 8, 0, 8)])):
        rc, _ = run_sar(ctx, cubes, rx, wins)
        assert rc == _lib.MMW_ERR_INVALID, (rx, wins)


def test_256_by_128_windows_of_every_row_dispatch():
    ctx = _lib.default_context()
    wins = [(3, 15, 58, 69), (0, 256, 64, 65), (100, 137, 0, 128), (255, 256, 127, 128), (7, 8, 0, 1), (40, 40, 0, 128), (250, 256, 0, 3)]
    cubes = noise_cubes((2, 256, 128), len(wins), seed=4)
    rc, blocks = run_sar(ctx, cubes, 1, wins)
    assert rc == _lib.MMW_OK
    w = worst_ratio(blocks, planes_of(cubes, 1), wins)
    print(f"sar 2x256x128, windows of 1 to 256 rows: worst error {w:.3g} of the plane's peak (bar {SPEC_TOL:g})")
    assert w <= SPEC_TOL
    for f in range(len(wins)):
        rc, one = run_sar(ctx, cubes, 1, [wins[f]], first=f, n_frames=1)
        assert rc == _lib.MMW_OK and np.array_equal(one[0].view(np.float32), blocks[f].view(np.float32)), wins[f]
    # the rows in flight do not change a bit either
    for kt in (4, 8, 16):
        ctx.set_option("MMW_SAR_KT", kt)
        try:
            rc, again = run_sar(ctx, cubes, 1, wins)
        finally:
            ctx.set_option("MMW_SAR_KT", None)
        assert rc == _lib.MMW_OK and all(np.array_equal(a.view(np.float32), b.view(np.float32)) for a, b in zip(again, blocks)), kt


def test_63_by_70_windows_on_the_last_of_three_antennas():
    ctx = _lib.default_context()
    S, C = 63, 70
    wins = [(0, S, 0, C), (5, 24, 40, C), (0, 17, 0, 9), (62, 63, 69, 70), (30, 31, 35, 36), (20, 20, 0, C), (7, 40, 33, 38), (0, S, C, C)]
    cubes = noise_cubes((3, S, C), len(wins), seed=6)
    rc, blocks = run_sar(ctx, cubes, 2, wins)
    assert rc == _lib.MMW_OK
    w = worst_ratio(blocks, planes_of(cubes, 2), wins)
    print(f"sar 3x63x70, antenna 2, windows up to the full plane: worst error {w:.3g} of the plane's peak (bar {SPEC_TOL:g})")
    assert w <= SPEC_TOL
    for f in range(len(wins)):
        rc, one = run_sar(ctx, cubes, 2, [wins[f]], first=f, n_frames=1)
        assert rc == _lib.MMW_OK and np.array_equal(one[0].view(np.float32), blocks[f].view(np.float32)), wins[f]


def test_the_most_chirps_served_and_the_first_refused():
    ctx = _lib.default_context()
    cubes = noise_cubes((1, 3, 3444), 1, seed=5)
    wins = [(1, 3, 1700, 1741)]
    rc, blocks = run_sar(ctx, cubes, 0, wins)
    assert rc == _lib.MMW_OK
    w = worst_ratio(blocks, planes_of(cubes, 0), wins)
    print(f"sar 1x3x3444: worst error {w:.3g} of the plane's peak (bar {SPEC_TOL:g})")
    assert w <= SPEC_TOL
    rc, _ = run_sar(ctx, np.zeros((1, 1, 3, 3445), dtype=np.complex64), 0, [(1, 3, 1700, 1741)])
    assert rc == _lib.MMW_ERR_UNSUPPORTED


@pytest.mark.parametrize("tag", ["ods", "synth"])
def test_class_and_pipeline_against_the_reference_fixture(golden, tag):
    g = golden("strip_map_sar.npz")
    cm = config_of(str(g[f"{tag}_cfg"]))
    proc = StripMapSARProcessor(cm)
    raw = g[f"{tag}_raw"]
    num_tx = cm.frameCfg_end_index - cm.frameCfg_start_index + 1
    V, S, C = raw.shape[0] * num_tx, raw.shape[1], raw.shape[2] // num_tx
    virt = proc.virtual_array_reformatter.process(raw).astype(np.complex64)
    calls = [i for i, k in enumerate(g[f"{tag}_kinds"].tolist()) if k != "geometry only"]
    worst = 0.0
    by_rx = {}
    for i in calls:
        v, h, d = g[f"{tag}_params"][i]
        rx = int(g[f"{tag}_rx"][i])
        want = g[f"{tag}_{i}_out"]
        got = proc.process(raw, v, sensor_height_m=h, rx_index=rx, max_SAR_distance=d)
        assert got.dtype == np.complex128 and got.shape == want.shape
        sl = g[f"{tag}_slices"][i]
        assert [proc.valid_ranges_slice.start, proc.valid_ranges_slice.stop, proc.valid_angles_slice.start,
                proc.valid_angles_slice.stop] == sl.tolist()
        peak = np.abs(np.fft.fft2(virt[rx].astype(np.complex128))).max()
        if want.size:
            worst = max(worst, float(np.abs(got - want).max() / peak))
        by_rx.setdefault((rx, h, d), []).append((i, v, got))
    print(f"strip-map SAR {V}x{S}x{C} against the reference: worst error {worst:.3g} of the plane's peak (bar {SPEC_TOL:g})")
    assert worst <= SPEC_TOL
    # the batch form: one resident frame per recorded call of an (antenna, height, distance) setting, bit for bit the class
    fp = FramePipeline(cm, max_frames=8, shape=(V, S, C))
    for (rx, h, d), entries in by_rx.items():
        fp.load_raw(np.stack([raw] * len(entries)), num_tx)
        vel = np.array([v for _, v, _ in entries])
        slices, win = fp.strip_map_sar(proc, vel, sensor_height_m=h, rx_index=rx, max_SAR_distance=d)
        assert win.shape == (len(entries), 4) and win.dtype == np.int32
        for (i, v, got), blk, w in zip(entries, slices, win):
            assert blk.dtype == np.complex128 and np.array_equal(blk, got), (tag, i)
            assert w.tolist() == g[f"{tag}_slices"][i].tolist()
        d_out, off, win2 = fp.strip_map_sar_device(proc, vel, h, rx, d)
        assert isinstance(d_out, _lib.DeviceBuffer) and off.dtype == np.int64 and off[-1] == sum(b.size for b in slices)
        assert np.array_equal(win, win2)
    # one speed for every frame, and the sharded form on one device
    fp.load_raw(np.stack([raw] * 3), num_tx)
    one, _ = fp.strip_map_sar(proc, 1.5)
    assert len(one) == 3 and np.array_equal(one[0], one[2]) and np.array_equal(one[0], proc.process(raw, 1.5))
    mp = MultiDeviceFramePipeline(cm, max_frames=4, shape=(V, S, C), devices=[0])
    mp.load(np.stack([virt] * 3))
    sharded, win = mp.strip_map_sar(proc, np.array([1.5, 0.0, -2.5]))
    assert np.array_equal(sharded[0], one[0]) and sharded[1].shape[1] == 0 and win.shape == (3, 4)
    mp.close()


@pytest.mark.parametrize("tag", ["ods", "synth"])
def test_a_batch_of_nan_inf_zero_and_ordinary_speeds_equals_the_class_per_frame(golden, tag):
    """Non-finite and zero speeds follow NumPy: frame f's window is the fixture's for its speed, its block what ``process`` gives."""
    g = golden("strip_map_sar.npz")
    cm = config_of(str(g[f"{tag}_cfg"]))
    proc = StripMapSARProcessor(cm)
    raw = g[f"{tag}_raw"]
    num_tx = cm.frameCfg_end_index - cm.frameCfg_start_index + 1
    V, S, C = raw.shape[0] * num_tx, raw.shape[1], raw.shape[2] // num_tx
    params = g[f"{tag}_params"]
    rows = [i for i, (v, h, d) in enumerate(params) if (h, d) == (0.24, 1.5)]
    order = rows + rows[::-1]                    # every speed twice: a NaN has to find its window again
    vel = params[order, 0]
    assert np.isnan(vel).any() and np.isinf(vel).any() and np.signbit(vel[vel == 0]).any() and not np.signbit(vel[vel == 0]).all()
    fp = FramePipeline(cm, max_frames=len(vel), shape=(V, S, C))
    fp.load_raw(np.stack([raw] * len(vel)), num_tx)
    slices, win = fp.strip_map_sar(proc, vel)
    assert win.tolist() == g[f"{tag}_slices"][order].tolist()
    assert any(b.size for b in slices) and any(b.size == 0 for b in slices)
    for f, v in enumerate(vel):
        one = proc.process(raw, v)
        assert slices[f].dtype == np.complex128 and slices[f].shape == one.shape and np.array_equal(slices[f], one), (tag, f, v)
    mp = MultiDeviceFramePipeline(cm, max_frames=len(vel), shape=(V, S, C), devices=[0])
    mp.load(np.stack([proc.virtual_array_reformatter.process(raw).astype(np.complex64)] * len(vel)))
    sharded, win2 = mp.strip_map_sar(proc, vel)
    assert np.array_equal(win2, win) and all(np.array_equal(a, b) for a, b in zip(sharded, slices))
    mp.close()


# ---------------------------------------------------------------------------------------------------------- range detector
def range_cases(golden):
    g = golden("range_detector.npz")
    out = []
    for name in g["cases"].tolist():
        key, rest = name.split("_S")
        S, chirp = int(rest.split("_chirp")[0]), int(rest.split("_chirp")[1])
        out.append((name, key, S, chirp, json.loads(str(g[f"{name}_params"]))))
    return g, out


def profile_budget(cube, chirp, S):
    x = cube[:, :, chirp].astype(np.complex128) * np.hanning(S)
    l1 = (np.abs(x.real) + np.abs(x.imag)).sum(axis=1).mean()
    return ac.range_profile_ulps(S) * ac.EPS64 * l1


def test_class_and_pipeline_reproduce_the_reference_detections(golden):
    g, cases = range_cases(golden)
    assert {c[1] for c in cases} == {"ca_cfar_1d", "os_cfar_1d", "go_cfar_1d", "so_cfar_1d"} and {c[2] for c in cases} == {63, 256}
    assert any(c[3] != 0 for c in cases)
    worst_p = worst_t = 0.0
    for name, key, S, chirp, params in cases:
        cube = g[f"{name}_cube"]
        V, _, C = cube.shape
        cm = config_of(str(g[f"cfg_S{S}"]))
        det = RangeDetector(cm, cfar_type=key, cfar_params=params)
        kind, T, G, scale, k = device_cfar1d_args(det.cfar_detector)
        bud = profile_budget(cube, chirp, S)
        fp = FramePipeline(cm, max_frames=2, shape=(V, S, C))
        fp.load(np.stack([cube, cube]))
        dets, thr = fp.range_detections(det, chirp_idx=chirp, return_thresholds=True)
        got = [(dets[0], thr[0], fp.range_profiles[0])]
        assert np.array_equal(dets[0], dets[1]) and np.array_equal(thr[0], thr[1])
        assert np.array_equal(fp.range_detections(det, chirp_idx=chirp)[1], dets[0])
        if chirp == 0:
            out = det.process(cube)
            assert out is det.dets
            got.append((out, det.thresholds, det.range_resp))
        for d_idx, d_thr, d_prof in got:
            assert np.array_equal(d_idx, g[f"{name}_dets"]), name
            assert np.issubdtype(np.asarray(d_idx).dtype, np.integer)
            perr = np.abs(d_prof - g[f"{name}_range_resp"]).max()
            worst_p = max(worst_p, perr / bud)
            assert perr <= bud, (name, perr, bud)
            # thresholds: what mmw_cfar1d's tests ask -- the oracle's values on the same input, bit for bit
            ref_thr, _, ref_mask = cc.ref_cfar1d(d_prof, kind, T, G, scale, k)
            np.testing.assert_array_equal(d_thr, ref_thr, err_msg=name)
            assert np.array_equal(np.flatnonzero(ref_mask), d_idx)
            want = g[f"{name}_thresholds"]
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(d_thr))
            tol = scale * bud + 4 * 2.0 ** -52 * np.abs(want[fin])
            worst_t = max(worst_t, float((np.abs(d_thr[fin] - want[fin]) / tol).max()))
            assert np.all(np.abs(d_thr[fin] - want[fin]) <= tol), name
        assert np.array_equal(det._map_detections_to_bins(dets[0]), g[f"{name}_bins"])
    print(f"range detector: profile error at most {worst_p:.3g} of its budget, thresholds {worst_t:.3g} of theirs")


def run_range_detect(ctx, cubes, chirp, args, cap, with_out=True):
    F, V, S, C = cubes.shape
    kind, T, G, scale, k = args
    bufs = _lib.BufferSet(ctx)
    try:
        d_in = bufs.get("in", cubes.nbytes)
        d_in.upload(cubes)
        d_prof, d_thr = bufs.get("prof", F * S * 8), bufs.get("thr", F * S * 8)
        d_dets, d_cnt = bufs.get("dets", (F * cap + GUARD) * 4), bufs.get("cnt", F * 4)
        d_dets.upload(np.full(F * cap + GUARD, -5, dtype=np.int32))
        _lib.check(ctx.lib.mmw_range_detect(ctx.handle, d_in.ptr, F, V, S, C, chirp, kind, T, G, scale, k, d_prof.ptr if with_out else None,
                                            d_thr.ptr if with_out else None, d_dets.ptr, d_cnt.ptr, cap))
        res = dict(dets=d_dets.download((F * cap + GUARD,), np.int32), counts=d_cnt.download((F,), np.int32))
        if with_out:
            res.update(prof=d_prof.download((F, S), np.float64), thr=d_thr.download((F, S), np.float64))
        # the same by the two existing entries
        d_p2, d_t2, d_m2 = bufs.get("p2", F * S * 8), bufs.get("t2", F * S * 8), bufs.get("m2", F * S)
        _lib.check(ctx.lib.mmw_range_profile_f64(ctx.handle, d_in.ptr, d_p2.ptr, F, V, S, C, chirp))
        _lib.check(ctx.lib.mmw_cfar1d(ctx.handle, d_p2.ptr, d_t2.ptr, None, d_m2.ptr, F, S, kind, T, G, scale, k))
        res.update(prof2=d_p2.download((F, S), np.float64), thr2=d_t2.download((F, S), np.float64), mask2=d_m2.download((F, S), np.uint8))
    finally:
        bufs.free()
    return res


@pytest.mark.parametrize("S", [63, 256])
def test_one_call_equals_profile_plus_cfar1d_bit_for_bit_and_counts_past_the_capacity(golden, S):
    g, cases = range_cases(golden)
    ctx = _lib.default_context()
    for name, key, S_case, chirp, params in cases:
        if S_case != S:
            continue
        det = RangeDetector(config_of(str(g[f"cfg_S{S}"])), cfar_type=key, cfar_params=params)
        args = device_cfar1d_args(det.cfar_detector)
        base = g[f"{name}_cube"]
        cubes = np.stack([base, base[::-1].copy(), (2 * base).astype(np.complex64)])
        full = run_range_detect(ctx, cubes, chirp, args, cap=S)
        assert np.array_equal(full["prof"].view(np.uint64), full["prof2"].view(np.uint64)), name
        assert np.array_equal(full["thr"].view(np.uint64), full["thr2"].view(np.uint64)), name
        n_hits = full["mask2"].sum(axis=1)
        assert np.array_equal(full["counts"], n_hits) and n_hits.min() > 3
        table = full["dets"][:3 * S].reshape(3, S)
        for f in range(3):
            hits = np.flatnonzero(full["mask2"][f])
            assert np.array_equal(table[f, :len(hits)], hits) and np.all(table[f, len(hits):] == -5)
        assert np.all(full["dets"][3 * S:] == -5)
        # a capacity of 3: exact counts, the first three hits, nothing behind them; the optional outputs left out
        small = run_range_detect(ctx, cubes, chirp, args, cap=3, with_out=False)
        assert np.array_equal(small["counts"], n_hits)
        assert np.array_equal(small["dets"][:9].reshape(3, 3), np.stack([np.flatnonzero(full["mask2"][f])[:3] for f in range(3)]))
        assert np.all(small["dets"][9:] == -5)
        none = run_range_detect(ctx, cubes, chirp, args, cap=0, with_out=False)
        assert np.array_equal(none["counts"], n_hits) and np.all(none["dets"] == -5)


def test_a_detector_of_the_users_own_takes_the_host_path(golden):
    class Mine(CaCFAR1D):
        calls = 0

        def _compute_thresholds(self, x):
            Mine.calls += 1
            return super()._compute_thresholds(x)

    g, cases = range_cases(golden)
    name, key, S, chirp, params = next(c for c in cases if c[1] == "ca_cfar_1d" and c[3] == 0)
    cm = config_of(str(g[f"cfg_S{S}"]))
    det = RangeDetector(cm, cfar_type=key, cfar_params=params)
    det.cfar_detector = Mine(**params)
    cube = g[f"{name}_cube"]
    assert np.array_equal(det.process(cube), g[f"{name}_dets"]) and Mine.calls == 1
    fp = FramePipeline(cm, max_frames=2, shape=cube.shape)
    fp.load(np.stack([cube, cube]))
    dets, thr = fp.range_detections(det, return_thresholds=True)
    assert Mine.calls == 3 and all(np.array_equal(d, g[f"{name}_dets"]) for d in dets) and np.array_equal(thr[0], det.thresholds)
    mp = MultiDeviceFramePipeline(cm, max_frames=2, shape=cube.shape, devices=[0])
    mp.load(np.stack([cube, cube]))
    stock = RangeDetector(cm, cfar_type=key, cfar_params=params)
    d2, t2 = mp.range_detections(stock, return_thresholds=True)
    assert all(np.array_equal(d, g[f"{name}_dets"]) for d in d2) and t2.shape == (2, S)
    mp.close()
