"""The Doppler-azimuth peak pickers on the device: mmw_doppler_azimuth_peaks against the host-only entry built on the same rule
(crafted maps, -2 included), and FramePipeline.doppler_azimuth_peaks against DopplerAzimuthProcessor.detect_peaks_rows /
detect_peak_zero_az applied to the maps of doppler_azimuth of the same call -- identical arrays, no tolerance.

Shapes: crafted maps with F = 3 and 1, 2, 33, 70 rows (one thread per line: fewer lines than a wave, more than a wave) and 320
rows (the image of a frame no longer fits the LDS: the lines are made from the maps; a thread takes a second line); end to end
the two shapes of tests/test_gpu_doppler_azimuth_batch.py."""
import functools

import numpy as np
import pytest

import dopaz_peaks_cases as K
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, precise_ranges_from_zero_az
from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor
from oracle import oracle_np as O
from test_gpu_doppler_azimuth_batch import SETS, SHIFTS, case, make_cm, window_of

pytestmark = pytest.mark.gpu
SENTINEL = -7
GUARD = 256
GROUPS = [(0, 1), (2, 3), (1,)]
VEL_RANGES = [[-0.25, 0.25], [0.3, 1.2], [-0.05, 0.02], [-500.0, 500.0], [-1.0, -0.2]]     # unequal m_f; [2] has a NaN half


def run_device(case_, prominence_dB=4.0, expect=_lib.MMW_OK, **override):
    """The device entry on uploaded maps; sentinel-filled outputs with a guard band behind them."""
    ctx = _lib.default_context()
    bufs = _lib.BufferSet(ctx)
    try:
        a = dict(n_sets=case_.n_sets, F=case_.F, n_rows=case_.n_rows, A=64, G=case_.G, a_lo=case_.a_lo, a_hi=case_.a_hi,
                 a_zero=case_.a_zero, thr=case_.thr)
        a.update(override)
        d_maps = bufs.get("maps", case_.maps.nbytes)
        d_maps.upload(case_.maps)
        n_row, n_zero = case_.G * case_.F * case_.n_rows, case_.G * case_.F
        d_row, d_zero = bufs.get("row", (n_row + GUARD) * 4), bufs.get("zero", (n_zero + GUARD) * 4)
        d_row.upload(np.full(n_row + GUARD, SENTINEL, dtype=np.int32))
        d_zero.upload(np.full(n_zero + GUARD, SENTINEL, dtype=np.int32))
        rc = ctx.lib.mmw_doppler_azimuth_peaks(ctx.handle, d_maps.ptr, a["n_sets"], a["F"], a["n_rows"], a["A"], K.ip(case_.groups),
                                               a["G"], K.ip(case_.m), a["a_lo"], a["a_hi"], a["a_zero"], a["thr"], prominence_dB,
                                               d_row.ptr, d_zero.ptr)
        assert rc == expect, (rc, ctx.lib.mmw_last_error())
        row, zero = d_row.download((n_row + GUARD,), np.int32).copy(), d_zero.download((n_zero + GUARD,), np.int32).copy()
        assert np.all(row[n_row:] == SENTINEL) and np.all(zero[n_zero:] == SENTINEL), "the entry wrote behind its outputs"
        if expect != _lib.MMW_OK:
            assert np.all(row == SENTINEL) and np.all(zero == SENTINEL), "a refused call wrote to its outputs"
            return None
        return row[:n_row].reshape(case_.G, case_.F, case_.n_rows), zero[:n_zero].reshape(case_.G, case_.F)
    finally:
        bufs.free()


@pytest.mark.parametrize("n_rows", [1, 2, 33, 70, 320])
def test_entry_equals_the_host_entry_on_the_crafted_maps(n_rows):
    cases = K.random_cases((n_rows,)) if n_rows < 320 else [K.random_case(900 + i, 320, thr=t) for i, t in enumerate((30.0, 3.0))]
    undecided = 0
    for c in cases:
        if n_rows >= 33:                                   # a NaN in frame 0 of set 1, an Inf behind m in frame 1
            maps = c.maps.copy()
            maps[1, 0, n_rows // 2, c.a_lo] = np.nan
            maps[2, 1, n_rows - 1, c.a_zero] = np.inf
            c = K.Case(maps, c.groups, c.m, c.a_lo, c.a_hi, c.a_zero, c.thr, c.label)
        want_row, want_zero = K.run_host_entry(c)
        got_row, got_zero = run_device(c)
        assert np.array_equal(got_row, want_row), c.label
        assert np.array_equal(got_zero, want_zero), c.label
        undecided += int(np.count_nonzero(got_row == K.UNDECIDED))
    assert (undecided > 0) == (n_rows >= 33)


@pytest.mark.parametrize("scale", [0.25, 4.0])
def test_entry_equals_the_host_entry_around_the_band(scale):
    for c, notes in K.band_cases(scale):
        want_row, want_zero = K.run_host_entry(c)
        got_row, got_zero = run_device(c)
        assert np.array_equal(got_row, want_row) and np.array_equal(got_zero, want_zero), c.label
        assert (np.any(got_row == K.UNDECIDED) or np.any(got_zero == K.UNDECIDED)) == (scale < 1)
    c = K.nonfinite_case()
    got_row, got_zero = run_device(c)
    want_row, want_zero = K.run_host_entry(c)
    assert np.array_equal(got_row, want_row) and np.array_equal(got_zero, want_zero)
    assert np.all(got_row[0, 0] == K.UNDECIDED) and got_zero[0, 0] == K.UNDECIDED


def test_refused_calls_and_empty_calls_leave_the_outputs_untouched():
    c = K.random_case(3, 9, width=20)
    run_device(c, expect=_lib.MMW_ERR_INVALID, a_zero=c.a_hi)
    run_device(c, expect=_lib.MMW_ERR_INVALID, thr=float("nan"))
    run_device(c, expect=_lib.MMW_ERR_INVALID, n_sets=2)              # group (3, 2) is outside
    run_device(c, expect=_lib.MMW_ERR_UNSUPPORTED, A=128)
    for empty in ({"F": 0}, {"G": 0}):
        ctx = _lib.default_context()
        a = dict(F=c.F, G=c.G)
        a.update(empty)
        bufs = _lib.BufferSet(ctx)
        try:
            d = bufs.get("x", 4096)
            d.upload(np.full(1024, SENTINEL, dtype=np.int32))
            rc = ctx.lib.mmw_doppler_azimuth_peaks(ctx.handle, d.ptr, c.n_sets, a["F"], c.n_rows, 64, K.ip(c.groups), a["G"], None,
                                                   c.a_lo, c.a_hi, c.a_zero, 30.0, 4.0, d.ptr, d.ptr)
            assert rc == _lib.MMW_OK
            assert np.all(d.download((1024,), np.int32) == SENTINEL)
        finally:
            bufs.free()


# ---------------------------------------------------------------------------------------------------------------- end to end
def group_map(maps_f, grp):
    """The reference's averaged response of one frame: maps_f [n_sets, m, n_valid] float64."""
    return maps_f[grp[0]] if len(grp) == 1 else (maps_f[grp[0]] + maps_f[grp[1]]) / 2


def host_picks(proc, maps_f, vel, thr=30.0):
    """(row_peaks[g], zero_az[g]) of one frame from the host pickers; a frame without rows has no peaks."""
    rows, zero = [], []
    for grp in GROUPS:
        resp = group_map(maps_f, grp)
        if resp.shape[0] == 0:
            rows.append(np.empty((0, 2))), zero.append(np.empty((0, 2)))
            continue
        rows.append(proc.detect_peaks_rows(resp.copy(), vel, thr))
        zero.append(proc.detect_peak_zero_az(resp.copy(), vel, thr))
    return rows, zero


def assert_same(got, want, what):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), what


def windows(name):
    text, _, _, rows = case(name)
    sc = O.cfg_scalars(text)
    return np.array([window_of(sc, lo, hi) for lo, hi in rows]), [f for f, (lo, hi) in enumerate(rows) if lo == hi]


def frame_maps(maps, f):
    return maps[f] if isinstance(maps, list) else maps[:, f]


@functools.lru_cache(maxsize=None)
def pipeline_results(name, precise):
    """One pipeline run per shape and mode, shared by the tests below: (maps, bins, row_peaks, zero_az, undecided)."""
    _, _, cubes, _ = case(name)
    F, V, S, C = cubes.shape
    cm = make_cm(name)
    proc = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    wins, _ = windows(name)
    vrs = np.array(VEL_RANGES[:F]) if precise else None
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    try:
        pipe.load(cubes)
        res = pipe.doppler_azimuth(proc, SETS, wins, SHIFTS, precise_vel_ranges=vrs)
        maps, bins = res if precise else (res, [proc.vel_bins] * F)
        maps = [np.array(x) for x in maps] if isinstance(maps, list) else np.array(maps)
        rows, zero = pipe.doppler_azimuth_peaks(proc, SETS, GROUPS, wins, SHIFTS, precise_vel_ranges=vrs)
        assert proc.zoomed_vel_bins is None
        return maps, bins, rows, zero, pipe.n_peaks_undecided
    finally:
        pipe.bufs.free()


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", ["golden", "ods"])
def test_pipeline_peaks_equal_the_host_pickers_on_the_maps_of_the_same_call(name, precise):
    maps, bins, rows, zero, undecided = pipeline_results(name, precise)
    proc = DopplerAzimuthProcessor(make_cm(name), num_angle_bins=64)
    _, empty = windows(name)
    F = len(bins)
    if precise:
        m = [len(b) for b in bins]
        assert len(set(m)) > 1                                       # unequal m_f
    assert len(rows) == len(zero) == len(GROUPS) and all(len(x) == F for x in rows + zero)
    n_peaks = 0
    for f in range(F):
        want_rows, want_zero = host_picks(proc, frame_maps(maps, f), bins[f])
        for g in range(len(GROUPS)):
            assert_same(rows[g][f], want_rows[g], (name, precise, "rows", g, f))
            assert_same(zero[g][f], want_zero[g], (name, precise, "zero", g, f))
            n_peaks += len(want_rows[g])
    print(f"{name} precise={precise}: {n_peaks} row peaks, {undecided} undecided (group, frame) pairs")
    assert n_peaks > 0
    assert undecided == len(empty) * len(GROUPS)                     # the NaN maps of the empty windows, nothing else


def test_two_pass_flow_equals_the_per_frame_flow_with_the_host_pickers():
    """coarse peaks -> precise_ranges_from_zero_az -> precise peaks, against the reference's flow written frame by frame
    (velocity_estimator.py:816-851) with the host pickers on the float32 batch maps."""
    name = "ods"
    _, _, cubes, _ = case(name)
    F, V, S, C = cubes.shape
    cm = make_cm(name)
    proc = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    wins = np.tile([0.5, 3.0], (F, 1))
    bound = 0.25
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    try:
        pipe.load(cubes)
        _, zero = pipe.doppler_azimuth_peaks(proc, SETS, GROUPS, wins, SHIFTS)
        assert pipe.n_peaks_undecided == 0
        ranges = precise_ranges_from_zero_az(zero[0], zero[1], bound)
        rows2, zero2 = pipe.doppler_azimuth_peaks(proc, SETS, GROUPS, wins, SHIFTS, precise_vel_ranges=ranges)
        assert pipe.n_peaks_undecided == 0
        coarse = pipe.doppler_azimuth(proc, SETS, wins, SHIFTS)
        want_ranges = np.zeros((F, 2))
        for f in range(F):
            _, z = host_picks(proc, coarse[:, f], proc.vel_bins)
            az, el = z[0], z[1]
            if az.shape[0] > 0 and el.shape[0] > 0:
                ego = -1 * (az[1] + el[1]) / 2.0
            elif az.shape[0] > 0:
                ego = -1 * az[1]
            elif el.shape[0] > 0:
                ego = -1 * el[1]
            else:
                ego = 0.0
            want_ranges[f] = [-1 * ego - bound, -1 * ego + bound]
        assert np.array_equal(ranges, want_ranges)
        assert len({tuple(r) for r in want_ranges}) > 1                  # the frames do ask for different ranges
        maps, bins = pipe.doppler_azimuth(proc, SETS, wins, SHIFTS, precise_vel_ranges=want_ranges)
        for f in range(F):
            want_rows, want_zero = host_picks(proc, frame_maps(maps, f), bins[f])
            for g in range(len(GROUPS)):
                assert_same(rows2[g][f], want_rows[g], ("rows", g, f))
                assert_same(zero2[g][f], want_zero[g], ("zero", g, f))
    finally:
        pipe.bufs.free()


@pytest.mark.parametrize("precise", [False, True])
def test_multi_device_peaks_equal_the_single_device_result(precise):
    name = "ods"
    _, _, cubes, _ = case(name)
    F, V, S, C = cubes.shape
    _, _, rows, zero, undecided = pipeline_results(name, precise)
    cm = make_cm(name)
    proc = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    wins, _ = windows(name)
    devices = [0, 1] if _lib.device_count() > 1 else [0, 0]
    mp = MultiDeviceFramePipeline(cm, max_frames=F, shape=(V, S, C), devices=devices)
    try:
        mp.load(cubes)
        assert 0 < mp.bounds[0][1] < F                                   # really split
        got_rows, got_zero = mp.doppler_azimuth_peaks(proc, SETS, GROUPS, wins, SHIFTS,
                                                      precise_vel_ranges=np.array(VEL_RANGES[:F]) if precise else None)
        assert mp.n_peaks_undecided == undecided
    finally:
        mp.close()
    for g in range(len(GROUPS)):
        for f in range(F):
            assert_same(got_rows[g][f], rows[g][f], ("rows", g, f))
            assert_same(got_zero[g][f], zero[g][f], ("zero", g, f))


@pytest.mark.parametrize("precise", [False, True])
def test_a_frames_peaks_do_not_depend_on_the_other_frames_of_the_batch(precise):
    name = "golden"
    _, _, cubes, _ = case(name)
    F, V, S, C = cubes.shape
    _, _, rows, zero, _ = pipeline_results(name, precise)
    perm = np.array([3, 0, 4, 2, 1])
    cm = make_cm(name)
    proc = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    wins, _ = windows(name)
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    try:
        pipe.load(cubes[perm])
        got_rows, got_zero = pipe.doppler_azimuth_peaks(proc, SETS, GROUPS, wins[perm], SHIFTS,
                                                        precise_vel_ranges=np.array(VEL_RANGES)[perm] if precise else None)
    finally:
        pipe.bufs.free()
    for g in range(len(GROUPS)):
        for i, f in enumerate(perm):
            assert_same(got_rows[g][i], rows[g][f], ("rows", g, f))
            assert_same(got_zero[g][i], zero[g][f], ("zero", g, f))
