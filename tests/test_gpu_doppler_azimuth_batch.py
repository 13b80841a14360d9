"""Batched Doppler-azimuth maps on the device: mmw_doppler_azimuth_batch, mmw_doppler_azimuth_zoom_batch and
FramePipeline.doppler_azimuth.

Expected values: the float64 oracle (``oracle.oracle_np.doppler_azimuth`` / ``doppler_azimuth_precise``) on ``cube_f[rx]`` and the
reference-generated fixture ``doppler_azimuth.npz``.  Bar: every value within 1e-5 of the map's peak, the bar every spectrum of
tests/test_gpu_parity.py is held to.  Every parity test prints the worst ratio it saw.

Shapes: the golden one (12 x 32 x 16, F = 5) and 12 x 63 x 70 (F = 4; odd S, more than 64 columns: a second column tile with dead
lanes, and windows of more than 32 rows: a second partition).  The angle / range-mean kernel deals row lo + q of a window to slot
q mod (4 P) of P partitions x 4 row lanes, P = ceil(rows / 32): two rows sit on two row lanes, rows 3 | 4 of a 33-row window on
two partitions."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline, doppler_azimuth_tables
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5
A = 64
ALL_ANGLES = (-10.0, 10.0)             # a valid-angle range that keeps all 64 columns: the C entries do not mask
SENTINEL = np.float32(-7.0)            # no result is negative
SETS = [[0, 3, 4, 7], [1, 2, 5, 6], [10, 11, 6, 7], [9, 8, 5, 4]]
SHIFTS = [True, True, False, False]    # azimuth sets shift, elevation sets do not
VEL_RANGES = [[-0.25, 0.25], [0.3, 1.2], [-0.05, 0.02], [-500.0, 500.0], [-1.0, -0.2]]
DP = _lib.C.POINTER(_lib.C.c_double)


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def ods_cfg_text():
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as f:
        return "\n".join(json.load(f)["6843_RadVel_ods_20Hz.cfg"]["lines"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg text, ConfigManager kwargs, cubes [F, 12, S, C], row intervals [F, 2]) -- made once, never written to."""
    if name == "golden":
        text, kw, shape, seeds = synth.synth_cfg_text(num_samples=32, num_loops=16), {}, (12, 32, 16), (101, 102, 103, 104, 105)
        rows = [[0, 32], [7, 8], [31, 32], [3, 5], [9, 9]]             # full, one row, the last row, two row lanes, empty
    else:
        text, kw, shape, seeds = ods_cfg_text(), {"array_geometry": "ods"}, (12, 63, 70), (202, 203, 204, 205)
        rows = [[0, 63], [62, 63], [10, 43], [30, 30]]                 # two partitions, the last row, rows on both partitions, empty
    cubes = np.stack([synth.synth_cube(s, shape) for s in seeds]).astype(np.complex64)
    cubes.setflags(write=False)
    return text, kw, cubes, np.array(rows, dtype=np.int32)


def make_cm(name):
    text, kw, _, _ = case(name)
    cm = ConfigManager()
    cm.load_cfg_text(text, **kw)
    return cm


def window_of(sc, lo, hi):
    """A window in metres that keeps exactly the range bins [lo, hi)."""
    res = sc["range_res_m"]
    return [(lo - 0.25) * res, (hi - 1 + 0.25) * res]


def ia(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_lib._ip)


class Device:
    """Cubes uploaded once; run() calls one of the two entries on a sentinel-filled output with a guard band behind it."""

    def __init__(self, cubes):
        self.ctx = _lib.default_context()
        self.bufs = _lib.BufferSet(self.ctx)
        self.cubes = cubes
        self.d_in = self.bufs.get("in", cubes.nbytes)
        self.d_in.upload(cubes)

    def run(self, sets, shifts, rows, flags, freq=None, n_used=None, A_=A, F=None, n_sets=None, n_rx=None, expect=_lib.MMW_OK):
        F0, V, S, C = self.cubes.shape
        F = F0 if F is None else F
        k = max(len(sets), 1) if n_sets is None else n_sets
        n_rows = C if freq is None else freq.shape[1]
        n = max(k, 1) * max(F, 1) * n_rows * A
        guard = 256
        d_out = self.bufs.get("out", (n + guard) * 4)
        d_out.upload(np.full(n + guard, SENTINEL, dtype=np.float32))
        self._keep = rx, prx = ia(sets if len(sets) else [[0]])
        self._keep2 = sf, psf = ia([0 if s else _lib.ANGLE_NO_SHIFT for s in shifts])
        self._keep3 = rw, prw = ia(rows)
        nrx = (len(sets[0]) if len(sets) else 0) if n_rx is None else n_rx
        L, h = self.ctx.lib, self.ctx.handle
        if freq is None:
            rc = L.mmw_doppler_azimuth_batch(h, self.d_in.ptr, d_out.ptr, F, V, S, C, A_, prx, k, nrx, psf, prw, flags)
        else:
            fq = np.ascontiguousarray(freq, dtype=np.float64)
            rc = L.mmw_doppler_azimuth_zoom_batch(h, self.d_in.ptr, d_out.ptr, F, V, S, C, A_, prx, k, nrx, psf, prw, flags,
                                                  C if n_used is None else n_used, fq.ctypes.data_as(DP), n_rows)
        assert rc == expect, rc
        raw = d_out.download((n + guard,), np.float32)
        assert np.all(raw[n:] == SENTINEL), "the entry wrote behind its output"
        if expect != _lib.MMW_OK:
            assert np.all(raw == SENTINEL), "a refused call wrote to d_out"
            return None
        return raw[:n].reshape(k, max(F, 1), n_rows, A).astype(np.float64)

    def free(self):
        self.bufs.free()


@pytest.fixture(scope="module", params=["golden", "ods"])
def dev(request):
    d = Device(case(request.param)[2])
    d.name = request.param
    yield d
    d.free()


def coarse_refs(name):
    """Oracle maps [set][frame] (None for the empty frame), float64, all 64 angle columns."""
    return _coarse_refs(name)


@functools.lru_cache(maxsize=None)
def _coarse_refs(name):
    text, kw, cubes, rows = case(name)
    sc = O.cfg_scalars(text)
    std = not kw
    return [[O.doppler_azimuth(cubes[f], sc, rx_antennas=rx, range_window=window_of(sc, lo, hi), shift_angle=sh,
                               valid_angle_range=ALL_ANGLES, standard_geometry=std) if hi > lo else None
             for f, (lo, hi) in enumerate(rows)] for rx, sh in zip(SETS, SHIFTS)]


def test_coarse_entry_four_sets_per_frame_windows(dev):
    _, kw, cubes, rows = case(dev.name)
    flags = _lib.ANGLE_NO_WINDOW if kw else 0
    got = dev.run(SETS, SHIFTS, rows, flags)
    refs, worst = coarse_refs(dev.name), 0.0
    for k in range(len(SETS)):
        for f, (lo, hi) in enumerate(rows):
            if hi == lo:
                assert np.all(np.isnan(got[k, f])), (k, f)          # np.mean over an empty axis
                continue
            assert np.all(np.isfinite(got[k, f])) and np.all(got[k, f] >= 0)
            worst = max(worst, rel_err(got[k, f], refs[k][f]))
    print(f"{dev.name}: coarse worst error {worst:.3e} of the map's peak")
    assert worst <= SPEC_TOL


def test_coarse_entry_all_antennas_against_the_single_frame_entry_and_two_antennas(dev):
    text, kw, cubes, rows = case(dev.name)
    F, V, S, C = cubes.shape
    sc, std = O.cfg_scalars(text), not kw
    flags = _lib.ANGLE_NO_WINDOW if kw else 0
    got = dev.run([], [True], rows, flags)
    assert got.shape == (1, F, C, A)
    d_one = dev.bufs.get("one", C * A * 4)
    worst = 0.0
    for f, (lo, hi) in enumerate(rows):
        if hi == lo:
            assert np.all(np.isnan(got[0, f]))
            continue
        _lib.check(dev.ctx.lib.mmw_doppler_azimuth(dev.ctx.handle, dev.d_in.at(f * V * S * C * 8), d_one.ptr, 1, V, S, C, A, int(lo),
                                                   int(hi), flags))
        worst = max(worst, rel_err(got[0, f], d_one.download((C, A), np.float32).astype(np.float64)))
    pair = dev.run([[2, 9], [11, 0]], [False, True], rows, flags)
    for k, (rx, sh) in enumerate((([2, 9], False), ([11, 0], True))):
        for f, (lo, hi) in enumerate(rows):
            if hi > lo:
                ref = O.doppler_azimuth(cubes[f], sc, rx_antennas=rx, range_window=window_of(sc, lo, hi), shift_angle=sh,
                                        valid_angle_range=ALL_ANGLES, standard_geometry=std)
                if np.max(ref) > 0:             # hann(2) = [0, 0]: the reference's own all-zero map
                    worst = max(worst, rel_err(pair[k, f], ref))
                else:
                    assert np.all(pair[k, f] == 0)
    print(f"{dev.name}: n_rx = 0 / n_rx = 2 worst error {worst:.3e} of the map's peak")
    assert worst <= SPEC_TOL


def test_chunked_calls_are_bit_identical_to_one_chunk():
    text, kw, cubes4, rows4 = case("ods")
    cubes = np.concatenate([cubes4, cubes4[:3][::-1]])              # 7 frames: chunks of 3, 3, 1 under a 2 MB budget
    rows = np.concatenate([rows4, [[5, 25], [0, 40], [61, 63]]]).astype(np.int32)
    d = Device(cubes)
    try:
        proc = DopplerAzimuthProcessor(make_cm("ods"))
        _, freq, m, _ = doppler_azimuth_tables(proc, np.zeros((7, 2)), np.array((VEL_RANGES + VEL_RANGES)[:7]))
        one = d.run(SETS, SHIFTS, rows, _lib.ANGLE_NO_WINDOW)
        one_z = d.run(SETS, SHIFTS, rows, _lib.ANGLE_NO_WINDOW, freq=freq)
        d.ctx.set_option("MMW_DOPAZ_CHUNK_MB", 2)
        d.ctx.profile_reset()
        d.ctx.profile_enable(1)
        try:
            many = d.run(SETS, SHIFTS, rows, _lib.ANGLE_NO_WINDOW)
            d.ctx.sync()
            assert d.ctx.profile_get("dopaz_batch")[1] == 3         # three chunks, the last one of a single frame
            d.ctx.set_option("MMW_DOPAZ_CHUNK_MB", 5)               # the zoom pass holds more per frame: 3, 3, 1 again
            many_z = d.run(SETS, SHIFTS, rows, _lib.ANGLE_NO_WINDOW, freq=freq)
            d.ctx.sync()
            assert d.ctx.profile_get("dopaz_zoom_rows")[1] == 3
        finally:
            d.ctx.profile_enable(0)
            d.ctx.set_option("MMW_DOPAZ_CHUNK_MB", None)
        assert np.array_equal(one, many, equal_nan=True) and np.array_equal(one_z, many_z, equal_nan=True)
    finally:
        d.free()


def test_reference_fixture_coarse(golden):
    g = golden("doppler_azimuth.npz")
    for name, key in (("golden", "std_sub_win"), ("ods", "ods_sub")):
        text, kw, cubes, _ = case(name)
        cm = make_cm(name)
        proc = DopplerAzimuthProcessor(cm, num_angle_bins=64, valid_angle_range=[-1.04719755, 1.04719755]) if kw else \
            DopplerAzimuthProcessor(cm, num_angle_bins=64)
        F = len(cubes)
        rows = doppler_azimuth_tables(proc, np.tile([0.9, 2.0], (F, 1)))
        d = Device(cubes)
        try:
            got = d.run([[4, 5, 8, 9]], [False], rows, _lib.ANGLE_NO_WINDOW if kw else 0)
        finally:
            d.free()
        err = rel_err(got[0, 0][:, proc.valid_angle_mask], g[key])          # frame 0 is the fixture's cube
        print(f"{name}: {key} error {err:.3e}")
        assert err <= SPEC_TOL


def test_zoom_entry_per_frame_lists(dev, golden):
    g = golden("doppler_azimuth.npz")
    text, kw, cubes, rows = case(dev.name)
    F, V, S, C = cubes.shape
    sc, std = O.cfg_scalars(text), not kw
    flags = _lib.ANGLE_NO_WINDOW if kw else 0
    proc = DopplerAzimuthProcessor(make_cm(dev.name))
    rows = rows.copy()
    rows[-1] = [4, 9]                                   # (the empty window is the coarse test's; here every frame has a map)
    vrs = np.array(VEL_RANGES[:F])
    if dev.name == "ods":
        rows[0] = doppler_azimuth_tables(proc, [0.9, 2.0])[0]       # frame 0 as the fixture's precise_ods call
    _, freq, m, bins = doppler_azimuth_tables(proc, np.zeros((F, 2)), vrs)
    assert len(set(m.tolist())) > 1 and np.isnan(freq[2, :m[2]]).any()          # M differs between frames; a NaN half inside a list
    got = dev.run(SETS, SHIFTS, rows, flags, freq=freq)
    worst = 0.0
    for f in range(F):
        lo, hi = rows[f]
        nan_rows = np.isnan(freq[f])
        assert np.all(got[:, f, nan_rows] == 0)                                  # NaN bins and the padding: exactly 0
        for k, (rx, sh) in enumerate(zip(SETS, SHIFTS)):
            ref, ref_bins = O.doppler_azimuth_precise(cubes[f], sc, rx_antennas=rx, range_window=window_of(sc, lo, hi), shift_angle=sh,
                                                      vel_range=VEL_RANGES[f], valid_angle_range=ALL_ANGLES, standard_geometry=std)
            np.testing.assert_allclose(bins[f], ref_bins, rtol=0, atol=1e-15)
            assert ref.shape == (m[f], A)
            worst = max(worst, rel_err(got[k, f, :m[f]], ref))
    print(f"{dev.name}: zoom worst error {worst:.3e} of the map's peak")
    assert worst <= SPEC_TOL
    if dev.name == "ods":
        p2 = DopplerAzimuthProcessor(make_cm("ods"), num_angle_bins=64, valid_angle_range=[-1.04719755, 1.04719755])
        fix = dev.run([[4, 5, 8, 9]], [True], rows, flags, freq=freq)
        np.testing.assert_allclose(bins[0], g["precise_ods_bins"], rtol=0, atol=1e-15)
        err = rel_err(fix[0, 0, :m[0]][:, p2.valid_angle_mask], g["precise_ods"])
        print(f"ods: precise_ods error {err:.3e}")
        assert err <= SPEC_TOL


def test_zoom_entry_with_fewer_chirps_than_the_cube(dev):
    """n_used = C - 2 against the explicit float64 sum (as tests/test_gpu_parity.py does for the single-list entry)."""
    _, kw, cubes, rows = case(dev.name)
    F, V, S, C = cubes.shape
    M = 40
    freq = np.stack([np.linspace(-0.2 - 0.01 * f, 0.3, M) for f in range(F)])
    freq[:, 5] = np.nan
    freq[1, 30:] = np.nan                                # a shorter list
    got = dev.run(SETS[:2], [True, False], rows, 0 if not kw else _lib.ANGLE_NO_WINDOW, freq=freq, n_used=C - 2)
    worst = 0.0
    for f, (lo, hi) in enumerate(rows):
        if hi == lo:
            assert np.all(np.isnan(got[:, f]))
            continue
        Z = np.exp(-2j * np.pi * np.outer(np.where(np.isnan(freq[f]), 0, freq[f]), np.arange(C - 2)))
        Z[np.isnan(freq[f])] = 0
        for k, (rx, sh) in enumerate(zip(SETS[:2], (True, False))):
            x = cubes[f][rx].astype(complex) * np.hanning(S)[None, :, None] * np.hanning(C)[None, None, :]
            if not kw:
                x = x * np.hanning(len(rx))[:, None, None]
            r = np.fft.fft(x, axis=1)[:, lo:hi, :C - 2]
            y = np.abs(np.fft.fft(np.einsum("kc,vsc->skv", Z, r), n=A, axis=2))
            ref = np.mean(np.fft.fftshift(y, axes=2) if sh else y, axis=0)
            worst = max(worst, rel_err(got[k, f], ref))
            assert np.all(got[k, f, np.isnan(freq[f])] == 0)
    print(f"{dev.name}: n_used = C - 2 worst error {worst:.3e}")
    assert worst <= SPEC_TOL


@pytest.mark.parametrize("name", ["golden", "ods"])
def test_pipeline_equals_process_per_frame_and_set(name):
    text, kw, cubes, _ = case(name)
    F, V, S, C = cubes.shape
    sc, std = O.cfg_scalars(text), not kw
    cm = make_cm(name)
    proc = DopplerAzimuthProcessor(cm, num_angle_bins=64)
    res = cm.range_res_m
    wins = np.array([[0.9, 2.0], [2.2 * res, 9.3 * res], [0.0, cm.range_max_m], [5.6 * res, 6.4 * res], [1.0, 1.7]][:F])
    vrs = np.array(VEL_RANGES[:F])
    pipe = FramePipeline(cm, max_frames=F, shape=(V, S, C))
    try:
        for resident in ("load", "load_raw"):
            if resident == "load":
                pipe.load(cubes)
            else:                                                   # virtual antenna v = tx * 4 + rx takes every 3rd chirp from tx
                raw = np.zeros((F, 4, S, 3 * C), dtype=np.complex64)
                for tx in range(3):
                    raw[:, :, :, tx::3] = cubes[:, tx * 4:tx * 4 + 4]
                pipe.load_raw(raw, 3)
            coarse = pipe.doppler_azimuth(proc, SETS, wins, shift_angle=SHIFTS)
            maps, zbins = pipe.doppler_azimuth(proc, SETS, wins, shift_angle=SHIFTS, precise_vel_ranges=vrs)
            assert proc.zoomed_vel_bins is None
            assert coarse.dtype == np.float64 and coarse.shape == (4, F, C, int(proc.valid_angle_mask.sum()))
            assert isinstance(maps, list) and len(maps) == F and len(zbins) == F
            worst = 0.0
            for f in range(F):
                for k, (rx, sh) in enumerate(zip(SETS, SHIFTS)):
                    one = DopplerAzimuthProcessor(cm, num_angle_bins=64)
                    want = one.process(cubes[f], rx_antennas=rx, range_window=wins[f], shift_angle=sh)
                    ref = O.doppler_azimuth(cubes[f], sc, rx_antennas=rx, range_window=wins[f], shift_angle=sh, standard_geometry=std)
                    assert coarse[k, f].shape == want.shape and coarse[k, f].dtype == want.dtype
                    worst = max(worst, rel_err(coarse[k, f], want), rel_err(coarse[k, f], ref), rel_err(want, ref))
                    if resident == "load_raw" and k % 2:
                        continue                                    # (the precise per-frame loop once per set pair is enough)
                    want = one.process(cubes[f], rx_antennas=rx, range_window=wins[f], shift_angle=sh, use_precise_fft=True,
                                       precise_vel_range=vrs[f])
                    ref, _ = O.doppler_azimuth_precise(cubes[f], sc, rx_antennas=rx, range_window=wins[f], shift_angle=sh,
                                                       vel_range=vrs[f], standard_geometry=std)
                    assert maps[f][k].shape == want.shape and maps[f][k].dtype == want.dtype
                    assert np.array_equal(zbins[f], one.zoomed_vel_bins)
                    worst = max(worst, rel_err(maps[f][k], want), rel_err(maps[f][k], ref), rel_err(want, ref))
            print(f"{name} / {resident}: pipeline worst error {worst:.3e}")
            assert worst <= SPEC_TOL
        same, sbins = pipe.doppler_azimuth(proc, SETS[:1], wins[0], precise_vel_ranges=[-0.25, 0.25])       # equal counts: one array
        assert isinstance(same, np.ndarray) and same.shape == (1, F, 2 * C, coarse.shape[-1]) and len(sbins) == F
        allv = pipe.doppler_azimuth(proc, (), wins)
        assert allv.shape == (1, F, C, coarse.shape[-1])
        assert rel_err(allv[0, 0], DopplerAzimuthProcessor(cm).process(cubes[0], range_window=wins[0])) <= SPEC_TOL
    finally:
        pipe.bufs.free()


def test_refused_calls_leave_the_output_untouched(dev):
    _, _, cubes, rows = case(dev.name)
    F, V, S, C = cubes.shape
    freq = np.full((F, 8), 0.1)
    INV, UNS = _lib.MMW_ERR_INVALID, _lib.MMW_ERR_UNSUPPORTED
    for fq in (None, freq):
        kw = {"freq": fq}
        dev.run(SETS, SHIFTS, rows, 0, F=-1, expect=INV, **kw)
        dev.run(SETS, SHIFTS, rows, 0, n_sets=0, expect=INV, **kw)
        dev.run(SETS, SHIFTS, rows, 0, n_rx=17, expect=INV, **kw)
        dev.run(SETS, SHIFTS, rows, 0, n_rx=-1, expect=INV, **kw)
        dev.run([[0, 3, 4, V]] + SETS[1:], SHIFTS, rows, 0, expect=INV, **kw)          # an antenna outside [0, V)
        dev.run([[0, 3, 4, -1]] + SETS[1:], SHIFTS, rows, 0, expect=INV, **kw)
        dev.run(SETS[:3] + [[9, 8, 5, 9]], SHIFTS, rows, 0, expect=INV, **kw)          # repeated within a set
        for bad in ([-1, 4], [5, 4], [0, S + 1]):
            r = rows.copy()
            r[1] = bad
            dev.run(SETS, SHIFTS, r, 0, expect=INV, **kw)
        dev.run(SETS, SHIFTS, rows, _lib.ANGLE_NO_SHIFT, expect=INV, **kw)             # the shift is per set
        dev.run(SETS, SHIFTS, rows, 8, expect=INV, **kw)
        dev.run(SETS, SHIFTS, rows, 0, A_=32, expect=UNS, **kw)
    dev.run(SETS, SHIFTS, rows, 0, freq=freq, n_used=0, expect=INV)
    dev.run(SETS, SHIFTS, rows, 0, freq=freq, n_used=C + 1, expect=INV)
    L, h = dev.ctx.lib, dev.ctx.handle
    assert L.mmw_doppler_azimuth_batch(h, None, None, F, V, S, C, A, None, 4, 4, None, None, 0) == INV         # null pointers
    assert L.mmw_doppler_azimuth_zoom_batch(h, dev.d_in.ptr, None, F, V, S, C, A, None, 4, 4, None, None, 0, C, None, 8) == INV
    # no frames: nothing launched, nothing written
    d_out = dev.bufs.get("out", 1024)
    d_out.upload(np.full(256, SENTINEL, dtype=np.float32))
    _, prx = keep = ia(SETS)
    _, psf = keep2 = ia([0, 0, 4, 4])
    _, prw = keep3 = ia(rows)
    _lib.check(L.mmw_doppler_azimuth_batch(h, dev.d_in.ptr, d_out.ptr, 0, V, S, C, A, prx, 4, 4, psf, prw, 0))
    _lib.check(L.mmw_doppler_azimuth_zoom_batch(h, dev.d_in.ptr, d_out.ptr, 0, V, S, C, A, prx, 4, 4, psf, prw, 0, C,
                                                freq.ctypes.data_as(DP), 8))
    assert np.all(d_out.download((256,), np.float32) == SENTINEL)
