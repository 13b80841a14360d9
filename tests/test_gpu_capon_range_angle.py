"""Capon range-azimuth maps over resident frames: mmw_range_snapshots through the C ABI and the host API on top of it.

Inputs and float64 references: tests/capon_ra_cases.py (tests/test_capon_range_angle_host.py checks them without a GPU).

| test                         | what would make it fail                                                                          |
|------------------------------|--------------------------------------------------------------------------------------------------|
| snapshots against float64    | a wrong twiddle, window, antenna, row or chirp index on either path; a write outside the result   |
| rows of the full transform   | a window's row computed by other arithmetic than the same row of the whole profile                |
| chain identity               | a wrong slice offset per pass, the scratch buffer reused too early, a short last pass             |
| float64 definition           | the Capon stage reading the snapshots in another layout than the snapshot stage writes            |
| end to end                   | any of the above, seen as a peak at the wrong angle                                               |
| entry points agree           | process_cube or the multi-device form making other calls than the pipeline                        |
| load_raw batch               | the path depending on how the frames became resident                                              |
| unsupported input            | a launch, or a write, on a sample count the kernels cannot hold                                   |
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capon_cases as cc
import capon_ra_cases as rc
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from mmwave_radar_processing_amd.processors.steering_beamformers import CaponBeamformer
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s)) for s in rc.SHAPES]
BAR = 1e-5                  # the project's bar for float32 spectra against float64 (README "parity")
GUARD = 4096                # bytes of poison kept before and behind every result
POISON = np.float32(-7.0)


class GridConfig:
    """The scalars FramePipeline reads: S range bins 1 m apart, C velocity bins 1 m/s apart."""

    def __init__(self, S, C):
        self.range_res_m, self.range_max_m = 1.0, float(S)
        self.vel_res_m_s, self.vel_max_m_s = 1.0, C / 2
        self.frameCfg_periodicity_ms = 50.0


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def snapshots(ctx, d_cube, shape, rx, window, windowing, n_frames=rc.F):
    """mmw_range_snapshots into a poisoned buffer with a guard on either side: (complex64 [F][n][R_w][C], guards intact)."""
    V, S, Cc = shape
    n = len(rx) if len(rx) else V
    Rw = window[1] - window[0]
    nbytes = n_frames * n * Rw * Cc * 8
    d_out = ctx.alloc(nbytes + 2 * GUARD)
    try:
        d_out.upload(np.full((nbytes + 2 * GUARD) // 4, POISON, np.float32))
        rx_arr, n_rx = _lib.int_array(rx)
        _lib.check(ctx.lib.mmw_range_snapshots(ctx.handle, d_cube.ptr, d_out.at(GUARD), n_frames, V, S, Cc, rx_arr, n_rx, window[0],
                                               window[1], int(windowing)))
        raw = d_out.download(((nbytes + 2 * GUARD) // 4,), np.float32)
    finally:
        d_out.free()
    g = GUARD // 4
    guards = bool(np.all(raw[:g] == POISON) and np.all(raw[-g:] == POISON))
    return raw[g:-g].view(np.complex64).reshape(n_frames, n, Rw, Cc).copy(), guards


@functools.lru_cache(maxsize=None)
def device_cases(shape):
    """Every snapshot case of the shape, run once and shared by the tests: {(rx, window, windowing): (array, guards intact)}."""
    ctx = _lib.default_context()
    cubes = rc.cubes(shape)
    d_cube = ctx.alloc(cubes.nbytes)
    try:
        d_cube.upload(cubes)
        return {(tuple(rx), w, win): snapshots(ctx, d_cube, shape, rx, w, win) for rx, w, win in rc.snapshot_cases(shape)}
    finally:
        d_cube.free()


def pipeline(shape, ctx=None):
    V, S, Cc = shape
    p = FramePipeline(GridConfig(S, Cc), max_frames=rc.F, shape=shape, ctx=ctx)
    p.load(rc.cubes(shape))
    return p


# ------------------------------------------------------------------------------------------------------ 1. snapshots
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
def test_snapshots_against_float64(shape):
    """max |dev - ref| <= 1e-5 of the frame's largest reference magnitude, for every window / antenna list / window switch; every
    entry of [F][n_rx][R_w][C] written and nothing before or behind it.  Observed on an MI355X: see DESIGN.md 4.20."""
    worst = 0.0
    for (rx, w, win), (dev, guards) in device_cases(shape).items():
        ref = rc.reference_snapshots(shape, list(rx), w, win)
        assert dev.shape == ref.shape
        assert guards, f"rx {rx} window {w}: written outside [F][n_rx][R_w][C]"
        flat = dev.view(np.float32)
        assert not np.any((flat[..., 0::2] == POISON) & (flat[..., 1::2] == POISON)), f"rx {rx} window {w}: entries left unwritten"
        # the frame's largest reference magnitude: of the whole profile of the listed antennas, so that a window without the
        # target is held to the same absolute error as the rows around it
        ants = list(rx) if rx else list(range(shape[0]))
        scale = np.abs(rc.full_reference(shape, win)[:, ants]).max(axis=(1, 2, 3))
        ratio = (np.abs(dev.astype(np.complex128) - ref).max(axis=(1, 2, 3)) / scale).max()
        worst = max(worst, ratio)
        assert ratio <= BAR, f"rx {rx} window {w} windowing {win}: error {ratio:.3e} of the peak"
    print(f"{shape} ({'FFT' if rc.is_fft_path(shape[1]) else 'direct'} path): worst error {worst:.3e} of the frame's peak "
          f"over {len(device_cases(shape))} cases")


# --------------------------------------------------------------------------------------- 2. rows of the full transform
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
def test_window_rows_are_the_full_transforms_rows_bit_for_bit(shape):
    S = shape[1]
    res = device_cases(shape)
    n = 0
    for (rx, w, win), (dev, _) in res.items():
        if w == (0, S):
            continue
        full = res[(rx, (0, S), win)][0]
        assert np.array_equal(dev.view(np.float32), full[:, :, w[0]:w[1]].view(np.float32)), f"rx {rx} window {w} windowing {win}"
        n += 1
    assert n == 3 * 4 * 2


# ------------------------------------------------------------------------------------------------- 3. chain identity
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
def test_passes_equal_one_capon_call_on_all_snapshots_bit_for_bit(ctx, shape):
    V, S, Cc = shape
    rx, window = rc.ula(V), rc.interior_window(S)
    Rw, T = window[1] - window[0], len(rc.THETAS)
    p = pipeline(shape, ctx)
    try:
        snaps, _ = snapshots(ctx, p.d_in, shape, rx, window, True)
        d_x, d_p = ctx.alloc(snaps.nbytes), ctx.alloc(rc.F * Rw * T * 4)
        try:
            d_x.upload(snaps)
            _lib.check(ctx.lib.mmw_capon(ctx.handle, d_x.ptr, dptr(rc.THETAS), d_p.ptr, rc.F, len(rx), Rw, Cc, T, rc.DELTA))
            want = d_p.download((rc.F, Rw, T), np.float32)
        finally:
            d_x.free()
            d_p.free()
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        for fpp in (1, 2, rc.F, None):
            d = p.capon_range_angle_device(rc.THETAS, rx, range_bins=window, delta=rc.DELTA, frames_per_pass=fpp)
            got = d.download((rc.F, Rw, T), np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"frames_per_pass {fpp}"
        assert np.array_equal(p.capon_range_angle(rc.THETAS, rx, range_bins=window, delta=rc.DELTA, frames_per_pass=2),
                              want.astype(np.float64))
    finally:
        p.bufs.free()


# --------------------------------------------------------------------------------------------- 4. float64 definition
@pytest.mark.parametrize("shape", rc.SHAPES, ids=SHAPE_IDS)
def test_maps_against_the_float64_definition_on_the_device_snapshots(ctx, shape):
    """The device spectrum against oracle_np.capon_spectrum on the DOWNLOADED device snapshots, at capon_cases.bound(cond2): the
    existing bound and constants of mmw_capon, nothing new pinned."""
    V, S, Cc = shape
    rx, window = rc.ula(V), rc.interior_window(S)
    p = pipeline(shape, ctx)
    try:
        snaps, _ = snapshots(ctx, p.d_in, shape, rx, window, True)
        P = p.capon_range_angle(rc.THETAS, rx, range_bins=window, delta=rc.DELTA)
    finally:
        p.bufs.free()
    ref = np.stack([O.capon_spectrum(snaps[f], rc.THETAS, rc.DELTA) for f in range(rc.F)])
    cond = cc.cond2(snaps, rc.DELTA)
    err = np.abs(P - ref) / np.abs(ref)
    i = np.unravel_index(np.argmax(err.max(axis=-1) / cc.bound(cond)), cond.shape)
    print(f"{shape}: cond2 {cond.min():.2e}..{cond.max():.2e}, worst error {err.max():.3e}, tightest bin: error "
          f"{err[i].max():.3e} of bound {cc.bound(cond[i]):.3e}")
    assert np.all(np.isfinite(P))
    assert np.all(err <= cc.bound(cond)[..., None])


# ---------------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("case", rc.point_target_cases(), ids=SHAPE_IDS)
def test_peak_angle_of_the_target_row(ctx, case):
    """The device argmax over angles of the target's row equals the float64 chain's argmax (reference snapshots ->
    oracle_np.capon_spectrum) or a grid neighbour of it -- test_capon_range_angle_host.py shows that chain's peak to stand more
    than 1 % above every non-neighbour --, through the pipeline and through CaponBeamformer.process_cube."""
    shape, rx, window, row = case
    ref_snaps = rc.reference_snapshots(shape, rx, window, True)
    want = [int(np.argmax(O.capon_spectrum(ref_snaps[f], rc.THETAS, rc.DELTA)[row])) for f in range(rc.F)]
    p = pipeline(shape, ctx)
    try:
        P = p.capon_range_angle(rc.THETAS, rx, range_bins=window, delta=rc.DELTA)
    finally:
        p.bufs.free()
    bf = CaponBeamformer(rc.THETAS, delta=rc.DELTA, ctx=ctx)
    Q = bf.process_cube(rc.cubes(shape), rx, range_bins=window)
    bf._bufs.free()
    assert P.shape == Q.shape == (rc.F, window[1] - window[0], len(rc.THETAS)) and P.dtype == Q.dtype == np.float64
    for name, maps in (("pipeline", P), ("process_cube", Q)):
        got = [int(np.argmax(maps[f, row])) for f in range(rc.F)]
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), (name, got, want)


# ------------------------------------------------------------------------------------------- 6. entry points agree
@pytest.mark.parametrize("shape", [rc.SHAPES[1], rc.SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[4]])
def test_entry_points_agree(ctx, shape):
    V, S, Cc = shape
    rx = rc.antenna_lists(V)[2]
    window = rc.interior_window(S)
    cubes = rc.cubes(shape)
    p = pipeline(shape, ctx)
    try:
        want = p.capon_range_angle(rc.THETAS, rx, range_bins=window, delta=rc.DELTA, perform_windowing=False)
        whole = p.capon_range_angle(rc.THETAS, rx, delta=rc.DELTA)
    finally:
        p.bufs.free()
    assert whole.shape == (rc.F, S, len(rc.THETAS))
    bf = CaponBeamformer(rc.THETAS, delta=rc.DELTA, ctx=ctx)
    try:
        assert np.array_equal(bf.process_cube(cubes, rx, range_bins=window, perform_windowing=False), want)
        assert np.array_equal(bf.process_cube(cubes, rx), whole)
        one = bf.process_cube(cubes[1], rx, range_bins=window, perform_windowing=False)        # a single cube: [R_w, T]
        assert one.shape == want.shape[1:] and np.array_equal(one, want[1])
    finally:
        bf._bufs.free()
    mp = MultiDeviceFramePipeline(GridConfig(S, Cc), max_frames=rc.F, shape=shape, devices=[0])
    try:
        mp.load(cubes)
        assert np.array_equal(mp.capon_range_angle(rc.THETAS, rx, range_bins=window, delta=rc.DELTA, perform_windowing=False), want)
    finally:
        mp.close()


# ------------------------------------------------------------------------------------------------- 7. load_raw batch
def test_load_raw_batch_equals_load(ctx):
    shape = rc.SHAPES[1]
    V, S, Cc = shape
    cubes = rc.cubes(shape)
    num_tx = 3
    num_rx = V // num_tx
    raw = np.zeros((rc.F, num_rx, S, num_tx * Cc), dtype=np.complex64)
    for tx in range(num_tx):
        raw[:, :, :, tx::num_tx] = cubes[:, tx * num_rx:(tx + 1) * num_rx]
    rx, window = rc.ula(V)[:8], rc.interior_window(S)
    p = pipeline(shape, ctx)
    try:
        want = p.capon_range_angle(rc.THETAS, rx, range_bins=window)
        p.load_raw(raw, num_tx)
        assert np.array_equal(p.cubes(), cubes)
        assert np.array_equal(p.capon_range_angle(rc.THETAS, rx, range_bins=window), want)
    finally:
        p.bufs.free()


# ---------------------------------------------------------------------------------------------- 8. unsupported input
def test_more_than_1024_samples_is_unsupported_and_writes_nothing(ctx):
    shape = (2, 1025, 4)
    T, F = 5, 2
    p = FramePipeline(GridConfig(shape[1], shape[2]), max_frames=F, shape=shape, ctx=ctx)
    try:
        p.load(np.ones((F,) + shape, dtype=np.complex64))
        mark = np.full(F * 1025 * T, POISON, np.float32)
        d_res = p.bufs.get("capon_ra", mark.nbytes)
        d_res.upload(mark)
        with pytest.raises(_lib.MmwGpuError, match=f"status {_lib.MMW_ERR_UNSUPPORTED}"):
            p.capon_range_angle_device(np.linspace(-1, 1, T), [0, 1])
        assert p.d_capon is d_res
        assert np.array_equal(d_res.download(mark.shape, np.float32), mark)
        # straight through the C ABI as well, and the refusals leave the result alone too
        rx_arr, n_rx = _lib.int_array([0, 1])
        lib, h = ctx.lib, ctx.handle
        assert lib.mmw_range_snapshots(h, p.d_in.ptr, d_res.ptr, F, 2, 1025, 4, rx_arr, n_rx, 0, 4, 1) == _lib.MMW_ERR_UNSUPPORTED
        assert lib.mmw_range_snapshots(h, p.d_in.ptr, d_res.ptr, F, 2, 1024, 4, rx_arr, n_rx, 4, 4, 1) == _lib.MMW_ERR_INVALID
        bad, _ = _lib.int_array([0, 2])
        assert lib.mmw_range_snapshots(h, p.d_in.ptr, d_res.ptr, F, 2, 1024, 4, bad, 2, 0, 4, 1) == _lib.MMW_ERR_INVALID
        assert lib.mmw_range_snapshots(h, p.d_in.ptr, d_res.ptr, 0, 2, 1024, 4, rx_arr, n_rx, 0, 4, 1) == _lib.MMW_OK
        ctx.sync()
        assert np.array_equal(d_res.download(mark.shape, np.float32), mark)
    finally:
        p.bufs.free()
