"""Kernels that walk their work behind a grid capped by the CU count, driven past the first trip of that walk.

| test                                              | kernels, and the count that starts a second trip                          |
|---------------------------------------------------|---------------------------------------------------------------------------|
| chirpz_rows_..._doppler_azimuth, ..._range_zoom   | k_czt_rows<16> / <32> (mmw_czt.h): x = min(ceil(rows / IPW), max(1, 8 num_cu / |
|                                                   | n_seg)) row blocks, IPW = 16 / 8                                          |
| fused_float64_plane_reuses_its_tile               | k_rd_mag64_256x128 (mmw_cells64.h): min(n_frames, num_cu) workgroups      |
| widen_past_the_first_trip                         | k_widen_f32_f64: min(ceil(n / 256), 16 num_cu) workgroups                 |
| argmax_refinement_lists_past_the_first_trip       | k_angle_argmax_dets (> 1024 detections in a frame), k_argmax_refine_part  |
|                                                   | (> 512 entries), _finish (> 4 num_cu), _whole (> num_cu)                  |
| dense_argmax_list_past_the_first_trip             | k_argmax64_list: > 16 num_cu flagged evaluations                          |
| per_frame_argmax_kernels_past_128_detections      | k_angle_argmax, k_angle_argmax_lanes: > 128 detections in a frame         |
| detection_stage_loops_past_the_first_trip         | k_detect_insert (> 4 num_cu flagged frames), k_cfar_cell_exact (> 2 num_cu |
|                                                   | undecided cells), k_angle_argmax_recs (> 512 num_cu detections)           |

Every case asserts its precondition -- work items against the cap as the launch code computes it, from the shapes or from
the counts the entry hands back -- so a later change of a cap fails here instead of quietly un-testing the loop, then

  * the float64 reference at the bar the suite already holds the entry point to, and
  * equality with the same work submitted in a call small enough for one trip: the plan, the tables and the arithmetic
    per item are the same, so any difference is the loop's (a buffer or tile reused too early, a tail block, an item of a
    later trip read from the wrong place).  Where the outputs are indices compared exactly with the oracle on every
    entry (the two argmax-list tests), that comparison and the one across routes stand in for the single-trip call.

DESIGN.md, "Loops behind capped grids", lists every such loop and the test that crosses it.
"""
import ctypes as C
import os

import numpy as np
import pytest

from mmwave_radar_processing_amd import synth, _lib

pytestmark = pytest.mark.gpu
SPEC_TOL = 1e-5          # float32 spectra: max |gpu - ref| / max |ref| (tests/test_gpu_parity.py)
MAG64_TOL = 1e-12        # float64 |RD| planes, the same measure (test_mixed_radix_rd_kernel_all_shipped_shapes)


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@pytest.fixture(scope="module")
def num_cu():
    return _lib.device_info(0)["num_cu"]


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def czt_segments(freq, n_used):
    """(number of segments, runs as (offset, length, zero)) of a frequency list, from the library's own splitter."""
    runs = (C.c_int * (3 * (freq.size + 4)))()
    n = C.c_int(0)
    _lib.check(_lib.load_library().mmw_diag_czt_runs(dptr(freq), freq.size, n_used, runs, freq.size + 4, C.byref(n)))
    return n.value, [tuple(runs[3 * i:3 * i + 3]) for i in range(n.value)]


def czt_cap(num_cu, n_seg):
    return max(1, 8 * num_cu // n_seg)          # launch_czt_rows() in csrc/mmw_czt.h


def czt_length(n_used):
    """czt_length() of csrc/mmw_czt.h: the smallest of 256 / 1024 that leaves segments of at least 32 bins."""
    return 256 if n_used + 31 <= 256 else 1024 if n_used + 31 <= 1024 else 0


def chirpz_on():
    """MMW_ZOOM_DIRECT=1 in the environment sends both zoom entries to the direct kernels: nothing here would test k_czt_rows."""
    return os.environ.get("MMW_ZOOM_DIRECT", "0") in ("", "0")


def frames_for(rows_per_frame, ipw, cap, trips, at_least=2):
    """Smallest frame count whose rows need more than `trips` full strides of the capped grid plus a block, with a tail
    block that is not full."""
    F = at_least
    while not (-(-F * rows_per_frame // ipw) > trips * cap + 1 and (F * rows_per_frame) % ipw):
        F += 1
    return F


def zoom_lists(kind):
    rng = np.random.default_rng(31)
    if kind == "l256":
        # no two spacings equal: runs of one and two bins (36 bins give twenty segments; 24 would give fourteen); NaN
        # (zero-filled) bins alone, as a pair and at the end
        freq = np.sort(rng.uniform(-0.5, 0.5, 36))
        freq[[5, 17, 18, 35]] = np.nan
        return 40, 40, 278, freq        # 275 kept range rows: three frames of 4 x 275 rows cross two strides on 256 CUs
    # twenty runs of three bins, each with its own spacing; one of them NaN
    freq = np.concatenate([-0.45 + 0.045 * i + 0.001 * (i + 1) * np.arange(3) for i in range(20)])
    freq[27:30] = np.nan
    return 320, 300, 176, freq


@pytest.mark.parametrize("kind", ["l256", "l1024"])
def test_chirpz_rows_past_the_first_trip_doppler_azimuth(ctx, num_cu, kind):
    """mmw_doppler_azimuth_zoom with more than two strides of row blocks per segment and a partial tail block."""
    assert chirpz_on()
    Cc, n_used, S, freq = zoom_lists(kind)
    L = czt_length(n_used)
    assert L == {"l256": 256, "l1024": 1024}[kind]
    ipw = 256 // int(round(L ** 0.5))                   # rows per 256-thread workgroup: R = sqrt(L) threads per row
    V, A, s_lo, s_hi = 4, 64, 1, S - 2
    Sk, M = s_hi - s_lo, freq.size
    n_seg, runs = czt_segments(freq, n_used)
    assert n_seg >= 16 and any(z for _, _, z in runs) and any(not z for _, _, z in runs)
    cap = czt_cap(num_cu, n_seg)
    F = frames_for(V * Sk, ipw, cap, trips=2)
    rows = F * V * Sk
    blocks = -(-rows // ipw)
    assert blocks > 2 * cap + 1 and rows % ipw != 0            # three trips, and a tail
    assert -(-V * Sk // ipw) <= cap                             # one frame alone: a single trip
    print(f"{kind}: {n_seg} segments, cap {cap} blocks, {F} frames = {rows} rows = {blocks} blocks of {ipw}")
    cubes = np.stack([synth.synth_cube(1900 + f, (V, S, Cc)) for f in range(F)]).astype(np.complex64)
    frame_bytes = V * S * Cc * 8
    d_in, d_out = ctx.alloc(cubes.nbytes), ctx.alloc(F * M * A * 4)
    try:
        d_in.upload(cubes)
        d_out.upload(np.full(F * M * A, -7.0, np.float32))
        _lib.check(ctx.lib.mmw_doppler_azimuth_zoom(ctx.handle, d_in.ptr, d_out.ptr, F, V, S, Cc, A, s_lo, s_hi, n_used,
                                                    dptr(freq), M, 0))
        got = d_out.download((F, M, A), np.float32)
        # the frame whose rows straddle the end of the first trip, the first and the last, each alone (the range-mean
        # after the transform splits its rows the same way for 1 and for F frames: ceil(Sk / 4) partitions either way)
        straddle = (cap * ipw) // (V * Sk)
        assert straddle * V * Sk < cap * ipw < (straddle + 1) * V * Sk and 0 < straddle < F - 1
        for f in (0, straddle, F - 1):
            d_out.upload(np.full(M * A, -7.0, np.float32))
            _lib.check(ctx.lib.mmw_doppler_azimuth_zoom(ctx.handle, d_in.at(f * frame_bytes), d_out.ptr, 1, V, S, Cc, A, s_lo,
                                                        s_hi, n_used, dptr(freq), M, 0))
            assert np.array_equal(d_out.download((M, A), np.float32), got[f]), f"frame {f} alone differs from the batch"
    finally:
        d_in.free()
        d_out.free()
    nan = np.isnan(freq)
    Z = np.exp(-2j * np.pi * np.outer(np.where(nan, 0, freq), np.arange(n_used)))
    Z[nan] = 0
    worst = 0.0
    for f in range(F):
        x = cubes[f].astype(complex) * np.hanning(S)[None, :, None] * np.hanning(Cc)[None, None, :] * np.hanning(V)[:, None, None]
        r = np.fft.fft(x, axis=1)[:, s_lo:s_hi, :n_used]
        y = np.einsum("kc,vsc->skv", Z, r)
        ref = np.mean(np.abs(np.fft.fftshift(np.fft.fft(y, n=A, axis=2), axes=2)), axis=0)
        worst = max(worst, rel_err(got[f], ref))
        assert rel_err(got[f], ref) <= SPEC_TOL, f
        assert np.all(got[f][nan] == 0), f              # zero-filled bins: exactly 0 in every trip
    print(f"{kind}: worst deviation {worst:.2e} of the frame's peak")


def test_chirpz_rows_past_the_first_trip_range_zoom(ctx, num_cu):
    """mmw_range_zoom: rows = (frame, antenna), strided input (one chirp of the cube), 200 samples -> 1100 bins in twenty
    segments of the 256-point transform."""
    assert chirpz_on()
    V, S, Cc, m = 12, 200, 1, 1100
    assert czt_length(S) == 256
    ipw = 16
    f0, df = 0.0123, 0.00031
    freq = f0 + df * np.arange(m)
    n_seg, _ = czt_segments(freq, S)
    cap = czt_cap(num_cu, n_seg)
    F = frames_for(V, ipw, cap, trips=1, at_least=-(-2000 // V))
    rows = F * V
    assert n_seg == -(-m // (256 - S + 1)) and -(-rows // ipw) > cap + 1 and rows % ipw != 0      # a second trip, and a tail
    print(f"range zoom: {n_seg} segments, cap {cap} blocks, {rows} rows = {-(-rows // ipw)} blocks")
    rng = np.random.default_rng(41)
    cubes = (rng.standard_normal((F, V, S, Cc), dtype=np.float32)
             + 1j * rng.standard_normal((F, V, S, Cc), dtype=np.float32)).astype(np.complex64)
    cubes[:, :, :, 0] += (8 * np.exp(2j * np.pi * 0.2 * np.arange(S)))[None, None, :].astype(np.complex64)
    d_in, d_out = ctx.alloc(cubes.nbytes), ctx.alloc(F * m * 4)
    try:
        d_in.upload(cubes)
        _lib.check(ctx.lib.mmw_range_zoom(ctx.handle, d_in.ptr, d_out.ptr, F, V, S, Cc, 0, m, f0, df))
        got = d_out.download((F, m), np.float32)
        edge = (cap * ipw) // V              # the frame that holds the first row of the second trip, and the one before
        for f in (0, edge - 1, edge, F - 1):
            _lib.check(ctx.lib.mmw_range_zoom(ctx.handle, d_in.at(f * V * S * Cc * 8), d_out.ptr, 1, V, S, Cc, 0, m, f0, df))
            assert np.array_equal(d_out.download((m,), np.float32), got[f]), f"frame {f} alone differs from the batch"
    finally:
        d_in.free()
        d_out.free()
    Z = np.exp(-2j * np.pi * np.outer(np.arange(S), freq))
    x = cubes[:, :, :, 0].astype(complex) * np.hanning(S)[None, None, :]
    ref = np.mean(np.abs(x.reshape(F * V, S) @ Z).reshape(F, V, m), axis=1)
    errs = np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref), axis=1)
    print(f"range zoom: worst deviation {errs.max():.2e} of the frame's peak")
    assert np.all(errs <= SPEC_TOL), int(np.argmax(errs))


def test_widen_past_the_first_trip(ctx, num_cu):
    """k_widen_f32_f64: min(ceil(n / 256), 16 num_cu) workgroups of 256 threads striding over n floats.  Two full strides
    and a tail of 77; the conversion is exact, so the float64 reference and the single-trip call are one comparison."""
    stride = 16 * num_cu * 256
    n = 2 * stride + 77
    assert -(-n // 256) > 2 * 16 * num_cu
    rng = np.random.default_rng(61)
    x = rng.standard_normal(n, dtype=np.float32)
    x[[0, stride - 1, stride, 2 * stride, n - 1]] = [np.float32(1e-45), -0.0, np.inf, np.float32(3.4e38), np.float32(-1e-40)]
    d_in, d_out = ctx.alloc(x.nbytes), ctx.alloc(n * 8 + 64)
    try:
        d_in.upload(x)
        d_out.upload(np.full(n + 8, -7.0))
        _lib.check(ctx.lib.mmw_widen_f32_f64(ctx.handle, d_in.ptr, d_out.ptr, n))
        got = d_out.download((n + 8,), np.float64)
        _lib.check(ctx.lib.mmw_widen_f32_f64(ctx.handle, d_in.at(4 * (2 * stride)), d_out.ptr, 77))      # the tail alone
        tail = d_out.download((77,), np.float64)
    finally:
        d_in.free()
        d_out.free()
    want = x.astype(np.float64)
    assert np.array_equal(got[:n], want) and np.array_equal(np.signbit(got[:n]), np.signbit(want))
    assert np.all(got[n:] == -7.0)                      # nothing written past the end
    assert np.array_equal(tail, want[2 * stride:])


def test_fused_float64_plane_reuses_its_tile(ctx, num_cu):
    """k_rd_mag64_256x128: min(n_frames, num_cu) workgroups, each taking frame after frame through one scratch tile and
    one LDS slab.  2 num_cu + 3 frames: every workgroup takes a second frame, three of them a third."""
    V, S, Cc = 1, 256, 128
    F = 2 * num_cu + 3
    assert F > 2 * min(F, num_cu) and os.environ.get("MMW_RD64_FUSED", "1") != "0"
    rng = np.random.default_rng(51)
    raw = rng.integers(-2048, 2048, (F, S, Cc, 2), dtype=np.int16)          # integer-valued samples, as an ADC gives them
    cubes = raw.astype(np.float32).view(np.complex64).reshape(F, V, S, Cc)
    del raw
    plane = S * Cc
    picks = [0, num_cu - 1, num_cu, 2 * num_cu, F - 1, 1, num_cu + 1, F - 2]        # eight frames: the fused kernel's minimum
    d_in, d_mag, d_in8 = ctx.alloc(cubes.nbytes), ctx.alloc(F * plane * 8), ctx.alloc(8 * plane * 8)
    try:
        d_in.upload(cubes)
        d_in8.upload(cubes[picks])
        d_mag.zero()
        _lib.check(ctx.lib.mmw_range_doppler_mag64(ctx.handle, d_in.ptr, d_mag.ptr, F, V, S, Cc, 0))
        got = d_mag.download((F, S, Cc), np.float64)
        ctx.set_option("MMW_RD64_FUSED", 0)
        try:
            d_mag.zero()
            _lib.check(ctx.lib.mmw_range_doppler_mag64(ctx.handle, d_in.ptr, d_mag.ptr, F, V, S, Cc, 0))
            unfused = d_mag.download((F, S, Cc), np.float64)
        finally:
            ctx.set_option("MMW_RD64_FUSED", None)
        _lib.check(ctx.lib.mmw_range_doppler_mag64(ctx.handle, d_in8.ptr, d_mag.ptr, 8, V, S, Cc, 0))
        got8 = d_mag.download((8, S, Cc), np.float64)
    finally:
        for b in (d_in, d_mag, d_in8):
            b.free()
    for i, f in enumerate(picks):
        assert np.array_equal(got8[i], got[f]), f"frame {f} in a single-trip batch differs from the {F}-frame batch"
    win = np.hanning(S)[:, None] * np.hanning(Cc)[None, :]
    worst = worst_u = 0.0
    for f0 in range(0, F, 32):
        x = cubes[f0:f0 + 32, 0].astype(np.complex128) * win
        ref = np.abs(np.fft.fftshift(np.fft.fft2(x, axes=(-2, -1)), axes=-1))
        peak = ref.max(axis=(1, 2))
        e = np.abs(got[f0:f0 + 32] - ref).max(axis=(1, 2)) / peak
        eu = np.abs(unfused[f0:f0 + 32] - ref).max(axis=(1, 2)) / peak
        worst, worst_u = max(worst, e.max()), max(worst_u, eu.max())
        assert np.all(e <= MAG64_TOL), f0 + int(np.argmax(e))
        assert np.all(eu <= MAG64_TOL), f0 + int(np.argmax(eu))
    print(f"{F} frames: fused {worst:.2e}, MMW_RD64_FUSED=0 (the single-pass mixed-radix kernel) {worst_u:.2e} of the frame's peak")


def _refine_case(name, seed, F, cap, counts):
    import refine_cases as rc
    return rc.Case(name, seed, (F, 4, 64, 128), cap, counts, "random")


def test_argmax_refinement_lists_past_the_first_trip(ctx, num_cu):
    """mmw_angle_argmax_exact on a list of 1100 + 10 flagged evaluations (tests/refine_cases.py: every evaluation is
    flagged by construction), direct and whole-plane routes:
      k_angle_argmax_dets    min(ceil(cap / 256), 4) workgroups of 256 detections per frame: 1100 > 1024 in frame 0
      k_argmax_refine_part   min(n_split, 512) workgroups per slice, one entry each: 1110 > 512
      k_argmax_refine_finish min(ceil(n_split / 4), num_cu) workgroups of four entries: 1110 > 4 num_cu
      k_argmax_refine_whole  num_cu workgroups, one entry each: 1110 > num_cu
    The outputs are indices: equality with the oracle's is the bit-exact comparison (evaluations whose two best bins lie
    within MARGIN_MIN are excluded by the builders, as in test_gpu_argmax_refine.py); it and the comparison between the two
    routes, whose grids and trip counts differ, stand in for a single-trip call."""
    import test_gpu_argmax_refine as ar
    case = _refine_case("second_trip_direct", 7300, 2, 1104, [1100, 10])
    assert case.n_evals > 4 * num_cu and case.n_evals > 512 and case.counts[0] > 1024 and case.cap > 1024
    with ar.Resident(ctx, case) as res:
        ar.check_indices(res, (0, 1, 2, 3), 1, ("direct", "whole"))


def test_dense_argmax_list_past_the_first_trip(ctx, num_cu):
    """k_argmax64_list: min(max(dense_cap / 4, 1), 4 num_cu) workgroups of four waves, one flagged evaluation per wave,
    dense_cap = min(frames x cap, 256 frames).  A wave takes a second evaluation only above 16 num_cu flagged evaluations
    in a call of more than num_cu / 16 frames: num_cu / 16 + 2 frames of 250 evaluations each, all on the dense route.
    Indices are compared exactly with the oracle and with the direct route (no k_argmax64_list at all), which stands in
    for a single-trip call."""
    import test_gpu_argmax_refine as ar
    F = num_cu // 16 + 2
    case = _refine_case("second_trip_dense", 7400, F, 256, [250] * F)
    dense_cap = min(F * case.cap, 256 * F)
    assert 16 * num_cu < case.n_evals <= dense_cap and dense_cap // 4 > 4 * num_cu
    with ar.Resident(ctx, case) as res:
        ar.check_indices(res, (0, 1, 2, 3), 1, ("dense", "direct"))


def test_per_frame_argmax_kernels_past_128_detections(ctx):
    """k_angle_argmax (mmw_argmax.h; what mmw_angle_argmax runs) and k_angle_argmax_lanes (mmw_detect.h; the first pass of
    mmw_angle_argmax_exact under MMW_ARGMAX_FORM=0) launch x = min(ceil(cap / 4), 32) workgroups of four waves per frame,
    one detection per wave (a cap on detections per frame, not a CU cap): a wave takes a second detection above 128 in
    ONE frame.  200 detections in frame 0, 9 in frame 1.
      k_angle_argmax: float32 indices against oracle_np.angle_argmax on noise cells whose two best bins are at least 1e-4
        apart (the float32 range-Doppler cells are held to 1e-5 of the PLANE's peak by the suite; near-ties are not this
        kernel's to decide), and detections 128 .. 199 resubmitted alone (72 < 128: one trip) give the very same indices.
      k_angle_argmax_lanes: on a list where every evaluation is flagged by construction, n_refined == evaluations says
        every detection of the second trip was evaluated and flagged, and the indices equal the oracle's and the default
        form's (k_angle_argmax_dets, one trip at 200)."""
    import refine_cases as rc
    import test_gpu_argmax_refine as ar
    ants, n_first = (0, 1, 2, 3), 128
    plain = rc.Case("plain_noise", 7500, (2, 4, 64, 128), 200, [200, 9], "random", P=0.0)
    assert plain.counts[0] > n_first and -(-plain.cap // 4) >= 32
    arr, n_ant = _lib.int_array(ants)
    with ar.Resident(ctx, plain) as res:
        b = res.bufs
        b["idx"].upload(np.full((2, 200), ar.SENTINEL, np.int32))
        _lib.check(ctx.lib.mmw_angle_argmax(ctx.handle, b["rd"].ptr, b["dets"].ptr, b["counts"].ptr, b["idx"].ptr, 2, 4, 64, 128, 200,
                                            arr, n_ant, rc.A_BINS, 1))
        got = b["idx"].download((2, 200), np.int32)
        # the second trip's detections of frame 0 as a list of their own
        tail = np.full((2, 200, 2), -12345, np.int32)
        tail[0, :72] = plain.dets[0, n_first:200]
        b["dets"].upload(tail)
        b["counts"].upload(np.array([72, 0], np.int32))
        b["idx"].upload(np.full((2, 200), ar.SENTINEL, np.int32))
        _lib.check(ctx.lib.mmw_angle_argmax(ctx.handle, b["rd"].ptr, b["dets"].ptr, b["counts"].ptr, b["idx"].ptr, 2, 4, 64, 128, 200,
                                            arr, n_ant, rc.A_BINS, 1))
        alone = b["idx"].download((2, 200), np.int32)
    assert np.array_equal(alone[0, :72], got[0, n_first:200])
    assert np.all(alone[0, 72:] == ar.SENTINEL) and np.all(got[1, 9:] == ar.SENTINEL)
    compared = 0
    for f, n in ((0, 200), (1, 9)):
        want, resp = O_angle_argmax(plain, f, n, ants)
        top = np.sort(resp, axis=1)[:, -2:]
        clear = (top[:, 1] - top[:, 0]) >= 1e-4 * top[:, 1]
        compared += int(clear[n_first:].sum()) if f == 0 else 0
        assert np.array_equal(got[f, :n][clear], want[clear]), f
    assert compared >= 60                                   # most of the second trip is compared with the oracle
    flagged = _refine_case("second_trip_lanes", 7600, 2, 200, [200, 9])
    with ar.Resident(ctx, flagged) as res:
        want, excl, _ = flagged.expected(ants, 1)
        direct = {"MMW_ARGMAX_DENSE_MIN": 1 << 30}
        rc_l, n_l, idx_l = res.argmax(ants, 1, dict(direct, MMW_ARGMAX_FORM=0))
        rc_d, n_d, idx_d = res.argmax(ants, 1, direct)
    assert rc_l == rc_d == _lib.MMW_OK and n_l == n_d == flagged.n_evals == 209
    cmp = (want >= 0) & ~excl
    assert np.array_equal(idx_l[cmp], want[cmp]) and np.array_equal(idx_d[cmp], want[cmp])
    assert np.all(idx_l[want < 0] == ar.SENTINEL)


def O_angle_argmax(case, f, n, ants):
    from oracle import oracle_np as O
    return O.angle_argmax(case.rd(f), case.dets[f, :n, 0], case.dets[f, :n, 1], list(ants), 64, True)


def _detect_points(ctx, d_in, F, shape, cfar, cap, az, el):
    import test_gpu_parity as par
    return par._detect_points_raw(ctx, d_in, F, shape, cfar, cap, az, el)


def test_detection_stage_loops_past_the_first_trip(ctx, num_cu):
    """One mmw_detect_points call on F = 4 num_cu + 1500 frames of 4 x 64 x 32 with a loose CA-CFAR (pfa 0.2) and the
    screening band widened (MMW_DETECT_BAND_MULT), sized from the counts the entry hands back in h_stats and d_counts:
      k_detect_insert      min(n_frames, 4 num_cu) workgroups, one FLAGGED frame per trip (a frame with undecided cells that
                           was not handed back: stats[0] counts exactly those): stats[0] > 4 num_cu
      k_cfar_cell_exact    min(cell_cap, 2 num_cu) workgroups, one undecided cell per trip:  stats[1] > 2 num_cu
      k_angle_argmax_recs  min(ceil(frames cap / 256), 2 num_cu) workgroups of 256 records, one record per detection:
                           sum(counts) > 512 num_cu
    Detections (values and order) and both index arrays are identical to the float64 path (mmw_detect_batch +
    mmw_angle_argmax_exact) on every frame not handed back -- the bar test_detect_points_screening_equals_the_float64_path
    holds the stage to -- and to the oracle on three frames; 16 frames from the middle of the batch submitted alone (at
    most 16 flagged frames, a few hundred cells and a few thousand records, asserted below the caps: one trip each) give the same arrays."""
    import test_gpu_parity as par
    from mmwave_radar_processing_amd.detectors import CaCFAR2D
    from oracle import oracle_np as O
    shape, cap = (4, 64, 32), 256
    V, S, C = shape
    F = 4 * num_cu + 1500
    cfar = CaCFAR2D((4, 4), (2, 2), 0.2)
    az, el = [0, 1, 2, 3], [2, 3]
    frame_bytes = V * S * C * 8
    d_in = ctx.alloc(F * frame_bytes)
    try:
        _lib.check(ctx.lib.mmw_synth_cubes(ctx.handle, d_in.ptr, F, V, S, C, 515151, 8, 30.0))
        assert ctx.lib.mmw_detect_points_supported(S, C, cfar.kind, 4, 4, 2, 2, len(az), len(el), 64) == 1
        ref = par._detect_float64_raw(ctx, d_in, F, shape, cfar, cap, az, el)
        f0 = F // 2
        try:
            ctx.set_option("MMW_DETECT_BAND_MULT", 10)
            got = par._detect_points_raw(ctx, d_in, F, shape, cfar, cap, az, el)
            sub = par._detect_points_raw(ctx, _Offset(d_in, f0 * frame_bytes), 16, shape, cfar, cap, az, el)
        finally:
            ctx.set_option("MMW_DETECT_BAND_MULT", None)
        cubes3 = [d_in.download(shape, np.complex64, f * frame_bytes) for f in (0, F // 2 + 1, F - 1)]
    finally:
        d_in.free()
    stats, keep = got[4], got[0] >= 0
    records = int(got[0][keep].sum())
    print(f"{F} frames: {stats[0]} flagged frames (cap {4 * num_cu}), {stats[1]} undecided cells (cap {2 * num_cu}), {records} records "
          f"(cap {512 * num_cu}), {stats[2]} frames handed back, {stats[3]} + {stats[4]} evaluations refined")
    assert np.all(ref[0] <= cap) and np.all(ref[0] >= 0)
    assert stats[0] > 4 * num_cu
    assert stats[1] > 2 * num_cu
    assert records > 512 * num_cu and -(-F * cap // 256) > 2 * num_cu
    assert keep.sum() == F - stats[2] and stats[2] <= F // 4
    par._same_points(tuple(x[keep] for x in got[:4]), tuple(x[keep] for x in ref))
    k64 = keep[f0:f0 + 16] & (sub[0] >= 0)
    assert k64.sum() >= 12 and sub[4][0] <= 4 * num_cu and sub[4][1] <= 2 * num_cu
    par._same_points(tuple(x[k64] for x in sub[:4]), tuple(x[f0:f0 + 16][k64] for x in got[:4]))
    for f, cube in zip((0, F // 2 + 1, F - 1), cubes3):
        if not keep[f]:
            continue
        raw, _, dets_ref, _, _ = O.rd_detect_2d(cube, (4, 4), (2, 2), 0.2)
        k = int(got[0][f])
        np.testing.assert_array_equal(got[1][f, :k], dets_ref)
        r, v = dets_ref[:, 0].astype(int), dets_ref[:, 1].astype(int)
        np.testing.assert_array_equal(got[2][f, :k], O.angle_argmax(raw, r, v, az, 64, True)[0])
        np.testing.assert_array_equal(got[3][f, :k], O.angle_argmax(raw, r, v, el, 64, False)[0])


class _Offset:
    """A view of a device buffer from a byte offset on (for helpers that take a buffer's .ptr)."""

    def __init__(self, buf, off):
        self.ptr = buf.at(off)
