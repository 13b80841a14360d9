"""Capon point clouds over resident frames on the GPU: FramePipeline.capon_point_clouds and mmw_capon_doppler under it.

Inputs and the float64 NumPy restatement: tests/capon_points_cases.py (tests/test_capon_points_host.py checks the host twin of
the kernel against it without a GPU).  Tolerances are the issue's: |z| within 1e-9 of the detection's peak (cond(R) n eps is about
6e-11 for delta = 1e-3, n <= 16), the Doppler bin identical wherever the restatement's two largest |z| differ by more than 1e-8
relatively -- and no detection of these seeds lies inside that band.

| test                         | what would make it fail                                                                          |
|------------------------------|--------------------------------------------------------------------------------------------------|
| pipeline against restatement | a stage reading another layout than the one before it writes; a wrong weight, window or bin       |
| device equals host twin      | the kernel summing in another order than the shared arithmetic, a lane taking another lane's cell |
| empty and overflowing frames | a frame without detections disturbing its neighbours; an overflow not reported as detect() does   |
| pass size                    | a wrong slice offset per pass, the snapshot buffer reused too early                               |
| one target                   | the sign of theta, the Doppler shift or the range offset disagreeing with PointCloudGenerator     |
| multi-device                 | the sharded form making other calls than the pipeline                                             |
| hand-off                     | lists ego_velocities does not accept                                                              |
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capon_points_cases as cc
from egovel_cases import Geometry, rel_err, cases as ego_cases
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from mmwave_radar_processing_amd.detectors import CaCFAR2D, OsCFAR2D
from mmwave_radar_processing_amd.point_cloud_processing import VelocityEstimator
from mmwave_radar_processing_amd.processors.steering_beamformers import CaponBeamformer

pytestmark = pytest.mark.gpu

RX = list(range(8))
F = 3
# (shape, seed): 12x32x16 takes the FFT snapshot path, 12x24x10 the direct one (S and K no powers of two)
SHAPES = (((12, 32, 16), 21), ((12, 24, 10), 22))
SHAPE_IDS = ["x".join(map(str, s)) for s, _ in SHAPES]
DETECTORS = {"ca": lambda: CaCFAR2D((2, 3), (1, 1), 1e-3), "os": lambda: OsCFAR2D((2, 3), (1, 1), 0.7, 6.0)}


class GridConfig:
    """The scalars FramePipeline reads: S range bins 1 m apart, C velocity bins 1 m/s apart."""

    def __init__(self, S, C):
        self.range_res_m, self.range_max_m = 1.0, float(S)
        self.vel_res_m_s, self.vel_max_m_s = 1.0, C / 2
        self.frameCfg_periodicity_ms = 50.0


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def pipeline(shape, n_frames, cap=256, **kw):
    return FramePipeline(GridConfig(shape[1], shape[2]), max_frames=n_frames, shape=shape, det_capacity=cap, **kw)


@functools.lru_cache(maxsize=None)
def run(shape, seed, kind, r_lo, frames_per_pass=None):
    """One capon_point_clouds call, shared by the tests: everything it returns and leaves behind, downloaded once."""
    V, S, K = shape
    pipe = pipeline(shape, F)
    pipe.load(cc.cubes(shape, F, seed))
    window = (r_lo, S)
    pcs = pipe.capon_point_clouds(cc.THETAS, RX, DETECTORS[kind](), range_bins=window, delta=cc.DELTA,
                                  frames_per_pass=frames_per_pass)
    Rw, T = S - r_lo, len(cc.THETAS)
    maps = pipe.d_capon.download((F, Rw, T), np.float32).astype(np.float64)
    # the snapshot buffer holds the last pass only: the snapshots of every frame are made again here (the same call, bit for bit)
    rx_arr, n_rx = _lib.int_array(RX)
    d_all = pipe.ctx.alloc(F * len(RX) * Rw * K * 8)
    _lib.check(pipe.ctx.lib.mmw_range_snapshots(pipe.ctx.handle, pipe.d_in.ptr, d_all.ptr, F, V, S, K, rx_arr, n_rx, r_lo, S, 1))
    X = d_all.download((F, len(RX), Rw, K), np.complex64).copy()
    d_all.free()
    return dict(pcs=pcs, dets=pipe.capon_dets, dop=pipe.capon_doppler_idx, peak=pipe.capon_peak, counts=pipe.capon_counts.copy(),
                maps=maps, X=X, range_bins=pipe.range_bins.copy(), vel_bins=pipe.vel_bins.copy(), window=window)


# ------------------------------------------------------------------------------------- 1. the pipeline against the restatement
@pytest.mark.parametrize("r_lo", [0, 1])
@pytest.mark.parametrize("kind", ["ca", "os"])
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_pipeline_against_detector_and_restatement(case, kind, r_lo):
    shape, seed = case
    out = run(shape, seed, kind, r_lo)
    det = DETECTORS[kind]()
    n_found = 0
    for f in range(F):
        want_dets = np.array(det.detect(out["maps"][f]), dtype=np.int64).reshape(-1, 2)
        got = out["dets"][f]
        assert got.dtype == np.int64 and np.array_equal(got - np.array([r_lo, 0]), want_dets)       # same cells, same order
        assert len(got) == out["counts"][f] and len(got) > 0
        dop, peak, spec = cc.doppler_reference(out["X"][f], want_dets, cc.THETAS, cc.DELTA, True)
        gaps = np.array([cc.top_two_gap(s) for s in spec])
        assert np.all(gaps > cc.DOP_BAND), f"frame {f}: a detection of this seed lies inside the Doppler band"
        assert np.array_equal(out["dop"][f], dop)
        err = np.max(np.abs(out["peak"][f] - peak) / peak)
        print(f"{shape} {kind} r_lo {r_lo} frame {f}: {len(got)} detections, peak error {err:.2e}, smallest gap {gaps.min():.1e}")
        assert err <= cc.SPEC_TOL
        rows = out["range_bins"][r_lo:]
        ref_pts = cc.points_reference(want_dets, dop, cc.THETAS, rows, out["vel_bins"])
        assert np.array_equal(out["pcs"][f], ref_pts)       # one rounding per product on tables made on the host: bit for bit
        assert out["pcs"][f].shape == (len(got), 4) and out["pcs"][f].dtype == np.float64
        cells = {(int(q), int(t)) for q, t in got}
        for r0, fd, th0 in cc.targets_of(shape, seed + f):
            t0 = int(np.argmin(np.abs(cc.THETAS - th0)))
            if 3 <= r0 - r_lo < shape[1] - r_lo - 3 and (r0, t0) in cells:       # inside the CFAR's valid rows
                n_found += 1
    assert n_found >= 2 * F     # the CFAR finds the targets (the restatement on the host finds all 3 per frame)


# ------------------------------------------------------------------------------------- 2. the device entry against its host twin
@pytest.mark.parametrize("windowing", [1, 0])
@pytest.mark.parametrize("case", cc.HOST_SHAPES + ((8, 40, 128, 31), (16, 3, 512, 32)), ids=lambda c: "x".join(map(str, c[:3])))
def test_device_entry_equals_host_twin_bit_for_bit(case, windowing):
    """Spectra, points, Doppler bins and peaks of mmw_capon_doppler against mmw_diag_capon_doppler_host on the same snapshots and
    detection lists: the shapes of the host tests, K = 128 with more rows than one pass of the list holds detections in (cap 300:
    two passes of 256), K = 512 with n = 16 (the largest LDS image, one detection per chunk).  The lists hold a degenerate row, a
    detection outside the map and a count above cap."""
    n, R, K, seed = case
    ctx = _lib.default_context()
    lib = ctx.lib
    X = np.array(cc.host_snapshots(n, R, K, seed))
    Fn = X.shape[0]
    if R >= 3:
        X[1, :, 1, :] = 0                                    # frame 1, row 1: degenerate
    cap = 300 if K == 128 else 24
    if K == 128:
        rng = np.random.default_rng(5)
        dets = np.stack([rng.integers(0, R, (Fn, cap)), rng.integers(0, cc.T_ANGLES, (Fn, cap))], axis=-1).astype(np.int32)
        dets[0] = dets[0][np.lexsort((dets[0][:, 1], dets[0][:, 0]))]       # frame 0 row-major, frame 1 in any order
        counts = np.array([cap + 7, cap - 5], np.int32)                     # frame 0 above cap: clamped
    else:
        dets, counts = cc.host_dets(n, R, K, seed)
        dets = dets.copy()
    dets[1, 0] = (R, 0)                                      # outside the map
    dets[1, 2] = (0, -1)
    rows, vel = cc.tables(R, K)
    th = cc.THETAS.copy()
    host = [np.full((Fn, cap), 9, np.int32), np.full((Fn, cap), 9.0), np.full((Fn, cap, K), 9.0), np.full((Fn, cap, 4), 9.0)]
    assert lib.mmw_diag_capon_doppler_host(X.ctypes.data, dets.ctypes.data, counts.ctypes.data, dptr(th), *(a.ctypes.data for a in host),
                                           rows.ctypes.data, vel.ctypes.data, Fn, n, R, K, len(th), cap, cc.DELTA, windowing) == 0
    bufs = [ctx.alloc(a.nbytes) for a in (X, dets, counts, rows, vel)]
    for b, a in zip(bufs, (X, dets, counts, rows, vel)):
        b.upload(a)
    outs = [ctx.alloc(a.nbytes) for a in host]
    for b, a in zip(outs, host):
        b.upload(np.full_like(a, 5))
    _lib.check(lib.mmw_capon_doppler(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, dptr(th), *(b.ptr for b in outs), bufs[3].ptr,
                                     bufs[4].ptr, Fn, n, R, K, len(th), cap, cc.DELTA, windowing))
    got = [b.download(a.shape, a.dtype).copy() for b, a in zip(outs, host)]
    for b in bufs + outs:
        b.free()
    for name, g, h in zip(("dop", "peak", "spec", "points"), got, host):
        assert np.array_equal(g, h, equal_nan=g.dtype != np.int32), name
    dop, peak = got[0], got[1]
    assert dop[1, 0] == -1 and np.isnan(peak[1, 0]) and dop[1, 2] == -1 and np.all(np.isnan(got[3][1, 0, [0, 1, 3]]))
    nf = np.minimum(counts, cap)
    if R >= 3:
        deg = np.nonzero((dets[1, :nf[1], 0] == 1) & (dets[1, :nf[1], 1] >= 0))[0]
        assert len(deg) > 0 and np.all(dop[1, deg] == -1) and np.all(np.isnan(peak[1, deg]))
        assert np.all(np.isfinite(got[3][1, deg, :2])) and np.all(np.isnan(got[3][1, deg, 3]))
    for f in range(Fn):
        assert np.all(dop[f, nf[f]:] == 0) and np.all(peak[f, nf[f]:] == 0) and np.all(got[2][f, nf[f]:] == 0)
        assert np.all(got[3][f, nf[f]:] == 0)
    ok = dop[0, :nf[0]] >= 0
    assert np.all(ok) and np.all(np.isfinite(peak[0, :nf[0]]))


def test_beamformed_doppler_api_against_restatement():
    n, R, K, seed = cc.HOST_SHAPES[0]
    X = cc.host_snapshots(n, R, K, seed)
    dets, counts = cc.host_dets(n, R, K, seed)
    lists = [dets[f, :counts[f]] for f in range(len(X))]
    bf = CaponBeamformer(cc.THETAS, cc.DELTA)
    dop, peak, spec = bf.beamformed_doppler(X, lists, return_spectra=True)
    for f in range(len(X)):
        rd, rp, rs = cc.doppler_reference(X[f], lists[f], cc.THETAS, cc.DELTA, True)
        assert np.array_equal(dop[f], rd) and dop[f].dtype == np.int64
        assert np.max(np.abs(spec[f] - rs) / rp[:, None]) <= cc.SPEC_TOL and np.max(np.abs(peak[f] - rp) / rp) <= cc.SPEC_TOL
    d1, p1 = bf.beamformed_doppler(X[0], lists[0], doppler_windowing=False)
    rd, rp, _ = cc.doppler_reference(X[0], lists[0], cc.THETAS, cc.DELTA, False)
    assert np.array_equal(d1, rd) and np.max(np.abs(p1 - rp) / rp) <= cc.SPEC_TOL
    d0, p0 = bf.beamformed_doppler(X[0], np.zeros((0, 2), int))
    assert d0.shape == (0,) and p0.shape == (0,)


# ------------------------------------------------------------------------------------- 3. empty and overflowing frames
def test_frame_without_detections_and_overflow():
    shape, seed = SHAPES[0]
    cubes = np.array(cc.cubes(shape, F, seed))
    quiet = cc.cubes(shape, 1, 99, amplitude=0.0, noise_sigma=2.0)[0]
    cubes[1] = quiet
    det = CaCFAR2D((2, 3), (1, 1), 1e-30)            # 140 times the local mean: noise alone does not cross it, a target does
    pipe = pipeline(shape, F)
    pipe.load(cubes)
    pcs = pipe.capon_point_clouds(cc.THETAS, RX, det, delta=cc.DELTA)
    assert pcs[1].shape == (0, 4) and pipe.capon_dets[1].shape == (0, 2) and pipe.capon_counts[1] == 0
    assert len(pcs[0]) > 0 and len(pcs[2]) > 0
    alone = pipeline(shape, 1)
    alone.load(cubes[2:3])
    assert np.array_equal(alone.capon_point_clouds(cc.THETAS, RX, det, delta=cc.DELTA)[0], pcs[2])
    small = pipeline(shape, F, cap=2)
    small.load(cubes)
    with pytest.raises(_lib.MmwGpuError, match="detection capacity 2 exceeded"):
        small.capon_point_clouds(cc.THETAS, RX, det, delta=cc.DELTA)
    assert small.capon_counts.max() == max(len(p) for p in pcs)         # the counts stay exact


# ------------------------------------------------------------------------------------- 4. pass size
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_result_does_not_depend_on_the_pass_size(case):
    shape, seed = case
    one, each = run(shape, seed, "ca", 0), run(shape, seed, "ca", 0, 1)
    for key in ("pcs", "dets", "dop", "peak"):
        for a, b in zip(one[key], each[key]):
            assert np.array_equal(a, b), key
    assert np.array_equal(one["maps"], each["maps"])


# ------------------------------------------------------------------------------------- 5. one target: sign, range and Doppler
def test_one_target_agrees_with_the_fft_point_cloud():
    """A single strong target: the Capon point and PointCloudGenerator's (FramePipeline.point_clouds on the same cube, azimuth from
    the angle FFT over the same antennas) agree in range bin and Doppler bin, in the sign of the azimuth, and in azimuth within one
    step of the coarser grid (64 FFT bins over sin(theta) in [-1, 1]: up to 7.3 degrees at 60 degrees; the Capon grid: 3.75)."""
    shape = (12, 32, 16)
    V, S, K = shape
    for th0_deg in (-25.0, 32.0):
        th0, r0, fd = np.deg2rad(th0_deg), 11, 3.2
        rng = np.random.default_rng(3)
        v, s, c = np.arange(V)[:, None, None], np.arange(S)[None, :, None], np.arange(K)[None, None, :]
        x = 2.0 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        x = x + 300.0 * np.exp(1j * (2 * np.pi * (r0 * s / S + fd * c / K) - np.pi * v * np.sin(th0)))
        cube = (np.rint(x.real) + 1j * np.rint(x.imag)).astype(np.complex64)[None]
        pipe = pipeline(shape, 1, az_antenna_idxs=RX, cfar=CaCFAR2D((2, 2), (1, 1), 1e-3))
        pipe.load(cube)
        fft_pts = pipe.point_clouds()[0]
        fft_dets = pipe.dets[0]
        j = [i for i, d in enumerate(fft_dets) if tuple(d) == (r0, int(np.rint(fd)) + K // 2)]
        assert len(j) == 1
        fft_az = np.arctan2(fft_pts[j[0], 1], fft_pts[j[0], 0])
        pcs = pipe.capon_point_clouds(cc.THETAS, RX, CaCFAR2D((2, 3), (1, 1), 1e-3), delta=cc.DELTA)[0]
        k = int(np.argmax(pipe.capon_peak[0]))                  # the strongest Capon detection is the target's cell
        assert pipe.capon_dets[0][k, 0] == r0 and pipe.capon_doppler_idx[0][k] == fft_dets[j[0], 1]
        capon_az = np.arctan2(pcs[k, 1], pcs[k, 0])
        assert np.isclose(capon_az, cc.THETAS[pipe.capon_dets[0][k, 1]], rtol=0, atol=1e-12)
        i = int(np.argmin(np.abs(pipe.angle_bins - fft_az)))
        step = max(np.max(np.abs(np.diff(pipe.angle_bins[i - 1:i + 2]))), np.max(np.diff(cc.THETAS)))
        print(f"target at {th0_deg} deg: FFT azimuth {np.rad2deg(fft_az):.2f}, Capon azimuth {np.rad2deg(capon_az):.2f}")
        assert np.sign(capon_az) == np.sign(fft_az) == np.sign(th0) and abs(capon_az - fft_az) <= step
        assert pcs[k, 3] == fft_pts[j[0], 3] and np.isclose(np.hypot(pcs[k, 0], pcs[k, 1]), pipe.range_bins[r0])


# ------------------------------------------------------------------------------------- 6. multi-device, 7. hand-off
def test_multi_device_equals_single_device():
    shape, seed = SHAPES[0]
    want = run(shape, seed, "ca", 0)
    mp = MultiDeviceFramePipeline(GridConfig(shape[1], shape[2]), max_frames=F, shape=shape, devices=[0], det_capacity=256)
    try:
        mp.load(cc.cubes(shape, F, seed))
        pcs = mp.capon_point_clouds(cc.THETAS, RX, DETECTORS["ca"](), delta=cc.DELTA)
        for key, got in (("pcs", pcs), ("dets", mp.capon_dets), ("dop", mp.capon_doppler_idx), ("peak", mp.capon_peak)):
            assert len(got) == F
            for a, b in zip(got, want[key]):
                assert np.array_equal(a, b), key
    finally:
        mp.close()


def test_point_clouds_are_accepted_by_ego_velocities():
    shape, seed = SHAPES[0]
    pcs = run(shape, seed, "os", 0)["pcs"]
    pipe = pipeline(shape, F)
    got = pipe.ego_velocities(VelocityEstimator(Geometry("standard")), point_clouds=pcs)
    ref = VelocityEstimator(Geometry("standard"))
    want = np.array([np.array(ref.process(points=p)) for p in pcs])
    assert got.shape == (F, 3) and rel_err(got, want) <= ego_cases().rel_tol
