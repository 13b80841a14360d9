"""Antenna-integrated CFAR detection on the GPU: FramePipeline(integrate_rx=...) against the NumPy restatement of
tests/integrated_cases.py (test_integrated_cases_host.py asserts the margin that lets the detections be demanded identical).

The power plane is held to the bound derived from the project's own figure for one antenna's float64 |RD| plane
(axis_fft_cases.mag64_ulps against the plane's L1 norm; integrated_cases.power_bound):
    delta_v = mag64_ulps(S, C) 2^-53 l1_v,    |dP| <= sum_v (2 |RD_v| + delta_v) delta_v + (n_ants + 2) 2^-53 P.
Two device results (another order of the list, another route) are each within that bound of the truth, so they are held to the
sum of their two bounds.

| test                      | what would make it fail                                                                             |
|---------------------------|-----------------------------------------------------------------------------------------------------|
| power plane               | a wrong antenna, a missed or doubled term, |RD| in place of |RD|^2, a stale first-antenna store       |
| detections, point clouds  | CFAR reading another plane than the one written, the argmax disturbed by the new route               |
| determinism and order     | a sum whose order depends on scheduling; a list order that changes more than rounding                |
| routes agree              | the persistent kernel and the per-antenna route computing different planes                           |
| default untouched         | the keyword's default changing what a pipeline without it does                                       |
| velocity estimators       | the device point clouds of the integrated route not being what ego / vehicle_velocities read        |
| multi-device              | the sharded form giving other results than one pipeline (two contexts on device 0)                  |
"""
import functools

import numpy as np
import pytest

import integrated_cases as ic
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

IDS = [c.name for c in ic.CASES]


def make_pipe(c, ants="case", **kw):
    cm, _ = ic.config(c.shape)
    ants = list(c.ants) if ants == "case" else ants
    pipe = FramePipeline(cm, len(c.seeds), c.shape, cfar=ic.make_cfar(c.cfar), az_antenna_idxs=ic.AZ[:min(8, c.shape[0])],
                         el_antenna_idxs=ic.EL if c.shape[0] == 12 else [], integrate_rx=ants, **kw)
    pipe.load(ic.cubes(c.shape, c.seeds))
    return pipe


@functools.lru_cache(maxsize=None)
def bounds(name):
    c = ic.BY_NAME[name]
    cubes, rd = ic.cubes(c.shape, c.seeds), ic.rd_planes(c.shape, c.seeds)
    b = np.stack([ic.power_bound(cubes[f], rd[f], c.ants) for f in range(len(c.seeds))])
    b.setflags(write=False)
    return b


@pytest.mark.parametrize("name", IDS)
def test_power_detections_and_point_clouds_match_the_restatement(name):
    c, ref = ic.BY_NAME[name], ic.reference(name)
    _, sc = ic.config(c.shape)
    rd = ic.rd_planes(c.shape, c.seeds)
    pipe = make_pipe(c)
    # ---- the power plane, within the derived bound
    got = pipe.integrated_power()
    assert got.shape == ref.power.shape and got.dtype == np.float64
    ratio = np.abs(got - ref.power) / bounds(name)
    print(f"{name}: worst |dP| / bound {ratio.max():.3e} (worst relative error {np.max(np.abs(got - ref.power) / ref.power):.3e})")
    assert ratio.max() <= 1.0
    assert np.array_equal(pipe.integrated_power(1, 2), got[1:2])
    # ---- detections: identical, order included
    dets = pipe.detect()
    assert len(dets) == len(c.seeds)
    for f, d in enumerate(dets):
        np.testing.assert_array_equal(d, ref.dets[f], err_msg=f"frame {f}")
    # ---- point clouds and argmax indices
    pcs = pipe.point_clouds()
    az = ic.AZ[:min(8, c.shape[0])]
    for f, pc in enumerate(pcs):
        np.testing.assert_array_equal(pipe.dets[f], ref.dets[f], err_msg=f"frame {f}")
        if c.shape[0] == 12:
            want, az_i, el_i = ic.point_cloud(rd[f], ref.dets[f], sc)
            np.testing.assert_array_equal(pipe.el_idx[f], el_i, err_msg=f"frame {f}")
        else:
            want, az_i = _point_cloud_az_only(rd[f], ref.dets[f], sc, az)
        np.testing.assert_array_equal(pipe.az_idx[f], az_i, err_msg=f"frame {f}")
        assert pc.shape == want.shape
        assert np.max(np.abs(pc - want), initial=0.0) <= 1e-9 * sc["range_max_m"]
    # ---- the device point clouds are the host's, bit for bit
    pipe.point_clouds_device()
    for f, pc in enumerate(pipe.fetch_point_clouds()):
        assert np.array_equal(pc, pcs[f]), f


def _point_cloud_az_only(rd, dets, sc, az, A=64):
    if dets.shape[0] == 0:
        return np.empty((0, 4)), np.empty(0, dtype=np.int64)
    rbins, vbins = O.rd_bins(sc)
    _, abins = O.angle_tables(A)
    az_i, _ = O.angle_argmax(rd, dets[:, 0], dets[:, 1], az, A, True)
    a, rng = abins[az_i], rbins[dets[:, 0]]
    return np.column_stack((rng * np.cos(a), rng * np.sin(a), np.zeros(len(a)), vbins[dets[:, 1]])), az_i


@pytest.mark.parametrize("name", ["256x128_f9-perm-ca", "256x128_f3-perm-ca", "63x70-perm-ca", "64x64-perm-ca", "512x64-perm-ca"])
def test_same_list_same_bits_and_other_order_within_the_bound(name):
    c = ic.BY_NAME[name]
    pipe = make_pipe(c)
    a = pipe.integrated_power().copy()
    b = pipe.integrated_power().copy()
    assert np.array_equal(a, b)
    d1 = pipe.detect()
    d2 = pipe.detect()
    assert all(np.array_equal(x, y) for x, y in zip(d1, d2))
    other = make_pipe(c, ants=sorted(c.ants), ctx=pipe.ctx)
    assert sorted(c.ants) != list(c.ants)
    o = other.integrated_power()
    ratio = np.abs(o - a) / (2.0 * bounds(name))
    print(f"{name}: sorted list against the permuted one, worst |dP| / (2 bound) {ratio.max():.3e}, "
          f"bits differ in {int(np.count_nonzero(o != a))} cells")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("lname", ["all", "one", "perm"])
def test_persistent_kernel_and_per_antenna_route_agree(lname):
    big, small = ic.BY_NAME[f"256x128_f9-{lname}-ca"], ic.BY_NAME[f"256x128_f3-{lname}-ca"]
    assert big.seeds[:3] == small.seeds and big.ants == small.ants
    p9, p3 = make_pipe(big), None
    p3 = make_pipe(small, ctx=p9.ctx)
    a, b = p9.integrated_power(0, 3), p3.integrated_power()
    ratio = np.abs(a - b) / (2.0 * bounds(small.name))
    print(f"{lname}: persistent against per-antenna, worst |dP| / (2 bound) {ratio.max():.3e}")
    assert ratio.max() <= 1.0
    d9, d3 = p9.detect(), p3.detect()
    for f in range(3):
        np.testing.assert_array_equal(d9[f], d3[f])
    # the switch that turns the persistent kernel off: the per-antenna route on the large batch (its one-antenna pass is then the
    # batch kernel of mmw_range_doppler_mag64, so the planes are a third computation of the same thing)
    p9.ctx.set_option("MMW_POW64_FUSED", 0)
    try:
        c = p9.integrated_power(0, 3)
    finally:
        p9.ctx.set_option("MMW_POW64_FUSED", None)
    assert np.max(np.abs(c - b) / (2.0 * bounds(small.name))) <= 1.0


def test_default_pipeline_is_untouched():
    c = ic.BY_NAME["256x128_f3-all-ca"]
    cm, _ = ic.config(c.shape)
    pipe = FramePipeline(cm, len(c.seeds), c.shape, cfar=ic.make_cfar(c.cfar), az_antenna_idxs=ic.AZ, el_antenna_idxs=ic.EL)
    assert pipe.integrate_rx is None and pipe._fused_supported(True)
    cubes = ic.cubes(c.shape, c.seeds)
    pipe.load(cubes)
    dets = pipe.detect()
    for f, d in enumerate(dets):
        np.testing.assert_array_equal(d, O.rd_detect_2d(cubes[f])[2])
    with pytest.raises(ValueError, match="integrate_rx"):
        pipe.integrated_power()


def test_weak_target_on_the_device():
    cube = ic.weak_cube()
    cm, _ = ic.config(ic.WEAK_SHAPE)
    cell = np.array(ic.WEAK_CELL)
    has = lambda d: bool(len(d)) and bool(np.any(np.all(d == cell, axis=1)))
    ctx = _lib.default_context()
    found = {}
    for key, ants in (("all", list(range(12))), ("one", [0]), ("default", None)):
        pipe = FramePipeline(cm, 1, ic.WEAK_SHAPE, cfar=ic.make_cfar(ic.CA), integrate_rx=ants, ctx=ctx)
        pipe.load(cube[None])
        found[key] = has(pipe.detect()[0])
    assert found == {"all": True, "one": False, "default": False}


def test_velocity_estimators_take_the_integrated_point_clouds():
    """ego_velocities / vehicle_velocities on the pipeline's own (device) point clouds against the same estimators handed the
    host lists of point_clouds(), which the restatement test has checked."""
    from egovel_cases import Geometry
    from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator, VelocityEstimator
    c = ic.BY_NAME["64x64-all-ca"]
    pipe = make_pipe(c)
    pcs = pipe.point_clouds()
    ego_dev = pipe.ego_velocities(VelocityEstimator(Geometry("standard")))
    ego_host = pipe.ego_velocities(VelocityEstimator(Geometry("standard")), point_clouds=pcs)
    assert ego_dev.shape == (len(c.seeds), 3) and np.array_equal(ego_dev, ego_host, equal_nan=True)
    veh_dev = pipe.vehicle_velocities(VehicleVelEstimator(seed=7))
    veh_host = pipe.vehicle_velocities(VehicleVelEstimator(seed=7), point_clouds=pcs)
    assert len(veh_dev) == len(c.seeds) and np.array_equal(np.asarray(veh_dev), np.asarray(veh_host), equal_nan=True)


def test_multi_device_equals_one_pipeline():
    """Two contexts on device 0 (one device can be opened twice), frames split between them."""
    c = ic.BY_NAME["256x128_f3-perm-ca"]
    cm, _ = ic.config(c.shape)
    single = make_pipe(c)
    mp = MultiDeviceFramePipeline(cm, len(c.seeds), c.shape, devices=[0, 0], cfar=ic.make_cfar(c.cfar), az_antenna_idxs=ic.AZ,
                                  el_antenna_idxs=ic.EL, integrate_rx=list(c.ants))
    try:
        mp.load(ic.cubes(c.shape, c.seeds))
        assert np.array_equal(mp.integrated_power(), single.integrated_power())
        pcs_m, pcs_s = mp.point_clouds(), single.point_clouds()
        for f in range(len(c.seeds)):
            np.testing.assert_array_equal(mp.dets[f], single.dets[f])
            assert np.array_equal(pcs_m[f], pcs_s[f])
    finally:
        mp.close()
