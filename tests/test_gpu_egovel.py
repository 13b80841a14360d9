"""Device point clouds and the batched ego-velocity RANSAC on the GPU: ``point_clouds_device()`` against ``point_clouds()`` bit for
bit under the three detectors, ``mmw_ego_velocity_ransac`` through the raw ABI against the reference's recorded fits (driven by
the recorded subset / trial tables: no scikit-learn needed), and ``FramePipeline.ego_velocities`` against the recorded tracks."""
import ctypes

import numpy as np
import pytest

from egovel_cases import DEGENERATE, Geometry, cases, rel_err
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.detectors import CaCFAR2D
from mmwave_radar_processing_amd.point_cloud_processing import VelocityEstimator, ransac_tables as T
from mmwave_radar_processing_amd.processors.range_doppler_detection import (RangeDopplerDetectorSequential,
                                                                           RangeDopplerGroundDetector)

pytestmark = pytest.mark.gpu

AZ, EL = [0, 3, 4, 7], [9, 8, 5, 4]
SHAPE = (12, 256, 128)
SEQ = dict(rng_cfar_type="os_cfar_1d", rng_cfar_params={"num_train": 5, "num_guard": 3, "rho": 0.6, "alpha": 2},
           vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 5, "num_guard": 2, "rho": 0.7, "alpha": 3})
GROUND = dict(vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 12, "num_guard": 4, "rho": 0.5, "alpha": 6},
              altimeter_params={"min_altitude_m": 0.6, "zoom_search_region_m": 0.2, "altitude_search_limit_m": 0.6,
                                "range_bias": 0.0, "precise_est_enabled": False})
FLAG_COND, FLAG_NONFINITE = 8, 16


def make_cm(text=synth.SYNTH_CFG_256x128x12):
    cm = ConfigManager()
    cm.load_cfg_text(text)
    return cm


def have_sklearn():
    try:
        import sklearn  # noqa: F401
        return True
    except ImportError:
        return False


def seed_tables_without_sklearn(c):
    if not have_sklearn():
        for n, sub, trials in zip(c.table_n.tolist(), c.table_subsets, c.table_trials):
            T.seed_tables(n, sub, trials)


def detector_kwargs(which, cm):
    if which == "cfar":
        return dict(cfar=CaCFAR2D((4, 4), (2, 2), 1e-5))
    if which == "ground":
        return dict(ground=RangeDopplerGroundDetector(cm, **GROUND))
    return dict(sequential=RangeDopplerDetectorSequential(cm, **SEQ))


@pytest.mark.parametrize("which", ["cfar", "ground", "sequential"])
@pytest.mark.parametrize("az,el", [(AZ, EL), ([], EL), (AZ, []), ([], [])])
def test_point_clouds_device_equals_point_clouds_bit_for_bit(which, az, el, golden):
    g = golden("frames_256.npz")
    cm = make_cm()
    cubes = np.stack([synth.synth_cube(int(s)) for s in g["seeds"]] + [synth.synth_cube(77, num_targets=0)])
    if which == "ground":
        cubes = synth.synth_ground_sequence(606, 5)     # the frames of the ground detector's reference fixtures
    pipes = [FramePipeline(cm, len(cubes), SHAPE, az_antenna_idxs=az, el_antenna_idxs=el, **detector_kwargs(which, cm))
             for _ in range(2)]                 # two pipelines: the ground detector's altimeter advances with every call
    for p in pipes:
        p.load(cubes)
    want = pipes[0].point_clouds()
    buf = pipes[1].point_clouds_device()
    got = pipes[1].fetch_point_clouds()
    assert buf.nbytes >= len(cubes) * pipes[1].cap * 32 and len(got) == len(want)
    assert sum(len(w) for w in want) > 0
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.float64, (f, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"frame {f} differs"
    np.testing.assert_array_equal(pipes[1].counts, [len(w) for w in want])
    full = buf.download((len(cubes), pipes[1].cap, 4), np.float64)
    for f, w in enumerate(want):
        assert not full[f, len(w):].any()       # the slots behind a frame's points are zero


def test_point_clouds_device_on_the_non_power_of_two_golden_frame(golden):
    """The (12, 63, 70) frame of small_chain.npz (the shipped 6843 ODS cfg): the float64 detection path and the separate exact
    argmax feed the device point clouds here; detections as recorded from the reference."""
    import json
    import os
    from conftest import GOLDEN
    from mmwave_radar_processing_amd.processors import VirtualArrayReformatter
    g = golden("small_chain.npz")
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        cm = make_cm("\n".join(json.load(fh)["6843_RadVel_ods_20Hz.cfg"]["lines"]))
    cube = VirtualArrayReformatter(cm).process(synth.synth_raw_cube(202, 4, 3, 63, 70))
    cubes = np.stack([cube, cube[::-1]]).astype(np.complex64)
    pipes = [FramePipeline(cm, 2, (12, 63, 70), az_antenna_idxs=AZ, el_antenna_idxs=EL, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5))
             for _ in range(2)]
    for p in pipes:
        p.load(cubes)
    want = pipes[0].point_clouds()
    np.testing.assert_array_equal(pipes[0].dets[0], g["np2_dets"])
    pipes[1].point_clouds_device()
    got = pipes[1].fetch_point_clouds()
    assert len(want[0]) == len(g["np2_dets"]) > 0
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def run_kernel(c, points, dim, r2_thr=0.6, cap=None, tables=None):
    """The frames ``points`` through mmw_ego_velocity_ransac with the recorded tables, or with ``tables(subsets, row, tab, offs)``'s
    edition of them: (out [F, dim + 2], flags, masks)."""
    ctx = _lib.default_context()
    cap = cap or c.cap
    F = len(points)
    counts = np.array([len(p) for p in points], dtype=np.int32)
    packed = np.zeros((F, cap, 4))
    for f, p in enumerate(points):
        packed[f, :len(p)] = p
    subsets, row, tab, offs = c.tables_for(counts) if tables is None else tables(*c.tables_for(counts))
    bufs = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        b = ctx.alloc(max(arr.nbytes, 16))
        b.upload(arr)
        bufs.append(b)
        return b
    d_pts, d_cnt, d_sub, d_row, d_tab, d_off = (dev(x) for x in (packed, counts, subsets, row, tab, offs))
    d_out, d_flags, d_mask = ctx.alloc(F * (dim + 2) * 8), ctx.alloc(F * 4), ctx.alloc(F * cap)
    bufs += [d_out, d_flags, d_mask]
    _lib.check(ctx.lib.mmw_ego_velocity_ransac(ctx.handle, d_pts.ptr, d_cnt.ptr, F, cap, dim, c.thr, r2_thr, d_sub.ptr, d_row.ptr,
                                               len(offs), d_tab.ptr, len(tab), d_off.ptr, d_out.ptr, d_flags.ptr, d_mask.ptr))
    out = d_out.download((F, dim + 2), np.float64).copy()
    flags = d_flags.download((F,), np.int32).copy()
    masks = d_mask.download((F, cap), np.uint8).copy().astype(bool)
    for b in bufs:
        b.free()
    return out, flags, masks


@pytest.mark.parametrize("dim", [2, 3])
def test_kernel_cases_against_the_reference(dim):
    """N = 0, 9, 10, 11, 64, 65, 256, 257, cap; clean / half outliers / no inlier / one inlier / <= 3 inliers / one bearing /
    a point at range 0.  Unflagged: identical inlier masks, coefficients, R^2 and share within the fixture's tolerance (ten
    times the distance of a NumPy normal-equation refit from the reference).  Flagged: the degenerate two only."""
    c = cases()
    want = c.fits[dim]
    assert sorted(c.counts[:9].tolist()) == [0, 9, 10, 11, 64, 65, 256, 257, c.cap]
    out, flags, masks = run_kernel(c, c.points, dim)
    worst = 0.0
    for i, name in enumerate(c.names):
        n = int(c.counts[i])
        print(f"dim {dim} {name}: N {n} flags {flags[i]} out {out[i].tolist()}")
        if name in DEGENERATE:
            assert flags[i] & (FLAG_COND if name == "one_bearing" else FLAG_NONFINITE), (name, flags[i])
            assert not out[i].any() and not masks[i].any()
            continue
        assert flags[i] == 0, (name, flags[i])
        np.testing.assert_array_equal(masks[i, :n], want["mask"][i], err_msg=name)
        assert not masks[i, n:].any()
        ref = np.r_[want["coef"][i][:dim], want["r2"][i], want["share"][i]]
        err = rel_err(out[i], ref)
        worst = max(worst, err)
        assert err <= c.rel_tol, (name, err, c.rel_tol, out[i].tolist(), ref.tolist())
        assert out[i, dim + 1] == want["share"][i]                  # an integer ratio: exact
    print(f"dim {dim}: worst relative distance {worst:.3e}, tolerance {c.rel_tol:.3e}")
    # what the content cases are there for
    by = dict(zip(c.names, range(len(c.names))))
    assert not out[by["clean_9"]].any() and not out[by["no_inlier"]].any() and not out[by["clean_0"]].any()
    assert want["mask"][by["one_inlier"]].sum() == 1 and out[by["one_inlier"], dim] == 0.0
    assert 2 <= want["mask"][by["few_inliers"]].sum() <= 3 and out[by["few_inliers"], dim] == 0.0
    assert 0.2 <= want["share"][by["half_outliers"]] <= 0.6


@pytest.mark.parametrize("dim", [2, 3])
def test_flagged_frames_equal_the_reference_after_the_fallback(dim):
    c = cases()
    seed_tables_without_sklearn(c)
    idx = [c.names.index(n) for n in DEGENERATE + ("clean_64", "half_outliers")]
    pts = [c.points[i] for i in idx]
    cm = make_cm(synth.synth_cfg_text(num_samples=16, num_loops=8))
    pipe = FramePipeline(cm, len(pts), (4, 16, 8), det_capacity=c.cap)
    est = VelocityEstimator(Geometry("standard" if dim == 2 else "ods"))
    if not have_sklearn():
        with pytest.raises(ImportError):        # a flagged frame needs scikit-learn, and says so
            pipe.ego_fits(est, pts)
        return
    fits, counts = pipe.ego_fits(est, pts, with_mask=True)
    assert pipe.n_ego_flagged == 2 and pipe.ego_flags[:2].all() and not pipe.ego_flags[2:].any()
    for k, i in enumerate(idx):
        want = c.fits[dim]
        ref = np.r_[want["coef"][i][:dim], want["r2"][i], want["share"][i]]
        assert rel_err(fits[k], ref) <= c.rel_tol, (c.names[i], fits[k], ref)
        np.testing.assert_array_equal(pipe.ego_masks[k, :counts[k]], want["mask"][i])


@pytest.mark.parametrize("geometry", ["standard", "ods"])
def test_pipeline_track_in_one_call_and_in_two(geometry):
    c = cases()
    seed_tables_without_sklearn(c)
    cm = make_cm(synth.synth_cfg_text(num_samples=16, num_loops=8))
    pipe = FramePipeline(cm, len(c.seq), (4, 16, 8), det_capacity=c.cap)
    one = pipe.ego_velocities(VelocityEstimator(Geometry(geometry)), c.seq)
    assert pipe.n_ego_flagged == 0 and one.shape == (len(c.seq), 3) and one.dtype == np.float64
    err = rel_err(one, c.track[geometry])
    print(f"{geometry}: track distance {err:.3e}, tolerance {c.rel_tol:.3e}")
    assert err <= c.rel_tol
    held = np.all(c.track[geometry][1:] == c.track[geometry][:-1], axis=1)
    np.testing.assert_array_equal(np.all(one[1:] == one[:-1], axis=1), held)       # the same frames adopt a new estimate
    est = VelocityEstimator(Geometry(geometry))
    two = np.concatenate([pipe.ego_velocities(est, c.seq[:20]), pipe.ego_velocities(est, c.seq[20:])])
    np.testing.assert_array_equal(one, two)


def test_ego_velocities_from_detected_frames_equals_the_frame_loop():
    """The whole path on detected (bin-grid) point clouds: detector -> device point clouds -> kernel (+ fallback) -> state scan,
    against the mirrored estimator fed the host point clouds frame by frame."""
    if not have_sklearn():
        pytest.skip("the frame loop of the mirrored estimator needs scikit-learn")
    cm = make_cm()
    cubes = np.stack([synth.synth_cube(s) for s in range(6)])
    pipes = [FramePipeline(cm, len(cubes), SHAPE, az_antenna_idxs=AZ, el_antenna_idxs=EL, cfar=CaCFAR2D((4, 4), (2, 2), 1e-5))
             for _ in range(2)]
    for p in pipes:
        p.load(cubes)
    ref_est, est = VelocityEstimator(cm, 0.0, 0.0), VelocityEstimator(cm, 0.0, 0.0)
    want = np.array([np.array(ref_est.process(points=pc)) for pc in pipes[0].point_clouds()])
    got = pipes[1].ego_velocities(est)
    print("flagged", pipes[1].n_ego_flagged, "of", len(cubes), "flags", pipes[1].ego_flags.tolist())
    assert rel_err(got, want) <= cases().rel_tol


def test_bad_arguments_are_refused():
    ctx = _lib.default_context()
    L, h = ctx.lib, ctx.handle
    d = ctx.alloc(1024)
    args = lambda cap, dim: (h, d.ptr, d.ptr, 1, cap, dim, 0.15, 0.6, d.ptr, d.ptr, 1, d.ptr, 16, d.ptr, d.ptr, d.ptr, None)  # noqa: E731
    assert L.mmw_ego_velocity_ransac(*args(16, 4)) == _lib.MMW_ERR_INVALID
    assert L.mmw_ego_velocity_ransac(*args(1 << 20, 2)) == _lib.MMW_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="geometry"):
        FramePipeline(make_cm(synth.synth_cfg_text(num_samples=16, num_loops=8)), 2, (4, 16, 8)).ego_fits(
            VelocityEstimator(Geometry("other")), [np.empty((0, 4))])
    d.free()
