"""The rounding bands of the ego and the vehicle velocity kernels on the GPU, on the crafted frames of
``lsq_band_cases`` and against its exact rational reference: every unflagged result lies within the band the design gives it,
every decision placed inside a band raises exactly its flag, the same decision eight bands away raises none and falls as the exact
reference says, a chained launch carries a refit's band into the next frame's static filter, and the flagged frames come back
from the pipeline equal to the host path.  Needs neither scikit-learn (but for the ego pipeline's host fits) nor the reference."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import lsq_band_cases as L
from egovel_cases import Geometry, cases as ego_cases
from vehicle_vel_cases import PARAMS, cases as veh_cases, restate_frame
from test_gpu_egovel import have_sklearn, make_cm, run_kernel as run_ego, seed_tables_without_sklearn
from test_gpu_vehicle_vel import make_pipe, run_kernel as run_veh
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator, VelocityEstimator
from mmwave_radar_processing_amd.point_cloud_processing.vel_estimator import ransac_fit

pytestmark = pytest.mark.gpu

assert (L.VEH_FLAG_RESIDUAL, L.VEH_FLAG_STATIC, L.VEH_FLAG_ERROR_TIE, L.VEH_FLAG_COND, L.VEH_FLAG_CHAIN) == (
    _lib.VEHICLE_FLAG_RESIDUAL, _lib.VEHICLE_FLAG_STATIC, _lib.VEHICLE_FLAG_ERROR_TIE, _lib.VEHICLE_FLAG_COND, _lib.VEHICLE_FLAG_CHAIN)


def veh_restate(f):
    return restate_frame(f.points, getattr(f, "init", None), f.dim, veh_cases().draws_of, **PARAMS)


def veh_check_exact(f, row, status, what):
    """An unflagged vehicle row against the exact result of the winning iteration: returns the two error / band ratios."""
    dim, r = f.dim, veh_restate(f)
    assert status == r["status"] and row[dim + 1] == r["kept"], (what, f.name, row.tolist(), r)
    if not status:
        assert not row[:dim + 1].any()
        return 0.0, 0.0, None
    pts, init = f.points, getattr(f, "init", None)
    if init is not None:                                         # the points the static filter keeps, by the exact residuals
        ex = L.Exact(pts, dim, 1.0)
        e = [(v + sum(h * Fr(float(x)) for h, x in zip(row_h, init))) ** 2 for v, row_h in zip(ex.vals, ex.rows)]
        pts = pts[[x < Fr(L.STATIC_THR) for x in e]]
    assert len(pts) == r["kept"]
    want = L.veh_exact(pts, dim, L.veh_draws(len(pts))[r["iter"]])
    dc, de = L.distance(row[:dim], want.vel), abs(float(Fr(float(row[dim])) - want.err))
    print(f"{what} {f.name}: refit cond {want.cond:.3e} |dc| {dc:.3e} band_c {want.band_c:.3e} ratio {dc / want.band_c:.3e}; "
          f"|derr| {de:.3e} band {want.band_err:.3e} ratio {de / want.band_err:.3e}")
    assert dc <= want.band_c and de <= want.band_err, (what, f.name, dc, want.band_c, de, want.band_err)
    return dc / want.band_c, de / want.band_err, want


# ------------------------------------------------------------------------------------------------------- soundness of the bands
@pytest.mark.parametrize("dim", [2, 3])
def test_ego_condition_sweep_stays_inside_its_bands(dim):
    """Condition bounds 10 ... 1e5, just below and just above the cap: coefficients within band_c and R^2 within band_s of the
    exact solution on the returned inlier set; above the cap COND, below it none."""
    frames = L.condition_sweep("ego", dim)
    out, flags, masks = run_ego(ego_cases(), [f.points for f in frames], dim)
    for i, f in enumerate(frames):
        n = len(f.points)
        if f.flag:
            assert flags[i] == L.EGO_FLAG_COND and not out[i].any() and not masks[i].any(), (f.name, flags[i])
            print(f"ego dim {dim} {f.name}: flagged COND")
            continue
        assert flags[i] == 0, (f.name, flags[i])
        inl = np.ones(n, dtype=bool)
        inl[f.outliers] = False
        np.testing.assert_array_equal(masks[i, :n], inl, err_msg=f.name)
        want = L.ego_exact(f.points, dim, masks[i, :n])
        dc, ds = L.distance(out[i, :dim], want.coef), abs(float(Fr(float(out[i, dim])) - want.r2))
        print(f"ego dim {dim} {f.name}: refit cond {want.cond:.3e} |dc| {dc:.3e} band_c {want.band_c:.3e} ratio {dc / want.band_c:.3e}; "
              f"|dR2| {ds:.3e} band_s {want.band_s:.3e} ratio {ds / want.band_s:.3e}")
        assert dc <= want.band_c and ds <= want.band_s and not want.loose, (f.name, dc, want.band_c, ds, want.band_s)
        assert out[i, dim + 1] == want.share
    assert frames[-1].flag and not frames[-2].flag and frames[-2].cond > 0.9 * L.COND_CAP and len(frames) >= 6


@pytest.mark.parametrize("dim", [2, 3])
def test_vehicle_condition_sweep_stays_inside_its_bands(dim):
    """The same for the vehicle kernel: the velocity within band_c and the error within its band of the exact refit on the
    members restated from the exact first fit."""
    frames = L.condition_sweep("veh", dim)
    out, status, flags = run_veh(veh_cases(), [f.points for f in frames], dim)
    for i, f in enumerate(frames):
        if f.flag:
            assert flags[i] == _lib.VEHICLE_FLAG_COND and not out[i].any() and status[i] == 0, (f.name, flags[i])
            print(f"vehicle dim {dim} {f.name}: flagged COND")
            continue
        assert flags[i] == 0, (f.name, flags[i])
        _, _, want = veh_check_exact(f, out[i], status[i], f"vehicle dim {dim}")
        assert status[i] == 1 and sorted(want.members) == [k for k in range(len(f.points)) if k not in f.outliers]
    assert frames[-1].flag and not frames[-2].flag and frames[-2].cond > 0.9 * L.COND_CAP and len(frames) >= 6


# ------------------------------------------------------------------------------------------------------- every undecided flag
@pytest.mark.parametrize("dim", [2, 3])
def test_ego_residual_score_tie_and_r2_flags(dim):
    """EGO_FLAG_RESIDUAL (1) at 0.15 + {0, +-1/4} band, nothing at +-8 bands with the moved point's mask bit as the exact residual
    says; EGO_FLAG_SCORE_TIE (2) between mirror-image sets, nothing between equal sets; EGO_FLAG_R2 (4) with r2_thr on the exact
    R^2 and on a frame of one speed, nothing with r2_thr eight band_s away."""
    c = ego_cases()
    r2 = L.ego_r2_cases(dim)
    frames = L.ego_residual_cases(dim) + L.ego_tie_cases(dim) + L.ego_same_set_case(dim) + r2[-1:]
    out, flags, masks = run_ego(c, [f.points for f in frames], dim)
    for i, f in enumerate(frames):
        print(f"ego dim {dim} {f.name}: flags {flags[i]} (want {f.flag}) row {out[i].tolist()}")
        assert flags[i] == f.flag, (f.name, flags[i], f.flag)
        if f.flag:
            assert not out[i].any() and not masks[i].any(), f.name
        elif f.moved is not None:
            far = 3 if "residual" in f.name else 0               # the residual frames' far outliers
            assert masks[i, f.moved] == f.inside and masks[i].sum() == len(f.points) - far - (0 if f.inside else 1), (f.name, masks[i].sum())
    assert {f.flag for f in frames} == {0, L.EGO_FLAG_RESIDUAL, L.EGO_FLAG_SCORE_TIE, L.EGO_FLAG_R2}
    for f in r2[:-1]:
        out, flags, masks = run_ego(c, [f.points], dim, r2_thr=f.r2_thr)
        print(f"ego dim {dim} {f.name}: r2_thr {f.r2_thr!r} flags {flags[0]} (want {f.flag}) R2 {out[0, dim]!r}")
        assert flags[0] == f.flag, (f.name, flags[0])
        if f.flag:
            assert not out[0].any() and not masks[0].any()
        else:
            want = L.ego_exact(f.points, dim, f.mask)
            np.testing.assert_array_equal(masks[0, :len(f.points)], f.mask)
            assert abs(float(Fr(float(out[0, dim])) - want.r2)) <= want.band_s and L.distance(out[0, :dim], want.coef) <= want.band_c


def test_ego_tables_flag():
    """EGO_FLAG_TABLES (32): a subset index equal to N, a subset_row outside the rows, a trials_off that runs past tab_len."""
    c = ego_cases()
    f, ok = L.condition_sweep("ego", 2)[1], L.ego_same_set_case(2)[0]
    n = len(f.points)
    k = int(np.nonzero(c.table_n == n)[0][0])

    def index_n(sub, row, tab, offs):
        sub = sub.copy()
        sub[k, 0, 3] = n
        return sub, row, tab, offs

    def row_beyond(sub, row, tab, offs):
        return sub, np.where(np.arange(len(row)) == 0, len(offs), row).astype(np.int32), tab, offs

    def row_negative(sub, row, tab, offs):
        return sub, np.where(np.arange(len(row)) == 0, -1, row).astype(np.int32), tab, offs

    def off_past_the_end(sub, row, tab, offs):
        offs = offs.copy()
        offs[k] = len(tab) - n                                    # n + 1 entries are needed
        return sub, row, tab, offs
    for edit in (index_n, row_beyond, row_negative, off_past_the_end):
        out, flags, masks = run_ego(c, [f.points, ok.points], 2, tables=edit)
        assert flags[0] == L.EGO_FLAG_TABLES and not out[0].any() and not masks[0].any(), (edit.__name__, flags[0])
        assert flags[1] == 0 and out[1, 3] == 10 / 11, (edit.__name__, flags[1], out[1].tolist())   # its neighbour reads other rows


@pytest.mark.parametrize("dim", [2, 3])
def test_vehicle_residual_static_and_error_tie_flags(dim):
    """MMW_VEHICLE_FLAG_RESIDUAL at fit_thresh + {0, +-1/4} band_e (N = 65 with outliers; N = 11, every point needed for a
    consensus), MMW_VEHICLE_FLAG_STATIC the same at static_vel_thresh with the evaluation-only band,
    MMW_VEHICLE_FLAG_ERROR_TIE between mirror-image member sets; eight bands away, and between equal sets, nothing, and the row is
    the exact reference's: status, kept points, the error with or without the moved point."""
    c = veh_cases()
    frames = L.veh_residual_cases(dim, 65, 2) + L.veh_residual_cases(dim, 11, 0) + L.veh_tie_cases(dim) + L.veh_same_set_case(dim)
    static = L.veh_static_cases(dim)
    out, status, flags = run_veh(c, [f.points for f in frames], dim)
    out_s, status_s, flags_s = run_veh(c, [f.points for f in static], dim, init=np.array([f.init for f in static]))
    frames, out, status, flags = frames + static, np.r_[out, out_s], np.r_[status, status_s], np.r_[flags, flags_s]
    for i, f in enumerate(frames):
        print(f"vehicle dim {dim} {f.name}: flags {flags[i]} (want {f.flag}) status {status[i]} row {out[i].tolist()}")
        assert flags[i] == f.flag, (f.name, flags[i], f.flag)
        if f.flag:
            assert not out[i].any() and status[i] == 0, f.name
            continue
        _, _, want = veh_check_exact(f, out[i], status[i], f"vehicle dim {dim}")
        if "static" in f.name:
            assert out[i, dim + 1] == f.kept and status[i] == 1, (f.name, out[i].tolist())
        elif f.moved is not None:
            drew_it = f.moved in L.veh_draws(len(f.points))[veh_restate(f)["iter"]]   # N = 11: most iterations draw the moved point
            assert status[i] == 1 and (drew_it or (f.moved in want.members) == f.inside), (f.name, status[i])
    assert {f.flag for f in frames} == {0, _lib.VEHICLE_FLAG_RESIDUAL, _lib.VEHICLE_FLAG_STATIC, _lib.VEHICLE_FLAG_ERROR_TIE}


# ------------------------------------------------------------------------------------------------------- the chain's carried band
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("side", [-1, 1])
def test_chain_carries_the_refit_band_into_the_next_static_filter(dim, side):
    """Frame 0's refit has a condition bound of 1e5; frame 1 holds a point a quarter of the widened band from static_vel_thresh,
    hundreds of thousands of plain bands away.  Chained: MMW_VEHICLE_FLAG_STATIC there and MMW_VEHICLE_FLAG_CHAIN behind it.
    Unchained with frame 0's exact refit as the caller's row, which carries no band: decided, as the exact reference says."""
    c = veh_cases()
    ch = L.veh_chain_cases(dim, side)
    out, status, flags = run_veh(c, ch.frames, dim, chain=True)
    print(f"chain dim {dim} side {side}: flags {flags.tolist()} distance {ch.dist_wide:.3f} widened bands, {ch.dist_plain:.3e} plain bands")
    assert flags.tolist() == [0, _lib.VEHICLE_FLAG_STATIC, _lib.VEHICLE_FLAG_CHAIN], flags.tolist()
    assert status.tolist() == [1, 0, 0] and not out[1:].any()
    assert L.distance(out[0, :dim], ch.est) <= ch.band_c         # what the chain carries lies within the band it carries
    init = np.full((3, dim), np.nan)
    init[1] = ch.seed
    out2, status2, flags2 = run_veh(c, ch.frames, dim, init=init)
    assert not flags2.any() and status2.tolist() == [1, 1, 1], (flags2.tolist(), status2.tolist())
    assert out2[1, dim + 1] == ch.kept, (out2[1].tolist(), ch.kept)
    # a caller's seed row carries no band in a chain either
    out3, status3, flags3 = run_veh(c, ch.frames[1:], dim, init=ch.seed[None, :], chain=True)
    assert not flags3.any() and out3[0, dim + 1] == ch.kept and status3.tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------------- hand-back
@pytest.mark.parametrize("dim", [2, 3])
def test_flagged_crafted_ego_frames_come_back_equal_to_the_host_path(dim):
    c = ego_cases()
    seed_tables_without_sklearn(c)
    res, sweep = L.ego_residual_cases(dim), L.condition_sweep("ego", dim)
    frames = [res[1], res[3], L.ego_tie_cases(dim)[0], L.ego_same_set_case(dim)[0], L.ego_r2_cases(dim)[-1], sweep[-1], sweep[2], res[4],
              res[0]]                                            # the last workgroup's frame is a flagged one
    pts = [f.points for f in frames]
    pipe = FramePipeline(make_cm(synth.synth_cfg_text(num_samples=16, num_loops=8)), len(pts), (4, 16, 8), det_capacity=c.cap)
    est = VelocityEstimator(Geometry("standard" if dim == 2 else "ods"))
    if not have_sklearn():
        with pytest.raises(ImportError):        # a flagged frame needs scikit-learn, and says so
            pipe.ego_fits(est, pts)
        return
    fits, counts = pipe.ego_fits(est, pts, with_mask=True)
    raw, raw_flags, raw_masks = run_ego(c, pts, dim)
    assert pipe.ego_flags.tolist() == [f.flag for f in frames] == raw_flags.tolist() and pipe.n_ego_flagged == 5
    for k, f in enumerate(frames):
        if f.flag:
            coef, r2, share, mask = ransac_fit(f.points, dim, return_mask=True)
            want = np.zeros(dim + 2)
            want[:len(coef)], want[dim:] = coef, (r2, share)
            assert np.array_equal(fits[k], want) and np.array_equal(pipe.ego_masks[k, :counts[k]], mask), (f.name, fits[k], want)
        else:
            assert np.array_equal(fits[k], raw[k]) and np.array_equal(pipe.ego_masks[k], raw_masks[k]), f.name


@pytest.mark.parametrize("dim", [2, 3])
def test_flagged_crafted_vehicle_frames_come_back_equal_to_the_host_path(dim):
    c = veh_cases()
    res, sweep, static = L.veh_residual_cases(dim, 65, 2), L.condition_sweep("veh", dim), L.veh_static_cases(dim)

    def host_row(points, prior):
        host = VehicleVelEstimator(seed=c.seed)
        with np.errstate(all="ignore"):
            found, kept = host.ransac(points, np.empty(0) if prior is None else prior, dim == 2)
        return (np.r_[host.get_vehicle_vel_est(), host.best_error, kept] if found else np.r_[np.zeros(dim + 1), kept]), int(found)

    def check(frames, initial, raw, raw_flags):
        pts = [f.points for f in frames]
        pipe = make_pipe(len(pts), c.cap)
        with np.errstate(all="ignore"):
            fits, status = pipe.vehicle_fits(VehicleVelEstimator(seed=c.seed), pts, initial, only_2D=dim == 2)
        assert pipe.vehicle_flags.tolist() == [f.flag for f in frames] == raw_flags.tolist()
        for k, f in enumerate(frames):
            if f.flag:
                want, found = host_row(f.points, None if initial is None else initial[k])
                assert status[k] == found and np.array_equal(fits[k], want), (f.name, fits[k], want)
            else:
                assert np.array_equal(fits[k], raw[k]), f.name
    frames = [res[1], res[3], L.veh_tie_cases(dim)[0], L.veh_same_set_case(dim)[0], sweep[-1], sweep[2], res[4], res[0]]
    raw, _, raw_flags = run_veh(c, [f.points for f in frames], dim)
    check(frames, None, raw, raw_flags)
    frames = [static[3], static[1], static[4], static[0]]
    initial = np.array([f.init for f in frames])
    raw, _, raw_flags = run_veh(c, [f.points for f in frames], dim, init=initial)
    check(frames, initial, raw, raw_flags)
    # a drive: the host decides the frame the carried band leaves open, with the estimate the kernel carried, and the drive goes on
    ch = L.veh_chain_cases(dim, 1)
    pipe = make_pipe(3, c.cap)
    fits, status = pipe.vehicle_fits(VehicleVelEstimator(seed=c.seed), ch.frames, track=True, only_2D=dim == 2)
    assert pipe.vehicle_flags.tolist() == [0, _lib.VEHICLE_FLAG_STATIC, 0] and pipe.n_vehicle_flagged == 1 and status.tolist() == [1, 1, 1]
    want, found = host_row(ch.frames[1], fits[0, :dim])
    assert found == 1 and np.array_equal(fits[1], want), (fits[1], want)
