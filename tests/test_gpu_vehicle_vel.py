"""The vehicle velocity estimator's batched RANSAC on the GPU: ``mmw_vehicle_velocity_ransac`` through the raw ABI against the
reference's recorded results (driven by the recorded draws: nothing but NumPy needed), and ``FramePipeline.vehicle_fits`` /
``vehicle_velocities`` with their host fallback.  Condition on the flags: no ordinary frame may be flagged, every degenerate one
must be."""
import numpy as np
import pytest

from vehicle_vel_cases import DEGENERATE, PARAMS, cases, rel_err
from mmwave_radar_processing_amd import _lib, synth
from mmwave_radar_processing_amd.batch import FramePipeline
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator

pytestmark = pytest.mark.gpu

GRID_MAX = 2048          # csrc/mmw_vehicle_vel.h VV_GRID_MAX: workgroups of one batch launch


def run_kernel(c, points, dim, init=None, chain=False, table=None, cap=None):
    """The frames ``points`` through the raw entry with the recorded draws: (rows [F, dim + 2], status, flags)."""
    ctx = _lib.default_context()
    cap = cap or c.cap
    F = len(points)
    counts = np.array([len(p) for p in points], dtype=np.int32)
    packed = np.zeros((F, cap, 4))
    for f, p in enumerate(points):
        packed[f, :len(p)] = p
    table = c.device_table(cap) if table is None else table
    bufs = []

    def dev(arr):
        arr = np.ascontiguousarray(arr)
        b = ctx.alloc(max(arr.nbytes, 16))
        b.upload(arr)
        bufs.append(b)
        return b
    d_pts, d_cnt, d_tab = dev(packed), dev(counts), dev(table)
    d_init = dev(np.asarray(init, dtype=np.float64)) if init is not None else None
    d_out, d_status, d_flags = ctx.alloc(F * (dim + 2) * 8), ctx.alloc(F * 4), ctx.alloc(F * 4)
    bufs += [d_out, d_status, d_flags]
    _lib.check(ctx.lib.mmw_vehicle_velocity_ransac(
        ctx.handle, d_pts.ptr, d_cnt.ptr, F, cap, dim, PARAMS["points_per_fit"], PARAMS["max_iters"], PARAMS["fit_thresh"],
        PARAMS["num_close_pts"], PARAMS["static_vel_thresh"], d_init.ptr if d_init else None, d_tab.ptr, len(table), int(chain),
        d_out.ptr, d_status.ptr, d_flags.ptr))
    out = d_out.download((F, dim + 2), np.float64).copy()
    status = d_status.download((F,), np.int32).copy()
    flags = d_flags.download((F,), np.int32).copy()
    for b in bufs:
        b.free()
    return out, status, flags


def check_rows(c, names, out, status, flags, want_rows, want_status, dim, what):
    worst = 0.0
    for i, name in enumerate(names):
        print(f"{what} {name}: flags {flags[i]} status {status[i]} row {out[i].tolist()}")
        assert flags[i] == 0, (what, name, flags[i])
        assert status[i] == want_status[i] and out[i, dim + 1] == want_rows[i, dim + 1], (what, name, out[i].tolist(), want_rows[i].tolist())
        err = rel_err(out[i, :dim + 1], want_rows[i, :dim + 1])
        worst = max(worst, err)
        assert err <= c.rel_tol, (what, name, err, c.rel_tol, out[i].tolist(), want_rows[i].tolist())
    print(f"{what}: worst relative distance {worst:.3e}, tolerance {c.rel_tol:.3e}")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tag", ["free", "init"])
def test_kernel_cases_against_the_reference(dim, tag):
    """N = 0, 9, 10, 11, 12, 63, 64, 65, 257, cap; half movers; no consensus; one bearing; a point at range 0 -- without and with
    an initial estimate."""
    c = cases()
    assert sorted(c.counts[:10].tolist()) == [0, 9, 10, 11, 12, 63, 64, 65, 257, c.cap]
    init = np.tile(c.init[dim], (len(c.names), 1)) if tag == "init" else None
    out, status, flags = run_kernel(c, c.points, dim, init)
    good = [i for i, n in enumerate(c.names) if n not in DEGENERATE]
    check_rows(c, [c.names[i] for i in good], out[good], status[good], flags[good], c.rows[dim, tag][good], c.status[dim, tag][good],
               dim, f"dim {dim} {tag}")
    for name, bit in zip(DEGENERATE, (_lib.VEHICLE_FLAG_COND, _lib.VEHICLE_FLAG_NONFINITE)):
        i = c.names.index(name)
        assert flags[i] & bit, (name, flags[i])
        assert not out[i].any() and status[i] == 0
    by = dict(zip(c.names, range(len(c.names))))
    assert status[by["clean_11"]] == 1 and status[by["clean_10"]] == 0 and status[by["no_consensus"]] == 0
    assert not out[by["clean_9"], :dim + 1].any() and out[by["clean_9"], dim + 1] == 9
    assert out[by["short_movers"], dim + 1] == 9                 # below num_close_pts the filter is not asked


def test_rows_without_an_estimate_in_the_initial_table():
    c = cases()
    idx = [c.names.index(n) for n in ("clean_64", "half_movers", "clean_257", "clean_65", "clean_12", "half_movers")]
    init = np.tile(c.init[2], (len(idx), 1))
    init[[0, 3], :] = np.nan
    init[5, 1] = np.nan                                       # one NaN: the row holds no estimate
    out, status, flags = run_kernel(c, [c.points[i] for i in idx], 2, init)
    has = ~np.isnan(init).any(axis=1)
    rows = np.array([c.rows[2, "init" if h else "free"][i] for i, h in zip(idx, has)])
    st = np.array([c.status[2, "init" if h else "free"][i] for i, h in zip(idx, has)])
    check_rows(c, [c.names[i] for i in idx], out, status, flags, rows, st, 2, "NaN rows")
    assert rows[1, 3] < rows[5, 3]                            # the estimate removed movers where it was given


def test_a_table_row_for_another_point_count_is_flagged():
    c = cases()
    i = c.names.index("clean_64")
    table = c.device_table(c.cap).copy()
    table[64 - 7] = c.draws_of(65)
    assert (c.draws_of(65) == 64).any()
    out, status, flags = run_kernel(c, [c.points[i], c.points[c.names.index("clean_63")]], 2, table=table)
    assert flags[0] == _lib.VEHICLE_FLAG_TABLES and not out[0].any() and status[0] == 0 and flags[1] == 0 and status[1] == 1
    out, status, flags = run_kernel(c, [c.points[i]], 2, table=c.device_table(c.cap)[:50])      # no row for N = 64
    assert flags[0] == _lib.VEHICLE_FLAG_TABLES and not out[0].any()
    table = c.device_table(c.cap).copy()
    assert (table[258 - 7] == -1).all()                       # a row without stored draws is never read for another N
    table[64 - 7] = -1
    out, status, flags = run_kernel(c, [c.points[i]], 2, table=table)
    assert flags[0] == _lib.VEHICLE_FLAG_TABLES
    table = c.device_table(c.cap).copy()
    table[64 - 7, 3, 2] = table[64 - 7, 3, 1]                 # a repeated index
    out, status, flags = run_kernel(c, [c.points[i]], 2, table=table)
    assert flags[0] == _lib.VEHICLE_FLAG_TABLES


@pytest.mark.parametrize("dim", [2, 3])
def test_chained_track_in_one_launch(dim):
    c = cases()
    out, status, flags = run_kernel(c, c.seq, dim, chain=True)
    check_rows(c, [f"frame {f}" for f in range(len(c.seq))], out, status, flags, c.seq_rows[dim], c.seq_status[dim], dim, f"chain dim {dim}")
    # the second half seeded with the first half's last estimate goes the same way
    found = np.nonzero(c.seq_status[dim][:20])[0]
    seed_row = c.seq_rows[dim][found[-1], :dim]
    out2, status2, flags2 = run_kernel(c, c.seq[20:], dim, init=seed_row[None, :], chain=True)
    check_rows(c, [f"frame {f}" for f in range(20, 40)], out2, status2, flags2, c.seq_rows[dim][20:], c.seq_status[dim][20:], dim, "seeded chain")
    nan_seed = np.full((1, dim), np.nan)
    out3, status3, flags3 = run_kernel(c, c.seq[:9], dim, init=nan_seed, chain=True)
    np.testing.assert_array_equal(out3, out[:9])
    # a flagged frame ends the chain: the frames behind it are not reached
    seq = c.seq[:5] + [c.points[c.names.index("range_zero")]] + c.seq[5:9]
    out4, status4, flags4 = run_kernel(c, seq, dim, chain=True)
    np.testing.assert_array_equal(out4[:5], out[:5])
    assert flags4[5] == _lib.VEHICLE_FLAG_NONFINITE and (flags4[6:] == _lib.VEHICLE_FLAG_CHAIN).all() and not flags4[:5].any()
    assert not out4[5:].any() and not status4[5:].any()


def test_more_frames_than_one_grid_pass():
    c = cases()
    names = ("clean_11", "clean_9", "clean_12", "clean_10", "clean_0")
    idx = [c.names.index(n) for n in names]
    F = GRID_MAX + 37
    order = [idx[f % len(idx)] for f in range(F)]
    out, status, flags = run_kernel(c, [c.points[i] for i in order], 3, cap=16)
    assert not flags.any()
    np.testing.assert_array_equal(status, c.status[3, "free"][order])
    np.testing.assert_array_equal(out[:, 4], c.rows[3, "free"][order, 4])
    assert rel_err(out, c.rows[3, "free"][order]) <= c.rel_tol
    for k in range(len(idx), F):                                # every pass computes what the first one did
        assert np.array_equal(out[k], out[k % len(idx)]), k


def make_pipe(n, cap):
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(num_samples=16, num_loops=8))
    return FramePipeline(cm, n, (4, 16, 8), det_capacity=cap)


@pytest.mark.parametrize("dim", [2, 3])
def test_flagged_frames_come_back_equal_to_the_host_path(dim):
    c = cases()
    names = DEGENERATE + ("clean_64", "half_movers", "clean_9")
    idx = [c.names.index(n) for n in names]
    pts = [c.points[i] for i in idx]
    pipe = make_pipe(len(pts), c.cap)
    est = VehicleVelEstimator(seed=c.seed)
    for initial, tag in ((None, "free"), (np.tile(c.init[dim], (len(pts), 1)), "init")):
        with np.errstate(all="ignore"):
            fits, status = pipe.vehicle_fits(est, pts, initial, only_2D=dim == 2)
        assert pipe.n_vehicle_flagged == 2 and pipe.vehicle_flags[:2].all() and not pipe.vehicle_flags[2:].any()
        assert pipe.vehicle_seed == c.seed and est.best_fit is None and est.best_error == np.inf
        for k in range(2):
            host = VehicleVelEstimator(seed=c.seed)
            with np.errstate(all="ignore"):
                found, kept = host.ransac(pts[k], np.empty(0) if initial is None else initial[k], dim == 2)
            want = np.r_[host.get_vehicle_vel_est(), host.best_error, kept] if found else np.r_[np.zeros(dim + 1), kept]
            assert status[k] == int(found) and np.array_equal(fits[k], want), (names[k], fits[k], want)
        check_rows(c, names[2:], fits[2:], status[2:], pipe.vehicle_flags[2:], c.rows[dim, tag][idx[2:]], c.status[dim, tag][idx[2:]], dim,
                   f"pipeline {tag}")


@pytest.mark.parametrize("dim", [2, 3])
def test_pipeline_track_in_one_call_in_two_and_across_a_flagged_frame(dim):
    c = cases()
    pipe = make_pipe(len(c.seq) + 1, c.cap)
    est = VehicleVelEstimator(seed=c.seed)
    one = pipe.vehicle_velocities(est, c.seq, track=True, only_2D=dim == 2)
    assert pipe.n_vehicle_flagged == 0 and one.shape == (len(c.seq), dim)
    np.testing.assert_array_equal(np.isnan(one[:, 0]), c.seq_status[dim] == 0)
    ok = c.seq_status[dim] == 1
    assert rel_err(one[ok], c.seq_rows[dim][ok, :dim]) <= c.rel_tol
    last = np.nonzero(ok)[0][-1]
    assert rel_err(est.best_fit, -c.seq_rows[dim][last, :dim]) <= c.rel_tol and rel_err(est.best_error, c.seq_rows[dim][last, dim]) <= c.rel_tol
    first = pipe.vehicle_velocities(VehicleVelEstimator(seed=c.seed), c.seq[:20], track=True, only_2D=dim == 2)
    seed_row = first[~np.isnan(first[:, 0])][-1]
    second = pipe.vehicle_velocities(VehicleVelEstimator(seed=c.seed), c.seq[20:], initial=seed_row, track=True, only_2D=dim == 2)
    np.testing.assert_array_equal(np.concatenate([first, second]), one)
    # a frame the kernel hands back in the middle of the drive: the host decides it and the chain goes on behind it
    seq = c.seq[:12] + [c.points[c.names.index("range_zero")]] + c.seq[12:]
    host, prev, want = VehicleVelEstimator(seed=c.seed), np.empty(0), []
    with np.errstate(all="ignore"):
        for pts in seq:
            v = host.estimate_ego_vel(pts, prev, only_2D=dim == 2)
            want.append(v if v.size else np.full(dim, np.nan))
            prev = v if v.size else prev
        got = pipe.vehicle_velocities(VehicleVelEstimator(seed=c.seed), seq, track=True, only_2D=dim == 2)
    assert pipe.n_vehicle_flagged == 1 and pipe.vehicle_flags[12] == _lib.VEHICLE_FLAG_NONFINITE
    want = np.array(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[12], want[12], equal_nan=True) and rel_err(np.nan_to_num(got), np.nan_to_num(want)) <= c.rel_tol


def test_unseeded_estimator_draws_one_seed_for_the_call():
    c = cases()
    pts = [c.points[c.names.index(n)] for n in ("clean_257", "clean_65")]    # scenes in which any draw finds a consensus
    pipe = make_pipe(2, c.cap)
    got = pipe.vehicle_velocities(VehicleVelEstimator(), pts)
    assert isinstance(pipe.vehicle_seed, int)
    want = [VehicleVelEstimator(seed=pipe.vehicle_seed).estimate_ego_vel(p) for p in pts]
    for f in range(2):                          # a frame the kernel hands back is the host path's own result
        assert want[f].shape == (2,) and rel_err(got[f], want[f]) <= (c.rel_tol if pipe.vehicle_flags[f] == 0 else 0.0)
