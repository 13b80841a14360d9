"""Host side of the vehicle velocity estimator (no device): the mirrored class against the reference-generated fixture (results,
state, empty results, the chained drive), the draw table against ``default_rng(seed).permutation``, the refused arguments, the new
C entry in the header, the ctypes table, the Makefile and the built library, its argument checks through ctypes and, host-only,
under AddressSanitizer + UndefinedBehaviorSanitizer, and the state scan / multi-device join of the batch forms."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from vehicle_vel_cases import DEGENERATE, PARAMS, cases, rel_err, restate_frame
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.batch import FramePipeline, MultiDeviceFramePipeline, vehicle_state_scan
from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator, ransac_tables as T

ENTRY = "mmw_vehicle_velocity_ransac"
NAMES = ["ctx", "d_points", "d_counts", "n_frames", "cap", "dim", "points_per_fit", "max_iters", "fit_thresh", "num_close_pts",
         "static_vel_thresh", "d_init", "d_draws", "n_tab", "chain", "d_out", "d_status", "d_flags"]


def test_public_surface_matches_the_reference_class():
    sig = inspect.signature(VehicleVelEstimator.__init__)
    assert {k: p.default for k, p in sig.parameters.items() if k != "self"} == dict(PARAMS, seed=None)
    est = VehicleVelEstimator()
    assert est.best_fit is None and est.best_error == np.inf
    assert [getattr(est, k) for k in PARAMS] == list(PARAMS.values())
    for name in ("lsq_fit_2D", "lsq_predict", "square_error_loss", "mean_square_error", "get_static_detections",
                 "estimate_ego_vel", "get_vehicle_vel_est"):
        assert callable(getattr(est, name))
    sig = inspect.signature(est.estimate_ego_vel)
    assert list(sig.parameters) == ["detections", "initial_ego_vel_est", "only_2D"] and sig.parameters["only_2D"].default is True
    assert sig.parameters["initial_ego_vel_est"].default.shape == (0,)
    assert inspect.signature(est.lsq_fit_2D).parameters["only_2D"].default is True


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tag", ["free", "init"])
def test_host_class_against_the_fixture(dim, tag):
    c = cases()
    init = c.init[dim] if tag == "init" else None
    rows, status = c.rows[dim, tag], c.status[dim, tag]
    assert sorted(c.counts[:10].tolist()) == [0, 9, 10, 11, 12, 63, 64, 65, 257, c.cap]
    for i, name in enumerate(c.names):
        if name in DEGENERATE:
            continue
        est = VehicleVelEstimator(seed=c.seed)
        got = est.estimate_ego_vel(c.points[i], *(() if init is None else (init,)), only_2D=dim == 2)
        assert got.shape == ((dim,) if status[i] else (0,)), name
        if status[i]:
            assert rel_err(np.r_[got, est.best_error], rows[i, :dim + 1]) <= c.rel_tol, name
            assert np.array_equal(est.get_vehicle_vel_est(), got) and np.array_equal(est.best_fit, -1 * got)
        mine = restate_frame(c.points[i], init, dim, c.draws_of, **PARAMS)
        assert mine["status"] == status[i] and mine["kept"] == rows[i, dim + 1], name
        assert rel_err(np.r_[mine["vel"], mine["err"]], rows[i, :dim + 1]) <= c.rel_tol, name
        found, kept = VehicleVelEstimator(seed=c.seed).ransac(c.points[i], np.empty(0) if init is None else init, dim == 2)
        assert (int(found), kept) == (status[i], rows[i, dim + 1]), name
    by = dict(zip(c.names, range(len(c.names))))
    assert status[by["clean_11"]] == 1 and not status[by["clean_10"]] and not status[by["no_consensus"]]   # strict: > num_close_pts
    assert 60 <= rows[by["half_movers"], dim + 1] <= 200
    assert rows[by["short_movers"], dim + 1] == 9 and not status[by["short_movers"]]      # empty before the filter is asked


def test_best_fit_survives_an_empty_result_and_best_error_does_not():
    c = cases()
    by = dict(zip(c.names, range(len(c.names))))
    est = VehicleVelEstimator(seed=c.seed)
    first = est.estimate_ego_vel(c.points[by["clean_64"]])
    fit, err = est.best_fit.copy(), est.best_error
    assert first.shape == (2,) and np.isfinite(err)
    assert est.estimate_ego_vel(c.points[by["clean_9"]]).shape == (0,)           # too few points: nothing is touched
    assert np.array_equal(est.best_fit, fit) and est.best_error == err
    assert est.estimate_ego_vel(c.points[by["no_consensus"]]).shape == (0,)      # no consensus: the error is reset, the fit stays
    assert np.array_equal(est.best_fit, fit) and est.best_error == np.inf
    assert np.array_equal(est.get_vehicle_vel_est(), first)
    movers_only = est.estimate_ego_vel(c.points[by["clean_64"]], np.array([40.0, 0.0]))   # the filter leaves too few
    assert movers_only.shape == (0,) and est.best_error == np.inf
    # seeded calls repeat; unseeded calls draw afresh and still find the scene's velocity
    again = VehicleVelEstimator(seed=c.seed).estimate_ego_vel(c.points[by["clean_64"]])
    assert np.array_equal(again, first)
    free = VehicleVelEstimator().estimate_ego_vel(c.points[by["clean_257"]])
    assert free.shape == (2,) and np.abs(free - c.rows[2, "free"][by["clean_257"], :2]).max() < 0.05


@pytest.mark.parametrize("dim", [2, 3])
def test_chained_drive_against_the_fixture(dim):
    c = cases()
    est, last = VehicleVelEstimator(seed=c.seed), np.empty(0)
    assert (c.seq_counts == 0).sum() >= 3 and ((c.seq_counts > 0) & (c.seq_counts < 10)).sum() >= 2
    for f, pts in enumerate(c.seq):
        got = est.estimate_ego_vel(pts, last, only_2D=dim == 2)
        assert got.size == dim * c.seq_status[dim][f], f
        if got.size:
            assert rel_err(np.r_[got, est.best_error], c.seq_rows[dim][f, :dim + 1]) <= c.rel_tol, f
            last = got
    fits, status = c.seq_rows[dim], c.seq_status[dim]
    scan = VehicleVelEstimator()
    out = vehicle_state_scan(scan, fits, status)
    assert out.shape == (len(fits), dim) and np.array_equal(np.isnan(out[:, 0]), status == 0)
    assert rel_err(scan.best_fit, est.best_fit) <= c.rel_tol and rel_err(scan.best_error, est.best_error) <= c.rel_tol


def test_vehicle_draws_are_the_heads_of_the_generator_s_permutations():
    c = cases()
    for n in (7, 10, 11, 64, 300):
        rng = np.random.default_rng(c.seed)
        want = np.array([rng.permutation(n)[:7] for _ in range(100)])
        got = T.vehicle_draws(c.seed, n, 100, 7)
        assert got.dtype == np.int32 and got.shape == (100, 7) and np.array_equal(got, want) and not got.flags.writeable
        assert T.vehicle_draws(c.seed, n, 100, 7) is got
    for n, stored in zip(c.table_n, c.table_draws):
        assert np.array_equal(T.vehicle_draws(c.seed, n, 100, 7), stored)
    assert T.vehicle_draws(3, 20, 5, 4).shape == (5, 4) and not np.array_equal(T.vehicle_draws(3, 20, 5, 4), T.vehicle_draws(4, 20, 5, 4))
    assert not np.array_equal(T.vehicle_draws(None, 50, 20, 7), T.vehicle_draws(None, 50, 20, 7))
    with pytest.raises(ValueError):
        T.vehicle_draws(1, 6, 100, 7)
    tab = T.vehicle_tables(c.seed, [12, 30, 5, 99], 30, 100, 7)
    assert tab.shape == (24, 100, 7) and np.array_equal(tab[5], T.vehicle_draws(c.seed, 12, 100, 7))
    assert np.array_equal(tab[23], T.vehicle_draws(c.seed, 30, 100, 7)) and (np.delete(tab, [5, 23], axis=0) == -1).all()
    assert T.vehicle_tables(c.seed, [], 0, 100, 7).shape == (1, 100, 7)
    for seed in range(T.VEHICLE_CACHE_TABLES // 64 + 2):                      # per-call seeds do not pile up
        for n in range(8, 72):
            T.vehicle_draws(10_000 + seed, n, 2, 7)
    assert len(T._vehicle) <= T.VEHICLE_CACHE_TABLES


def test_refused_arguments():
    with pytest.raises(ValueError, match="num_close_pts"):
        VehicleVelEstimator(points_per_fit=7, num_close_pts=6)
    VehicleVelEstimator(points_per_fit=7, num_close_pts=7)
    fp = FramePipeline.__new__(FramePipeline)        # no context, no buffers: a refused call must not need them
    fp.n_frames = 3
    est = VehicleVelEstimator(seed=1)
    for initial, track in ((np.zeros((3, 3)), False), (np.zeros(2), False), (np.zeros((3, 2)), True), (np.zeros(3), True)):
        with pytest.raises(ValueError, match="initial"):
            fp.vehicle_fits(est, None, initial, track, True)
    with pytest.raises(ValueError, match="initial"):
        fp.vehicle_fits(est, [np.empty((0, 4))] * 2, np.zeros((3, 2)))


def test_entry_is_declared_bound_built_and_leaves_the_abi_revision():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmwgpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % ENTRY, text)
    assert m, f"{ENTRY} is not declared in include/mmwgpu.h"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == NAMES
    assert ENTRY in _lib.EXPORTED and len(_lib._SIGNATURES[ENTRY]) == len(NAMES)
    lib = _lib.load_library()
    assert hasattr(lib, ENTRY) and lib.mmw_abi_version() == _lib.ABI_VERSION == 7
    assert re.search(r"#define\s+MMWGPU_ABI_VERSION\s+7\b", text)
    for name in ("RESIDUAL", "STATIC", "ERROR_TIE", "COND", "NONFINITE", "TABLES", "CHAIN"):
        m = re.search(r"#define\s+MMW_VEHICLE_FLAG_%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, f"VEHICLE_FLAG_{name}")
    make = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS = .*\bmmw_tu_vehicle_vel\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_vehicle_vel\.o:.*-ffp-contract=off", make, flags=re.M)


def test_entry_refuses_bad_arguments_without_a_device():
    lib = _lib.load_library()
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)       # never dereferenced: the checks come first
    buf = ctypes.create_string_buffer(4096)
    before = buf.raw

    def call(ctx=ctx, points=buf, counts=buf, F=1, cap=16, dim=2, ppf=7, iters=100, fit=0.05, ncp=10, stat=0.2, init=None, draws=buf,
             n_tab=1, chain=0, out=buf, status=buf, flags=buf):
        return lib.mmw_vehicle_velocity_ransac(ctx, points, counts, F, cap, dim, ppf, iters, fit, ncp, stat, init, draws, n_tab, chain,
                                               out, status, flags)

    assert call(F=0) == _lib.MMW_OK and call(F=0, chain=1, dim=3, init=buf) == _lib.MMW_OK
    bad = [dict(ctx=None), dict(points=None), dict(counts=None), dict(draws=None), dict(out=None), dict(status=None), dict(flags=None),
           dict(F=-1), dict(cap=0), dict(cap=-4), dict(n_tab=-1), dict(dim=1), dict(dim=4), dict(ppf=1), dict(dim=3, ppf=2), dict(ncp=6),
           dict(iters=0), dict(iters=-1), dict(fit=float("nan")), dict(stat=float("inf")), dict(chain=2), dict(chain=-1),
           dict(F=0, ncp=6), dict(F=0, dim=5)]
    for kw in bad:
        assert call(**kw) == _lib.MMW_ERR_INVALID, kw
        assert lib.mmw_last_error(), kw
    assert call(cap=4848) == _lib.MMW_ERR_UNSUPPORTED and call(F=0, cap=4848) == _lib.MMW_ERR_UNSUPPORTED and call(F=0, cap=4847) == _lib.MMW_OK
    assert call(iters=1 << 20) == _lib.MMW_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="num_close_pts 6"):
        _lib.check(call(ncp=6))
    assert buf.raw == before


class _FitPart:
    """Host-only stand-in for a per-device FramePipeline: hands out its rows of a prepared fit table and records the call."""

    def __init__(self, fits, status):
        self.fits, self.status, self.lo, self.n, self.n_vehicle_flagged = fits, status, 0, 0, 1

    def vehicle_fits(self, estimator, point_clouds, initial, track, only_2D):
        self.seen = dict(seed=estimator.seed, initial=initial, track=track, only_2D=only_2D, point_clouds=point_clouds)
        return self.fits[self.lo:self.lo + self.n], self.status[self.lo:self.lo + self.n]


@pytest.mark.parametrize("world", [1, 3, 8])
def test_multi_device_form_shards_the_batch_and_refuses_a_chain(world):
    from mmwave_radar_processing_amd.batch import shard_bounds
    c = cases()
    fits, status = c.seq_rows[2], c.seq_status[2]
    F = len(fits)
    mp = MultiDeviceFramePipeline(None, max_frames=F, shape=(2, 2, 2), devices=list(range(world)),
                                  part_factory=lambda d, n: _FitPart(fits, status))
    mp._set_frames(F)
    for r, part in enumerate(mp.parts):
        lo, hi = shard_bounds(F, r, world)
        part.lo, part.n = lo, hi - lo
    init = np.arange(2.0 * F).reshape(F, 2)
    est, one = VehicleVelEstimator(), VehicleVelEstimator()
    got = mp.vehicle_velocities(est, initial=init)
    np.testing.assert_array_equal(got, vehicle_state_scan(one, fits, status))
    assert np.array_equal(est.best_fit, one.best_fit) and est.best_error == one.best_error and est.seed is None
    assert mp.n_vehicle_flagged == world and len({p.seen["seed"] for p in mp.parts}) == 1 and mp.parts[0].seen["seed"] == mp.vehicle_seed
    for r, part in enumerate(mp.parts):
        lo, hi = shard_bounds(F, r, world)
        assert np.array_equal(part.seen["initial"], init[lo:hi]) and part.seen["track"] is False and part.seen["point_clouds"] is None
    mp.vehicle_velocities(VehicleVelEstimator(seed=5))
    assert mp.vehicle_seed == 5 and mp.parts[0].seen["initial"] is None
    with pytest.raises(ValueError, match="track"):
        mp.vehicle_velocities(est, track=True)
    with pytest.raises(ValueError, match="initial"):
        mp.vehicle_velocities(est, initial=init[:-1])
    mp.close()


def test_argument_checks_under_address_and_ub_sanitizers(tmp_path):
    """mmw_tu_vehicle_vel.hip's host code compiled host-only with AddressSanitizer + UndefinedBehaviorSanitizer and linked with
    tests/cpp/vehicle_vel_sanitize.cpp, a program of its own that launches nothing: every class of refused argument, the LDS
    limit and n_frames == 0 through mmw_vehicle_velocity_ransac.  (No GPU sanitizer is involved; the kernel is a launch stub that
    is never reached.)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    obj = str(tmp_path / "mmw_tu_vehicle_vel.o")
    subprocess.run([hipcc, *flags, "-c", "-o", obj, os.path.join(csrc, "mmw_tu_vehicle_vel.hip")], check=True)
    # the host-only object still refers to its (absent) device code object: an empty stand-in, never launched
    nm = shutil.which("nm") or "/usr/bin/nm"
    undefined = subprocess.run([nm, "-u", obj], capture_output=True, text=True, check=True).stdout
    fatbins = sorted({ln.split()[-1] for ln in undefined.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "fatbin_stubs.cpp"
    stub.write_text("".join(f'extern "C" const char {name}[16] __attribute__((aligned(4096))) = {{0}};\n' for name in fatbins))
    exe = str(tmp_path / "vehicle_vel_sanitize")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "vehicle_vel_sanitize.cpp"), "-x", "c++",
                    str(stub), "-x", "none", obj, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "0 failures" in run.stdout and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
