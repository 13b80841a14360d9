"""The crafted frames of ``lsq_band_cases`` on the host (no device): these tests prove the builders, not the kernels.  Every intended
distance holds by the exact reference (the builders assert it while they build), the two NumPy restatements raise the flag each frame
is built for and no other, the host estimators -- scikit-learn's RANSAC for the ego estimator, the mirrored vehicle class with
the stored draws -- decide every "far" variant as the exact reference says, and the Python bands equal mmw_lsq_core.h's, which a
small program of its own (tests/cpp/lsq_core_bands.cpp, host-only, under AddressSanitizer + UndefinedBehaviorSanitizer) prints."""
import os
import shutil
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import lsq_band_cases as L
from conftest import ROOT
from vehicle_vel_cases import (PARAMS, U, band_coef, band_r2, band_residual, band_sq, band_sum_sq, cases as veh_cases, restate_frame)
from mmwave_radar_processing_amd.point_cloud_processing import VehicleVelEstimator
from mmwave_radar_processing_amd.point_cloud_processing.vel_estimator import ransac_fit

DIMS = (2, 3)


def have_sklearn():
    try:
        import sklearn  # noqa: F401
        return True
    except ImportError:
        return False


def ego_frames(dim):
    return (L.condition_sweep("ego", dim) + L.ego_residual_cases(dim) + L.ego_tie_cases(dim) + L.ego_same_set_case(dim)
            + L.ego_r2_cases(dim))


def veh_frames(dim):
    return (L.condition_sweep("veh", dim) + L.veh_residual_cases(dim, 65, 2) + L.veh_residual_cases(dim, 11, 0) + L.veh_static_cases(dim)
            + L.veh_tie_cases(dim) + L.veh_same_set_case(dim))


def veh_restate(f):
    return restate_frame(f.points, getattr(f, "init", None), f.dim, veh_cases().draws_of, **PARAMS)


def test_exact_reference_on_a_system_with_a_known_solution():
    pts = np.array([[3.0, 4.0, 0.0, 0.0], [4.0, -3.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0]])
    ex = L.Exact(pts, 2, 1.0)
    assert ex.rows[0] == [Fr(0.6), Fr(0.8)] and ex.rows[3] == [Fr(0), Fr(1)]
    c = [Fr(3, 7), Fr(-5, 3)]
    pts[:, 3] = [float(sum(h * x for h, x in zip(r, c))) for r in ex.rows]
    ex = L.Exact(pts, 2, 1.0)
    fit = ex.fit(range(4))
    assert L.distance([3 / 7, -5 / 3], fit.c) < 4 * U and float(ex.sums(fit.c, range(4)).mse) < U * U
    pts[2, 3] += 1.0                                              # G = [[2, 0], [0, 2]]: the residual splits in halves
    ex = L.Exact(pts, 2, 1.0)
    fit = ex.fit(range(4))
    assert abs(float(fit.c[0] - c[0]) - 0.5) < 4 * U and fit.cond == 4.0 and abs(float(ex.residual(fit.c, 2)) - 0.5) < 4 * U
    assert L.sqrt_fr(Fr(1, 4)) == Fr(1, 2) and abs(float(L.sqrt_fr(2) ** 2 - 2)) < 1e-60
    ex3 = L.Exact(np.array([[1.0, 2.0, 2.0, 3.0], [2.0, 1.0, -2.0, 1.0], [2.0, -2.0, 1.0, -2.0]]), 3, -1.0)
    fit = ex3.fit(range(3))                                       # an orthonormal system: c = H^T y, cond = 27
    assert fit.cond == 27.0 and L.distance([-1 / 3, -11 / 3, -2 / 3], fit.c) < 8 * U


@pytest.mark.parametrize("dim", DIMS)
def test_ego_frames_hold_their_distances_and_flags(dim):
    frames = ego_frames(dim)
    assert {f.flag for f in frames} == {0, L.EGO_FLAG_RESIDUAL, L.EGO_FLAG_SCORE_TIE, L.EGO_FLAG_R2, L.EGO_FLAG_COND}
    for f in frames:
        r = L.ego_restate(f.points, dim, r2_thr=getattr(f, "r2_thr", 0.6))
        assert r["flag"] == f.flag, (f.name, r["flag"], f.flag)
        if not f.flag:
            assert r["margin"] >= 2.0, (f.name, r["margin"])     # nothing else in the frame is near a decision
        k = getattr(f, "k", None)
        if k is not None:
            assert (abs(f.dist) <= 0.5) if abs(k) <= 0.25 else (abs(f.dist) >= 2.0 and abs(abs(f.dist) - 8.0) < 0.1), (f.name, f.dist)
        if getattr(f, "moved", None) is not None and not f.flag:
            assert r["mask"][f.moved] == f.inside, f.name
    same = L.ego_same_set_case(dim)[0]
    assert L.ego_restate(same.points, dim)["same_ties"] >= 1     # the counter-case does tie, with the same set
    sweep = L.condition_sweep("ego", dim)
    assert [f.flag for f in sweep[-2:]] == [0, L.EGO_FLAG_COND] and 0.98e6 <= sweep[-2].cond <= 1e6 < sweep[-1].cond <= 1.02e6
    assert all(a.cond < b.cond for a, b in zip(sweep, sweep[1:])) and sweep[0].cond <= (10 if dim == 2 else 100)
    for f in L.ego_residual_cases(dim):
        assert f.band >= 1e-13
    for f in L.ego_r2_cases(dim)[:-1]:                            # the exact R^2 is the one of the set the frame is built for
        assert np.array_equal(L.ego_restate(f.points, dim, r2_thr=0.6)["mask"], f.mask)
    assert len({len(f.points) for f in frames}) >= 4 and max(len(f.points) for f in frames) <= 512


@pytest.mark.parametrize("dim", DIMS)
def test_vehicle_frames_hold_their_distances_and_flags(dim):
    kind = {L.VEH_FLAG_RESIDUAL: "residual", L.VEH_FLAG_STATIC: "static", L.VEH_FLAG_ERROR_TIE: "tie"}
    frames = veh_frames(dim)
    assert {f.flag for f in frames} == {0, L.VEH_FLAG_RESIDUAL, L.VEH_FLAG_STATIC, L.VEH_FLAG_ERROR_TIE, L.VEH_FLAG_COND}
    for f in frames:
        r = veh_restate(f)
        if f.flag == L.VEH_FLAG_COND:
            assert r["cond"] > L.COND_CAP
            continue
        assert r["cond"] <= L.COND_CAP, f.name
        for name, margin in r["margins"].items():                 # the decision the frame is built for is inside its band,
            if kind.get(f.flag) == name:                          # every other one at least two bands from turning
                assert margin <= 0.5, (f.name, name, margin)
            elif not (f.flag == L.VEH_FLAG_STATIC and name != "static"):       # (behind an undecided filter nothing is defined)
                assert margin >= 2.0, (f.name, name, margin)
        k = getattr(f, "k", None)
        if k is not None:
            assert (abs(f.dist) <= 0.5) if abs(k) <= 0.25 else (abs(f.dist) >= 2.0 and abs(abs(f.dist) - 8.0) < 0.1), (f.name, f.dist)
            assert f.band >= 1e-13 or "static" in f.name
            if not f.flag and "static" in f.name:
                assert r["kept"] == f.kept and r["status"] == 1
            elif not f.flag:
                drew_it = f.moved in L.veh_draws(len(f.points))[r["iter"]]      # N = 11: most iterations draw the moved point itself
                assert r["status"] == 1 and (drew_it or (f.moved in r["members"]) == f.inside), f.name
    sweep = L.condition_sweep("veh", dim)
    assert [f.flag for f in sweep[-2:]] == [0, L.VEH_FLAG_COND] and 0.98e6 <= sweep[-2].cond <= 1e6 < sweep[-1].cond <= 1.02e6
    for f in sweep:
        assert abs(veh_restate(f)["cond"] / f.cond - 1.0) < 1e-6, f.name    # no member set is conditioned worse than the draws


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("side", [-1, 1])
def test_chain_frames_hold_their_distances(dim, side):
    c = veh_cases()
    ch = L.veh_chain_cases(dim, side)
    assert abs(ch.dist_wide) <= 0.5 and abs(ch.dist_plain) >= 8.0 and (ch.dist_plain < 0) == (side < 0)
    r0 = restate_frame(ch.frames[0], None, dim, c.draws_of, **PARAMS)
    assert r0["status"] == 1 and r0["margin"] >= 2.0 and len(r0["members"]) == 64 and 0.9e5 <= r0["cond"] <= L.COND_CAP
    assert L.distance(r0["vel"], ch.est) <= ch.band_c             # the float refit is within the band the chain carries
    plain = restate_frame(ch.frames[1], ch.seed, dim, c.draws_of, **PARAMS)
    assert plain["kept"] == ch.kept and plain["status"] == 1 and plain["margin"] >= 2.0
    # the float refit in place of the exact one moves the residual by far more than a plain band, and by less than a widened one
    moved = restate_frame(ch.frames[1], r0["vel"], dim, c.draws_of, **PARAMS)
    assert moved["margins"]["static"] >= 2.0 and restate_frame(ch.frames[2], ch.seed, dim, c.draws_of, **PARAMS)["margin"] >= 2.0


@pytest.mark.parametrize("dim", DIMS)
def test_scikit_learn_decides_the_far_ego_variants_as_the_exact_reference(dim):
    if not have_sklearn():
        pytest.skip("the ego estimator's host fit needs scikit-learn")
    for f in ego_frames(dim):
        if f.flag:
            continue
        coef, r2, share, mask = ransac_fit(f.points, dim, return_mask=True)
        want = L.ego_exact(f.points, dim, mask)
        assert L.distance(coef, want.coef) <= want.band_c and abs(float(Fr(float(r2)) - want.r2)) <= want.band_s, f.name
        assert np.array_equal(mask, L.ego_restate(f.points, dim, r2_thr=getattr(f, "r2_thr", 0.6))["mask"]), f.name
        if getattr(f, "moved", None) is not None:
            assert mask[f.moved] == f.inside, f.name
        if hasattr(f, "r2_thr"):
            assert (r2 >= f.r2_thr) == (want.r2 >= Fr(float(f.r2_thr))) == (f.k < 0), f.name


@pytest.mark.parametrize("dim", DIMS)
def test_the_vehicle_class_decides_the_far_variants_as_the_exact_reference(dim):
    c = veh_cases()

    def host(points, init):
        est = VehicleVelEstimator(seed=c.seed)
        found, kept = est.ransac(points, np.empty(0) if init is None else init, dim == 2)
        return est, found, kept
    for f in veh_frames(dim):
        if f.flag:
            continue
        est, found, kept = host(f.points, getattr(f, "init", None))
        r = veh_restate(f)
        assert found == bool(r["status"]) and kept == r["kept"], f.name
        if "static" in f.name:
            assert kept == f.kept
        elif found:
            want = L.veh_exact(f.points, dim, L.veh_draws(len(f.points))[r["iter"]])
            assert L.distance(est.get_vehicle_vel_est(), want.vel) <= want.band_c, f.name
            assert abs(float(Fr(float(est.best_error)) - want.err)) <= want.band_err, f.name
            if getattr(f, "moved", None) is not None and f.moved not in L.veh_draws(len(f.points))[r["iter"]]:
                assert (f.moved in want.members) == f.inside, f.name
    for side in (-1, 1):
        ch = L.veh_chain_cases(dim, side)
        assert host(ch.frames[1], ch.seed)[1:] == (True, ch.kept)


def test_python_bands_equal_the_header_s(tmp_path):
    """tests/cpp/lsq_core_bands.cpp includes mmw_lsq_core.h, compiled host-only with -ffp-contract=off under AddressSanitizer +
    UndefinedBehaviorSanitizer (a program of its own; no GPU sanitizer is involved), and answers the requests below: the bands
    bit for bit, the solve against the exact solution."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-ffp-contract=off", "--cuda-host-only"]
    exe = str(tmp_path / "lsq_core_bands")
    subprocess.run([hipcc, *flags, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "lsq_core_bands.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(3)
    asked, want = [], []

    def ask(name, args, result):
        asked.append(name + " " + " ".join(float(a).hex() for a in args))
        want.append(result)
    for _ in range(40):
        n, m = int(rng.integers(1, 600)), int(rng.integers(2, 600))
        cond, scale, ymax, c1 = 10.0 ** rng.uniform(0, 6.2), rng.uniform(0.1, 30), rng.uniform(0, 20), rng.uniform(0, 10)
        bc, r, br = band_coef(n, cond, scale), rng.normal() * 10.0 ** rng.uniform(-8, 1), 10.0 ** rng.uniform(-16, -6)
        sr, sr2, syy = rng.uniform(0, 50), rng.uniform(0, 10), rng.choice([0.0, 10.0 ** rng.uniform(-30, 3)])
        sr2 = float(rng.choice([0.0, sr2]))
        ask("coef", (n, cond, scale), [bc])
        ask("residual", (bc, ymax, c1), [band_residual(bc, ymax, c1)])
        ask("sq", (r, br), [float(band_sq(r, br))])
        ask("sumsq", (m, br, sr, sr2), [band_sum_sq(m, br, sr, sr2)])
        band, loose = band_r2(m, ymax, br, sr2, sr, syy)
        ask("r2", (m, ymax, br, sr2, sr, syy), [L._r2(sr2, syy), band, float(loose)])
    systems = []
    for dim in DIMS:
        for width in (1.5, 0.05, 0.0):                            # well conditioned, poorly, one bearing (det <= 0 or nonsense)
            H = L.unit_rows(L.fan(7, 12, dim, width), dim)
            y = H @ L.C0[:dim] + 0.01 * rng.normal(size=12)
            g, b = np.zeros(6), np.zeros(3)
            G = np.zeros((3, 3))
            G[:dim, :dim] = H.T @ H
            g[:] = G[0, 0], G[0, 1], G[1, 1], G[0, 2], G[1, 2], G[2, 2]
            b[:dim] = H.T @ y
            systems.append((dim, g, b, float(np.abs(y).max())))
            ask("solve", (dim, *g, *b), None)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input="\n".join(asked) + "\n", capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = [[float.fromhex(t) if t not in ("inf", "nan", "-nan") else float(t.strip("-")) for t in ln.split()] for ln in run.stdout.splitlines()]
    assert len(got) == len(asked) and f"{len(asked)} requests" in run.stderr
    solves = iter(systems)
    for line, g, w in zip(asked, got, want):
        if w is not None:
            assert g == w, (line, g, w)                           # the same operations in the same order: the same bits
            continue
        dim, gram, b, ymax = next(solves)
        G = [[Fr(float(gram[k])) for k in row] for row in ([[0, 1], [1, 2]] if dim == 2 else [[0, 1, 3], [1, 2, 4], [3, 4, 5]])]
        det = L._det(G)
        if det <= 0:
            assert g[3] == np.inf, line
            continue
        c = [L._det([[Fr(float(b[r])) if k == col else G[r][k] for k in range(dim)] for r in range(dim)]) / det for col in range(dim)]
        cond = float(sum(G[a][a] for a in range(dim)) ** dim / det)
        if cond > 1e12:                                           # one bearing: beyond the cap whatever the rounding of det
            assert g[3] > L.COND_CAP, line
            continue
        assert abs(g[3] / cond - 1.0) <= 64 * U * cond and (dim == 3 or g[2] == 0.0), line
        if cond <= L.COND_CAP:                                    # the adjugate's own error on the rounded system: within band_c
            c1 = float(sum(abs(x) for x in c))
            assert L.distance(g[:dim], c) <= band_coef(12, cond, ymax + c1), (line, g, [float(x) for x in c])
