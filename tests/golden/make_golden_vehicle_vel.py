#!/usr/bin/env python3
"""Generate ``vehicle_vel.npz`` from the IMPORTED reference ``VehicleVelEstimator`` (build container only: the reference never has
to exist where the GPU tests run).

    cd <repo> && PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vehicle_vel.py

The reference draws ``np.random.default_rng()`` unseeded on every call; here the ``np`` of its module is a stand-in whose
``random.default_rng`` returns ``default_rng(SEED)``, so a frame's draws depend on its point count alone.

Stored, for 2-D and 3-D: point clouds (continuous random coordinates), the reference's per-frame (ego velocity, best error, points
behind the static filter, status) without and with an initial estimate, a 40-frame chained track (every frame's estimate is the
next one's initial estimate; empty frames, frames below 10 points, mover-heavy frames), and the draws of every point count used.

Asserted here, on the CPU (``restate_frame`` of tests/vehicle_vel_cases.py): on every ordinary frame no squared residual lies
within the kernel's band of ``fit_thresh`` or ``static_vel_thresh``, and the smallest error is further from every
other member set's than their bands.  ``rel_tol``: ten times the worst distance of that restatement -- the same decisions, sums in
ascending index order, ``np.linalg.solve`` -- from the reference's values.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

import mmwave_radar_processing.point_cloud_processing.vehicle_vel_estimator as ref_module          # noqa: E402
from vehicle_vel_cases import COUNTS, DEGENERATE, PARAMS, restate_frame                             # noqa: E402

CAP = 512
SEED = 20261020
PPF, ITERS = PARAMS["points_per_fit"], PARAMS["max_iters"]


class _PinnedRandom:
    def __getattr__(self, name):
        return getattr(np.random, name)

    @staticmethod
    def default_rng(*_):
        return np.random.default_rng(SEED)


class _PinnedNumpy(types.ModuleType):
    random = _PinnedRandom()

    def __getattr__(self, name):
        return getattr(np, name)


ref_module.np = _PinnedNumpy("numpy")
Reference = ref_module.VehicleVelEstimator

_draws = {}


def draws_of(n):
    if n not in _draws:
        rng = np.random.default_rng(SEED)
        _draws[n] = np.array([rng.permutation(n)[:PPF] for _ in range(ITERS)], dtype=np.int32)
    return _draws[n]


def scene(rng, n, u, noise=0.02, movers=0.0, spread=1.0):
    """n points at continuous random positions in front of the radar; radial speeds of a static scene seen at ego velocity u
    plus noise; a share of them replaced by movers."""
    az = rng.uniform(-spread, spread, n)
    el = rng.uniform(-0.5, 0.5, n)
    r = rng.uniform(0.5, 9.0, n)
    p = np.column_stack((r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)))
    h = p / np.linalg.norm(p, axis=1, keepdims=True)
    v = -(h @ np.asarray(u)) + rng.normal(0.0, noise, n)
    k = int(round(movers * n))
    if k:
        v[rng.permutation(n)[:k]] = rng.uniform(-5.0, 5.0, k)
    return np.column_stack((p, v))


def reference_row(est, points, init, dim):
    """(row [dim + 2], status) of one reference call: ego velocity, best error, points behind the static filter."""
    vel = est.estimate_ego_vel(points, np.empty(0) if init is None else np.asarray(init), only_2D=dim == 2)
    kept = len(points)
    if init is not None and len(points) >= est.num_close_pts:
        kept = len(est.get_static_detections(points, np.asarray(init)))
    row = np.zeros(dim + 2)
    if vel.size:
        row[:dim], row[dim] = vel, est.best_error
    row[dim + 1] = kept
    return row, int(vel.size > 0)


def checked(points, init, dim, row, status, ordinary, what):
    """The restatement's distance from the reference's row (0 for a frame without estimate), after the band assertions."""
    mine = restate_frame(points, init, dim, draws_of, **PARAMS)
    if not ordinary:
        return 0.0
    assert mine["status"] == status and mine["kept"] == row[dim + 1], (what, mine, row)
    assert mine["margin"] > 2.0, (what, "a decision within twice the kernel's band", mine["margin"])
    if not status:
        return 0.0
    got = np.r_[mine["vel"], mine["err"]]
    return float(np.abs(got - row[:dim + 1]).max() / max(1.0, np.abs(row[:dim + 1]).max()))


def degenerate(rng, u, kind):
    """A frame the kernel hands back, on which the reference itself neither raises nor decides anything by an exception."""
    for _ in range(200):
        pts = scene(rng, 40, u)
        if kind == "one_bearing":
            # one bearing to within 5e-5 rad: a Gram matrix far beyond the condition cap that LAPACK still inverts (on exactly
            # one bearing the reference's inv raises LinAlgError, and so does the host class)
            th, ph = rng.uniform(0.1, 0.6) + rng.uniform(-5e-5, 5e-5, 40), rng.uniform(0.1, 0.4) + rng.uniform(-5e-5, 5e-5, 40)
            pts[:, :3] = rng.uniform(0.5, 9.0, 40)[:, None] * np.column_stack((np.cos(ph) * np.cos(th), np.cos(ph) * np.sin(th), np.sin(ph)))
        else:
            pts[int(rng.integers(0, 40)), :3] = 0.0
        try:
            with np.errstate(all="ignore"):
                for dim in (2, 3):
                    Reference().estimate_ego_vel(pts, only_2D=dim == 2)
            return pts
        except np.linalg.LinAlgError:
            continue
    raise SystemExit(f"no {kind} frame on which the reference does not raise")


def main():
    rng = np.random.default_rng(SEED)
    u = np.array([1.2, -0.4, 0.3])
    init = u + np.array([0.1, -0.05, 0.05])
    cases = [(f"clean_{n}", scene(rng, n, u)) for n in COUNTS + (CAP,)]
    cases.append(("half_movers", scene(rng, 200, u, movers=0.5)))
    nocon = scene(rng, 60, u)
    nocon[:, 3] = rng.uniform(-1000.0, 1000.0, 60)
    cases.append(("no_consensus", nocon))
    for kind in DEGENERATE:
        cases.append((kind, degenerate(rng, u, kind)))

    seq = []
    for f in range(40):
        uf = (1.0 + 0.02 * f, -0.3 + 0.01 * f, 0.2)
        if f in (0, 7, 8, 21):
            seq.append(np.empty((0, 4)))
        elif f in (3, 15):
            seq.append(scene(rng, int(rng.integers(1, 10)), uf))
        elif f in (5, 11, 12, 30):
            seq.append(scene(rng, int(rng.integers(40, 200)), uf, movers=0.6))
        else:
            seq.append(scene(rng, int(rng.integers(12, 300)), uf, movers=float(rng.uniform(0.0, 0.2))))

    # after everything else, so that the frames above keep their values: a frame below num_close_pts points with movers in it,
    # which is empty before the static filter is asked (its count is the unfiltered one, with or without an initial estimate)
    short = scene(rng, 9, u)
    short[[1, 4, 6, 8], 3] = (4.0, -3.0, 2.5, -4.5)
    cases.append(("short_movers", short))

    out = {"cap": np.int32(CAP), "seed": np.int64(SEED), "case_names": np.array([c[0] for c in cases]), "case_init": init}
    out["case_counts"] = np.array([len(c[1]) for c in cases], dtype=np.int32)
    out["case_points"] = np.concatenate([c[1] for c in cases])
    out["seq_counts"] = np.array([len(p) for p in seq], dtype=np.int32)
    out["seq_points"] = np.concatenate(seq)
    worst = 0.0
    for dim in (2, 3):
        for tag, ini in (("free", None), ("init", init[:dim])):
            rows, status = [], []
            for name, pts in cases:
                ordinary = name not in DEGENERATE
                with np.errstate(all="ignore"):
                    row, st = reference_row(Reference(), pts, ini, dim) if ordinary else (np.zeros(dim + 2), 0)
                worst = max(worst, checked(pts, ini, dim, row, st, ordinary, (name, dim, tag)))
                rows.append(row), status.append(st)
            out[f"case_rows_{dim}_{tag}"] = np.array(rows)
            out[f"case_status_{dim}_{tag}"] = np.array(status, dtype=np.int32)
        # the drive: one estimator, every found estimate is the next frame's initial estimate
        est, last, rows, status = Reference(), None, [], []
        for f, pts in enumerate(seq):
            row, st = reference_row(est, pts, last, dim)
            worst = max(worst, checked(pts, last, dim, row, st, True, ("seq", f, dim)))
            if st:
                last = row[:dim].copy()
            rows.append(row), status.append(st)
        out[f"seq_rows_{dim}"] = np.array(rows)
        out[f"seq_status_{dim}"] = np.array(status, dtype=np.int32)
        print(dim, "track status", status, "kept", [int(r[dim + 1]) for r in rows])
    sizes = sorted(_draws)
    out["table_n"] = np.array(sizes, dtype=np.int32)
    out["table_draws"] = np.array([_draws[n] for n in sizes], dtype=np.int32)
    out["rel_tol"] = np.float64(10.0 * worst)
    print("worst distance of the restatement from the reference", worst, "-> rel_tol", out["rel_tol"])
    path = os.path.join(HERE, "vehicle_vel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", len(seq), "sequence frames,", len(sizes), "draw tables")
    for key in ("case_status_2_free", "case_status_2_init", "case_status_3_free", "case_status_3_init"):
        print(key, dict(zip(out["case_names"].tolist(), out[key].tolist())))


if __name__ == "__main__":
    main()
