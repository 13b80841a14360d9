"""Crafted frames (built once per process; treat them as read-only) for the rounding bands of the ego and the vehicle velocity estimators, and the exact
reference they are measured with.

``Exact`` forms a frame's unit rows as the kernels do (float64, each step rounded) and then computes in rational arithmetic:
least-squares solutions, residuals, sums, R^2, mean squared errors.  The bands are those of ``vehicle_vel_cases`` (one restatement
for the host and the GPU tests).  ``ego_restate`` walks scikit-learn's trial loop in plain NumPy as ``restate_frame`` walks the
vehicle class's.  Every builder returns frames with the flag each must raise (0: none) and, from the exact reference, the distance
of its critical decision from turning in units of the band.  Only point counts whose subset and draw tables are stored in the two
fixtures are used, so nothing here imports scikit-learn or the reference."""
from fractions import Fraction as Fr
from functools import lru_cache
from math import isqrt
from types import SimpleNamespace as NS

import numpy as np

import egovel_cases as E
import vehicle_vel_cases as V
from vehicle_vel_cases import (PARAMS, band_coef, band_error, band_r2, band_residual, band_sq, cond_bound, restate_frame)

COND_CAP = 1e6                    # csrc/mmw_lsq_core.h LSQ_COND_CAP
EGO_THR = 0.15                    # the ego estimator's residual threshold
EGO_FLAG_RESIDUAL, EGO_FLAG_SCORE_TIE, EGO_FLAG_R2, EGO_FLAG_COND, EGO_FLAG_NONFINITE, EGO_FLAG_TABLES = 1, 2, 4, 8, 16, 32
VEH_FLAG_RESIDUAL, VEH_FLAG_STATIC, VEH_FLAG_ERROR_TIE, VEH_FLAG_COND, VEH_FLAG_CHAIN = 1, 2, 4, 8, 64   # _lib.VEHICLE_FLAG_*
SWEEP = (1e1, 1e2, 1e3, 1e4, 1e5, 0.99e6, 1.01e6)     # condition bounds asked of the sweep: the last two straddle the cap
OFFSETS = (0.0, 0.25, -0.25, 8.0, -8.0)               # of a threshold decision, in bands: |k| <= 1/4 must flag, 8 must not
FIT_THR, STATIC_THR, NCP = PARAMS["fit_thresh"], PARAMS["static_vel_thresh"], PARAMS["num_close_pts"]


# ------------------------------------------------------------------------------------------------------- exact reference
def unit_rows(points, dim):
    """p / sqrt(x^2 + y^2 [+ z^2]), the sum left to right, every step one float64 operation: lsq_load_unit_rows' values."""
    p = np.asarray(points, dtype=np.float64)
    ss = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
    if dim == 3:
        ss = ss + p[:, 2] * p[:, 2]
    return p[:, :dim] / np.sqrt(ss)[:, None]


def _det(m):
    if len(m) == 2:
        return m[0][0] * m[1][1] - m[0][1] * m[1][0]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def sqrt_fr(x, bits=240):
    """sqrt of a rational to 2^-bits."""
    x = Fr(x)
    return Fr(isqrt((x.numerator << (2 * bits)) // x.denominator), 1 << bits)


class Exact:
    """One point list: float64 unit rows and values y = sign * v, then rational arithmetic on them."""

    def __init__(self, points, dim, sign):
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
        self.dim, self.H, self.y = dim, unit_rows(pts, dim), sign * pts[:, 3]
        self.rows = [[Fr(x) for x in h] for h in self.H.tolist()]
        self.vals = [Fr(v) for v in self.y.tolist()]
        self.ymax = float(np.abs(self.y).max())

    def fit(self, idx):
        """The exact least-squares solution over the rows idx (Cramer on the normal equations, which are exact here), the
        condition bound tr^dim / det of its Gram matrix and the bands of a fit over these points."""
        idx, d = [int(i) for i in idx], self.dim
        G = [[sum(self.rows[i][a] * self.rows[i][b] for i in idx) for b in range(d)] for a in range(d)]
        b = [sum(self.rows[i][a] * self.vals[i] for i in idx) for a in range(d)]
        det = _det(G)
        c = [_det([[b[r] if k == col else G[r][k] for k in range(d)] for r in range(d)]) / det for col in range(d)]
        cond = float(sum(G[a][a] for a in range(d)) ** d / det) if det > 0 else np.inf
        c1 = float(sum(abs(x) for x in c))
        bc = band_coef(len(idx), cond, self.ymax + c1)
        return NS(c=c, n=len(idx), cond=cond, c1=c1, band_c=bc, band_r=band_residual(bc, self.ymax, c1))

    def residual(self, c, i):
        return self.vals[i] - sum(h * x for h, x in zip(self.rows[i], c))

    def sums(self, c, idx):
        """Of the residuals of the rows idx from c: m, sum r^2, sum |r|, sum (y - ybar)^2, R^2 (None: no variance), mse."""
        idx = [int(i) for i in idx]
        r = [self.residual(c, i) for i in idx]
        m = len(idx)
        ybar = sum(self.vals[i] for i in idx) / m
        syy = sum((self.vals[i] - ybar) ** 2 for i in idx)
        sr2 = sum(x * x for x in r)
        return NS(m=m, sr2=sr2, sr=sum(abs(x) for x in r), syy=syy, r2=1 - sr2 / syy if syy else None, mse=sr2 / m)


def distance(got, want):
    """|got - want|_2 of float64 values from rationals, rounded once."""
    return float(sqrt_fr(sum((Fr(float(g)) - w) ** 2 for g, w in zip(got, want)), 1200))


def ego_exact(points, dim, mask):
    """What the ego kernel returns for the inlier set mask, exactly, with band_c of the refit and band_s of its R^2."""
    ex = Exact(points, dim, -1.0)
    idx = np.flatnonzero(mask)
    fit = ex.fit(idx)
    s = ex.sums(fit.c, idx)
    band_s, loose = band_r2(s.m, ex.ymax, fit.band_r, float(s.sr2), float(s.sr), float(s.syy))
    return NS(coef=fit.c, r2=s.r2, band_c=fit.band_c, band_s=band_s, loose=loose, cond=fit.cond, share=len(idx) / len(mask))


def veh_exact(points, dim, drawn):
    """What the vehicle kernel returns when the iteration that drew ``drawn`` wins, exactly: the members from the exact first fit,
    the exact refit (the vehicle's velocity is its negative) and its mean squared error, with band_c and the error's band."""
    ex = Exact(points, dim, 1.0)
    first = ex.fit(drawn)
    drawn = set(int(i) for i in drawn)
    members = [i for i in range(len(ex.vals)) if i in drawn or ex.residual(first.c, i) ** 2 < Fr(FIT_THR)]
    fit = ex.fit(members)
    s = ex.sums(fit.c, members)
    return NS(vel=[-x for x in fit.c], err=s.mse, members=members, band_c=fit.band_c, cond=fit.cond, refit=fit,
              band_err=band_error(s.m, fit.band_r, float(s.sr), float(s.sr2)))


# ------------------------------------------------------------------------------------------------------- tables, restatement
def ego_tables(n):
    """(subsets [20, 10], trials [n + 1]) stored for n points."""
    c = E.cases()
    k = int(np.nonzero(c.table_n == n)[0][0])
    return np.asarray(c.table_subsets[k]), np.asarray(c.table_trials[k])


def veh_draws(n):
    return np.asarray(V.cases().draws_of(n))


def _r2(sr2, syy):
    return 1.0 if sr2 == 0.0 else 0.0 if syy == 0.0 else 1.0 - sr2 / syy


def ego_restate(points, dim, r2_thr=0.6, thr=EGO_THR):
    """The ego kernel's decision sequence in plain NumPy (np.linalg.solve, NumPy's summation order): dict(flag: the first flag
    the sequence meets with these bands, 0 none; mask, coef, r2, share; margin: the smallest distance / band over the decisions
    taken; trials: how many ran; same_ties: tied trials that selected the best one's set; cond: the largest condition bound)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    N = len(pts)
    out = dict(flag=0, mask=np.zeros(N, dtype=bool), coef=np.zeros(dim), r2=0.0, share=0.0, margin=np.inf, trials=0, same_ties=0,
               cond=0.0)
    if N < 10:
        return out
    sub, tab = ego_tables(N)
    H, y = unit_rows(pts, dim), -pts[:, 3]
    ymax = np.abs(y).max()

    def solve(idx):
        G = H[idx].T @ H[idx]
        cond = cond_bound(G)
        out["cond"] = max(out["cond"], cond)
        if not cond <= COND_CAP:
            return None, 0.0
        c = np.linalg.solve(G, H[idx].T @ y[idx])
        c1 = np.abs(c).sum()
        return c, band_residual(band_coef(len(idx), cond, ymax + c1), ymax, c1)

    def stop(flag):
        out.update(flag=flag, margin=min(out["margin"], 1.0))
        return out

    best, n_best, score_best, band_best, max_trials = None, 1, -np.inf, 0.0, 20
    while out["trials"] < max_trials:
        idx = sub[out["trials"]]
        out["trials"] += 1
        c, band_r = solve(idx)
        if c is None:
            return stop(EGO_FLAG_COND)
        r = np.abs(y - H @ c)
        out["margin"] = min(out["margin"], (np.abs(r - thr) / band_r).min())
        if (np.abs(r - thr) <= band_r).any():
            return stop(EGO_FLAG_RESIDUAL)
        inl = r <= thr
        mi = int(inl.sum())
        if mi < n_best:
            continue
        score, band_s = np.nan, 0.0
        if mi >= 2:
            syy, sr2 = ((y[inl] - y[inl].sum() / mi) ** 2).sum(), (r[inl] ** 2).sum()
            score = _r2(sr2, syy)
            band_s, loose = band_r2(mi, ymax, band_r, sr2, r[inl].sum(), syy)
            band_s = np.inf if loose else band_s
        if mi == n_best and best is not None:
            if np.array_equal(inl, best):
                if abs(score - score_best) <= band_s + band_best:
                    out["same_ties"] += 1
                    continue
            else:
                out["margin"] = min(out["margin"], abs(score - score_best) / (band_s + band_best))
                if abs(score - score_best) <= band_s + band_best:
                    return stop(EGO_FLAG_SCORE_TIE)
        if mi == n_best and score < score_best:
            continue
        best, n_best, score_best, band_best = inl, mi, score, band_s
        max_trials = min(max_trials, int(tab[mi]))
    if best is None:
        return out
    idx = np.flatnonzero(best)
    m = len(idx)
    if m == 1:
        c = H[idx[0]] * y[idx[0]] / (H[idx[0]] @ H[idx[0]])
        band_r = band_residual(band_coef(1, 1.0, ymax + np.abs(c).sum()), ymax, np.abs(c).sum())
    else:
        c, band_r = solve(idx)
        if c is None:
            return stop(EGO_FLAG_COND)
    r2 = 0.0
    if m > 3:
        r = np.abs(y[idx] - H[idx] @ c)
        syy, sr2 = ((y[idx] - y[idx].sum() / m) ** 2).sum(), (r ** 2).sum()
        r2 = _r2(sr2, syy)
        band_s, loose = band_r2(m, ymax, band_r, sr2, r.sum(), syy)
        out["margin"] = min(out["margin"], 0.0 if loose else abs(r2 - r2_thr) / band_s if band_s else np.inf)
        if loose or abs(r2 - r2_thr) <= band_s:
            return stop(EGO_FLAG_R2)
    out.update(mask=best, coef=c, r2=r2, share=m / N)
    return out


# ------------------------------------------------------------------------------------------------------- frames
def fan(seed, n, dim, width, centre=0.5, el_width=None):
    """n points at bearings in a fan of ``width`` radians about ``centre`` (dim 3: also ``el_width``, by default 0.8 width, in
    elevation), ranges 2 .. 40 m; the same seed gives the same pattern at every width."""
    rng = np.random.default_rng(seed)
    u, w, rg, zz = rng.random(n) - 0.5, rng.random(n) - 0.5, rng.uniform(2.0, 40.0, n), rng.uniform(-1.0, 1.0, n)
    az = centre + width * u
    el = 0.15 + (0.8 * width if el_width is None else el_width) * w if dim == 3 else np.zeros(n)
    pts = np.zeros((n, 4))
    pts[:, 0], pts[:, 1] = rg * np.cos(el) * np.cos(az), rg * np.cos(el) * np.sin(az)
    pts[:, 2] = rg * np.sin(el) if dim == 3 else zz
    return pts


def on_model(pts, dim, c0, sign, noise=0.0, seed=0):
    """v so that y = sign * v lies on y = H c0 (to the rounding of the product), plus uniform noise."""
    y = unit_rows(pts, dim) @ np.asarray(c0[:dim])
    if noise:
        y = y + noise * np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, len(y))
    pts[:, 3] = sign * y
    return pts


C0 = np.array([1.6, -0.9, 0.5])          # the model of the crafted frames (ego: the velocity; vehicle: the environment's)


def frame(name, est, dim, points, flag=0, **kw):
    return NS(name=name, est=est, dim=dim, points=points, flag=flag, **kw)


def _outside(n, taken, count, seed):
    free = [i for i in range(n) if i not in set(int(t) for t in taken)]
    return sorted(np.random.default_rng(seed).choice(free, count, replace=False).tolist())


@lru_cache(maxsize=None)
def condition_sweep(est, dim, n=64):
    """Inliers exactly on the model, bearings in a fan whose width puts the largest condition bound of a Gram matrix the kernel
    solves at each value of SWEEP (a value no fan of this pattern reaches: the widest fan; the frame's ``cond`` is the bound it has),
    four far outliers.  est: "ego" (y = -v) or "veh" (y = v)."""
    sign = -1.0 if est == "ego" else 1.0
    if est == "ego":
        sub, tab = ego_tables(n)
        outliers = _outside(n, sub[0], 4, 3)
        sets = [sub[t] for t in range(int(tab[n - 4]))]
    else:
        outliers = _outside(n, (), 4, 3)
        sets = list(veh_draws(n))
    sets.append([i for i in range(n) if i not in outliers])

    def cond_at(width):
        H = unit_rows(fan(11 + dim, n, dim, width), dim)
        return max(cond_bound(H[s].T @ H[s]) for s in sets)

    frames, w_max = [], 2.4
    for target in SWEEP:
        lo, hi = np.log(1e-5), np.log(w_max)                      # the bound falls as the fan opens
        if cond_at(w_max) < target:
            for _ in range(48):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if cond_at(np.exp(mid)) > target else (lo, mid)
        width = float(np.exp(hi if target < COND_CAP else lo))    # at or below the value asked; above it behind the cap
        pts = on_model(fan(11 + dim, n, dim, width), dim, C0, sign)
        pts[outliers, 3] += sign * np.array([5.0, -6.0, 4.5, -5.5])
        cond = cond_at(width)
        if frames and frames[-1].cond == cond:
            continue
        frames.append(frame(f"{est}{dim}_cond_{cond:.3g}", est, dim, pts, EGO_FLAG_COND if cond > COND_CAP else 0, cond=cond,
                            outliers=outliers))
    return frames


def _clean_frame(est, dim, n, seed, n_out, keep_free, width=1.3, noise=0.0):
    """A frame on the model with n_out far outliers at indices outside keep_free; the largest |v| is an outlier's."""
    sign = -1.0 if est == "ego" else 1.0
    pts = on_model(fan(seed, n, dim, width), dim, C0, sign, noise, seed)
    outliers = _outside(n, keep_free, n_out, seed + 1)
    pts[outliers, 3] = sign * np.resize([8.0, -7.0, 7.5], n_out) if n_out else 0.0
    return pts, outliers


@lru_cache(maxsize=None)
def ego_residual_cases(dim):
    """One point outside the subsets of the first trials is moved so that its exact residual from the first trial's exact fit is
    0.15 + k * band for k in OFFSETS, band the largest band_r among the trials that can run and fit inliers only.  Near variants
    (|k| <= 1/4) carry EGO_FLAG_RESIDUAL; far ones none, and ``inside`` says whether the exact residual is within the threshold.
    ``dist``: the exact distance, in that trial's own band, at the trial with the largest band."""
    n, seed = {2: (64, 21), 3: (65, 22)}[dim]                     # patterns in which no later trial has a band four times the widest
    sub, tab = ego_tables(n)
    base, outliers = _clean_frame("ego", dim, n, seed + dim, 3, sub[0])
    j = _outside(n, list(np.concatenate(sub[:3])) + outliers, 1, 5)[0]
    run = range(int(tab[n - 4]))                                  # the trials that run when the moved point is no inlier
    clean = [t for t in run if not set(sub[t].tolist()) & set(outliers + [j])]
    assert clean and clean[0] == 0
    frames = []
    near = [t for t in clean if t < int(tab[n - 3])]               # the trials that run when it is an inlier as well
    band = max(Exact(base, dim, -1.0).fit(sub[t]).band_r for t in near)
    for k in OFFSETS:
        pts = base.copy()
        ex = Exact(pts, dim, -1.0)
        first = ex.fit(sub[0])
        pts[j, 3] = -float(ex.vals[j] - ex.residual(first.c, j) + Fr(EGO_THR) + Fr(k) * Fr(band))
        ex = Exact(pts, dim, -1.0)
        assert ex.ymax > abs(pts[j, 3])
        fits = {t: ex.fit(sub[t]) for t in clean}
        dists = {t: float((abs(ex.residual(f.c, j)) - Fr(EGO_THR)) / Fr(f.band_r)) for t, f in fits.items()}
        widest = max(near, key=lambda t: fits[t].band_r)
        assert fits[widest].band_r >= 1e-13
        if abs(k) <= 0.25:
            assert abs(dists[widest]) <= 0.5 and abs(dists[widest] - k) <= 0.05, (k, dists)
        else:
            assert all(abs(d) >= 2.0 and (d > 0) == (k > 0) for d in dists.values()), (k, dists)
        frames.append(frame(f"ego{dim}_residual_{k:+g}", "ego", dim, pts, EGO_FLAG_RESIDUAL if abs(k) <= 0.25 else 0, moved=j,
                            inside=k < 0, dist=dists[widest], band=fits[widest].band_r, k=k))
    return frames


@lru_cache(maxsize=None)
def veh_residual_cases(dim, n=65, n_out=2):
    """The same at fit_thresh on the squared residual: over every iteration that draws inliers only and not the moved point, band
    is the largest band_e; the moved point's exact squared residual from the first such iteration's exact fit is fit_thresh +
    k * band.  n = 11 has no outlier: a consensus needs all eleven points, so only iterations that draw the moved point can reach one when it is
    outside."""
    draws = veh_draws(n)
    base, outliers = _clean_frame("veh", dim, n, 31 + dim, n_out, ())
    j = _outside(n, outliers, 1, 6)[0]
    clean = [it for it in range(len(draws)) if not set(draws[it].tolist()) & set(outliers + [j])]
    r0 = np.sqrt(FIT_THR)
    probe = base.copy()
    probe[j, 3] += r0                                             # near its final value: y_max, and so the band, may depend on it
    ex = Exact(probe, dim, 1.0)
    band = max(float(band_sq(r0, ex.fit(draws[it]).band_r)) for it in clean)
    frames = []
    for k in OFFSETS:
        pts = base.copy()
        ex = Exact(pts, dim, 1.0)
        first = ex.fit(draws[clean[0]])
        pts[j, 3] = float(ex.vals[j] - ex.residual(first.c, j) + sqrt_fr(Fr(FIT_THR) + Fr(k) * Fr(band)))
        ex = Exact(pts, dim, 1.0)
        fits = {it: ex.fit(draws[it]) for it in clean}
        res = {it: ex.residual(f.c, j) for it, f in fits.items()}
        bands = {it: float(band_sq(float(res[it]), fits[it].band_r)) for it in clean}
        dists = {it: float((res[it] ** 2 - Fr(FIT_THR)) / Fr(bands[it])) for it in clean}
        widest = max(clean, key=lambda it: bands[it])
        assert bands[widest] >= 1e-13
        if abs(k) <= 0.25:
            assert abs(dists[widest]) <= 0.5, (k, dists[widest])
        else:
            assert all(abs(d) >= 2.0 and (d > 0) == (k > 0) for d in dists.values()), (k, min(dists.values()), max(dists.values()))
        frames.append(frame(f"veh{dim}_n{n}_residual_{k:+g}", "veh", dim, pts, VEH_FLAG_RESIDUAL if abs(k) <= 0.25 else 0, moved=j,
                            inside=k < 0, dist=dists[widest], band=bands[widest], k=k, init=None))
    return frames


@lru_cache(maxsize=None)
def veh_static_cases(dim, n=66):
    """An initial estimate is given (the model itself) and one point's exact squared residual from it lies at static_vel_thresh +
    k * band, band the evaluation-only band_e.  One far outlier, which the filter drops, holds y_max.  ``kept``: the points
    behind the filter by the exact decision."""
    init = -C0[:dim]                                              # the vehicle's velocity: the fit's negative
    base, outliers = _clean_frame("veh", dim, n, 41 + dim, 1, ())
    j = _outside(n, outliers, 1, 7)[0]
    ex = Exact(base, dim, 1.0)
    ini = [Fr(float(x)) for x in init]
    r0 = np.sqrt(STATIC_THR)
    band = float(band_sq(r0, band_residual(0.0, ex.ymax, float(np.abs(init).sum()))))
    frames = []
    for k in OFFSETS:
        pts = base.copy()
        on = -sum(h * x for h, x in zip(ex.rows[j], ini))         # v that the estimate explains exactly
        pts[j, 3] = float(on + sqrt_fr(Fr(STATIC_THR) + Fr(k) * Fr(band)))
        e = (Fr(float(pts[j, 3])) - on) ** 2
        dist = float((e - Fr(STATIC_THR)) / Fr(band))
        assert abs(pts[j, 3]) < ex.ymax
        assert abs(dist) <= 0.5 if abs(k) <= 0.25 else (abs(dist) >= 2.0 and (dist > 0) == (k > 0)), (k, dist)
        frames.append(frame(f"veh{dim}_static_{k:+g}", "veh", dim, pts, VEH_FLAG_STATIC if abs(k) <= 0.25 else 0, moved=j,
                            inside=k < 0, kept=n - 1 - (0 if k < 0 else 1), dist=dist, band=band, k=k, init=init.copy()))
    return frames


@lru_cache(maxsize=None)
def veh_chain_cases(dim, side):
    """Three frames of one drive.  Frame 0: every point on the model, a fan narrow enough that its refit's condition bound is
    1e5, so the estimate it hands on carries a large band_c.  Frame 1: one point whose exact squared residual from frame 0's exact
    refit is static_vel_thresh + side * band / 4, band the band_e widened by that band_c: at least eight plain evaluation bands
    away, yet undecided in a chain.  Frame 2: clean.  ``seed``: frame 0's exact refit rounded to float64, the caller's row that
    carries no band."""
    n0, n1 = 64, 66
    seed = {2: 51, 3: 55}[dim]                                    # patterns none of whose 7-point draws passes the cap
    sets = list(veh_draws(n0)) + [np.arange(n0)]
    lo, hi = np.log(1e-5), np.log(2.4)

    def refit_cond(width):
        H = unit_rows(fan(seed + dim, n0, dim, width, el_width=2.0), dim)
        return cond_bound(H.T @ H)
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if refit_cond(np.exp(mid)) > 1e5 else (lo, mid)
    f0 = on_model(fan(seed + dim, n0, dim, float(np.exp(hi)), el_width=2.0), dim, C0, 1.0)
    H0 = unit_rows(f0, dim)
    assert max(cond_bound(H0[s].T @ H0[s]) for s in sets) < 0.9 * COND_CAP
    ex0 = Exact(f0, dim, 1.0)
    refit = ex0.fit(range(n0))
    assert 0.9e5 <= refit.cond <= 1.1e5
    est = [-x for x in refit.c]                                   # the estimate the chain carries, exactly
    f1 = on_model(fan(61 + dim, n1, dim, 1.3), dim, C0, 1.0)
    f1[40, 3] = 8.0                                               # a far outlier, which the filter drops, holds y_max
    f2 = on_model(fan(71 + dim, 64, dim, 1.3), dim, C0, 1.0)
    j = 17
    ex1 = Exact(f1, dim, 1.0)
    r0 = np.sqrt(STATIC_THR)
    c1 = float(sum(abs(x) for x in est))
    plain = float(band_sq(r0, band_residual(0.0, ex1.ymax, c1)))
    wide = float(band_sq(r0, band_residual(refit.band_c, ex1.ymax, c1)))
    on = -sum(h * x for h, x in zip(ex1.rows[j], est))
    f1[j, 3] = float(on + sqrt_fr(Fr(STATIC_THR) + Fr(side) * Fr(wide) / 4))
    assert abs(f1[j, 3]) <= ex1.ymax
    e = (Fr(float(f1[j, 3])) - on) ** 2
    assert abs(e - Fr(STATIC_THR)) <= Fr(wide) / 2 and abs(e - Fr(STATIC_THR)) >= 8 * Fr(plain)
    row = np.array([float(x) for x in est])
    e_seed = (Fr(float(f1[j, 3])) + sum(h * Fr(float(x)) for h, x in zip(ex1.rows[j], row))) ** 2
    assert abs(e_seed - Fr(STATIC_THR)) >= 8 * Fr(plain) and (e_seed < Fr(STATIC_THR)) == (side < 0)
    return NS(dim=dim, frames=[f0, f1, f2], moved=j, seed=row, est=est, kept=n1 - 1 - (0 if side < 0 else 1), side=side,
              dist_wide=float((e - Fr(STATIC_THR)) / Fr(wide)), dist_plain=float((e_seed - Fr(STATIC_THR)) / Fr(plain)),
              band_c=refit.band_c)


def mirror_frame(n, dim, s0, s1, sign, seed, noise=0.01):
    """An involution of the rows that maps the index set s0 onto s1: paired points are reflected in y and share v, rows of both
    sets (and an odd one left over) lie on the axis y = 0.  Every first partner lies on the model (plus noise), so the fit of s1
    is the mirror image of the fit of s0, the two consensus sets are mirror images of equal size -- about half the frame each --
    and their scores and errors are equal in exact arithmetic."""
    s0, s1 = [int(i) for i in s0], [int(i) for i in s1]
    both = [i for i in s0 if i in s1]
    only0, only1 = [i for i in s0 if i not in s1], [i for i in s1 if i not in s0]
    rest = [i for i in range(n) if i not in s0 and i not in s1]
    pairs = list(zip(only0, only1)) + list(zip(rest[0::2], rest[1::2]))
    fixed = both + (rest[-1:] if len(rest) % 2 else [])
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 4))
    c0 = np.array([1.6, 1.0, 0.5])[:dim]

    def place(i, az, mirror_of=None):
        if mirror_of is not None:
            pts[i] = pts[mirror_of] * np.array([1.0, -1.0, 1.0, 1.0])
            return
        rg, el = rng.uniform(2.0, 40.0), rng.uniform(-0.5, 0.5)
        pts[i, :3] = rg * np.cos(el) * np.cos(az), rg * np.cos(el) * np.sin(az), rg * np.sin(el)
        if az == 0.0:
            pts[i, 1] = 0.0
        pts[i, 3] = sign * (unit_rows(pts[i:i + 1], dim)[0] @ c0 + noise * rng.uniform(-1.0, 1.0))
    for a, b in pairs:
        place(a, rng.uniform(0.3, 1.2) * rng.choice([-1.0, 1.0]))
        place(b, None, mirror_of=a)
    for i in fixed:
        place(i, 0.0)
    return pts, [a for a, _ in pairs] + fixed, [b for _, b in pairs] + fixed


@lru_cache(maxsize=None)
def ego_tie_cases(dim, n=64):
    """SCORE_TIE between different sets: the mirror frame on the first two subsets.  The exact scores are equal."""
    sub, tab = ego_tables(n)
    pts, set0, set1 = mirror_frame(n, dim, sub[0], sub[1], -1.0, 81 + dim)
    ex = Exact(pts, dim, -1.0)
    scores = []
    for t, want in ((0, set0), (1, set1)):
        fit = ex.fit(sub[t])
        inl = [i for i in range(n) if abs(ex.residual(fit.c, i)) <= Fr(EGO_THR)]
        assert sorted(inl) == sorted(want) and int(tab[len(inl)]) > 1
        scores.append(ex.sums(fit.c, inl).r2)
    assert scores[0] == scores[1] and sorted(set0) != sorted(set1)
    return [frame(f"ego{dim}_score_tie", "ego", dim, pts, EGO_FLAG_SCORE_TIE, dist=0.0, moved=None)]


@lru_cache(maxsize=None)
def ego_same_set_case(dim, n=11):
    """The counter-case: N = 11 with one far outlier at an index that two of the trials run leave out, so both draw the same ten
    points (in another order), tie within rounding and select the same set: no flag."""
    sub, tab = ego_tables(n)
    run = int(tab[n - 1])
    missing = [int((set(range(n)) - set(s.tolist())).pop()) for s in sub[:run]]
    q = next(i for i in missing if missing.count(i) >= 2)
    pts = on_model(fan(91 + dim, n, dim, 1.3), dim, C0, -1.0, 0.01, 3)
    pts[q, 3] += 6.0
    return [frame(f"ego{dim}_same_set_tie", "ego", dim, pts, 0, moved=q, inside=False)]


@lru_cache(maxsize=None)
def veh_tie_cases(dim, n=64):
    """ERROR_TIE between different sets: the mirror frame on the draws of iterations 0 and 1.  The exact errors are equal."""
    draws = veh_draws(n)
    pts, set0, set1 = mirror_frame(n, dim, draws[0], draws[1], 1.0, 85 + dim)
    a, b = veh_exact(pts, dim, draws[0]), veh_exact(pts, dim, draws[1])
    assert sorted(a.members) == sorted(set0) and sorted(b.members) == sorted(set1) and a.err == b.err and a.err > 0
    assert len(set0) > NCP and sorted(set0) != sorted(set1)
    return [frame(f"veh{dim}_error_tie", "veh", dim, pts, VEH_FLAG_ERROR_TIE, dist=0.0, moved=None, init=None)]


@lru_cache(maxsize=None)
def veh_same_set_case(dim, n=11):
    """The counter-case: every iteration of a noisy N = 11 frame selects all eleven points: equal sets, no flag."""
    pts = on_model(fan(95 + dim, n, dim, 1.3), dim, C0, 1.0, 0.01, 4)
    return [frame(f"veh{dim}_same_set", "veh", dim, pts, 0, moved=None, init=None)]


@lru_cache(maxsize=None)
def ego_r2_cases(dim, n=65):
    """A noisy frame whose refit has R^2 well inside (0, 1): with r2_thr = float(exact R^2) the frame carries EGO_FLAG_R2, with
    r2_thr 8 band_s to either side none.  Last: N = 10 points of one speed (sum (y - ybar)^2 = 0), flagged whatever r2_thr."""
    sub, _ = ego_tables(n)
    pts, outliers = _clean_frame("ego", dim, n, 101 + dim, 3, sub[0], noise=0.04)
    mask = np.ones(n, dtype=bool)
    mask[outliers] = False
    want = ego_exact(pts, dim, mask)
    r2 = float(want.r2)
    assert 0.5 < r2 < 0.9999 and not want.loose and 0 < want.band_s < 1e-9
    frames = [frame(f"ego{dim}_r2_{k:+g}", "ego", dim, pts, EGO_FLAG_R2 if k == 0 else 0, r2_thr=r2 + k * want.band_s, k=k, mask=mask,
                    dist=float((want.r2 - Fr(r2 + k * want.band_s)) / Fr(want.band_s)), moved=None) for k in (0.0, 8.0, -8.0)]
    flat = fan(111 + dim, 10, dim, 0.5, centre=0.0)
    flat[:, 3] = -1.0
    frames.append(frame(f"ego{dim}_one_speed", "ego", dim, flat, EGO_FLAG_R2, r2_thr=0.6, k=None, moved=None))
    return frames
