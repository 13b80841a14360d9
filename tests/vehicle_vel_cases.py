"""The vehicle-velocity fixture (tests/golden/vehicle_vel.npz, written by tests/golden/make_golden_vehicle_vel.py) unpacked once for
the host and the GPU tests, and ``restate_frame``: one frame's decision sequence written out in plain NumPy, independent of the
product package and of the reference (the generator measures the fixture's tolerance and its distance from every band with it)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEGENERATE = ("one_bearing", "range_zero")     # the frames the kernel must hand back (rank-deficient, a point at range 0)
PARAMS = dict(points_per_fit=7, max_iters=100, fit_thresh=0.05, num_close_pts=10, static_vel_thresh=0.2)
U = 2.0 ** -53
COUNTS = (0, 9, 10, 11, 12, 63, 64, 65, 257)     # and cap


def unit_rows(points, dim):
    p = points[:, :dim]
    return p / np.sqrt((p * p).sum(axis=1))[:, None]


def cond_bound(G):
    """tr(G)^dim / det(G) >= cond_2(G): the bound the kernels' bands are computed from."""
    det = np.linalg.det(G)
    return np.trace(G) ** len(G) / det if det > 0 else np.inf


def band_coef(n, cond, scale):
    """band_c of a fit over n points: scale = y_max + |c|_1."""
    return 8.0 * (n + 8) * U * cond * scale


def band_residual(band_c, ymax, c1):
    """band_r of a residual on a unit row from the band of its coefficients (0: an estimate that was not fitted)."""
    return band_c + 8.0 * U * (ymax + c1)


def band_sq(r, band_r):
    """band_e of a squared residual."""
    return 2.0 * np.abs(r) * band_r + band_r * band_r + 4.0 * U * r * r


def band_sum_sq(m, band_r, sr, sr2):
    """The band of the sum of m squared residuals: sr = sum |r|, sr2 = sum r^2."""
    return 2.0 * band_r * sr + m * band_r * band_r + (m + 4) * U * sr2


def band_error(m, band_r, sr, sr2):
    """The band of the mean squared error sr2 / m of a refit over m members."""
    return band_sum_sq(m, band_r, sr, sr2) / m + 2.0 * U * (sr2 / m)


def band_r2(m, ymax, band_r, sr2, sr, syy):
    """(band_s, loose) of R^2 = 1 - sr2 / syy over m points, syy = sum (y - ybar)^2; loose: the denominator is not clearly
    non-zero and R^2 is not trusted at all."""
    e = 2.0 * (m + 4) * U * ymax
    db = 2.0 * e * np.sqrt(m * syy) + m * e * e + (m + 4) * U * syy
    loose = not syy > 4.0 * db
    if sr2 == 0.0 or syy == 0.0:
        return 0.0, loose
    return 2.0 * (band_sum_sq(m, band_r, sr, sr2) + (sr2 / syy) * db) / syy, loose


def restate_frame(points, init, dim, draws_of, points_per_fit=7, max_iters=100, fit_thresh=0.05, num_close_pts=10,
                  static_vel_thresh=0.2):
    """One frame: dict(status, vel [dim], err, kept; with an estimate also iter, the winning iteration, and members, its member
    indices among the kept points; cond: the largest condition bound of a Gram matrix solved; margins: ``margin`` apart for the
    static filter, the fit threshold and the choice among near-equal errors) and ``margin``, the smallest (distance from a decision) / (the kernel's band
    there) over every decision taken: above 1 the kernel has no reason to flag the frame.  ``draws_of(n)``: the
    ``[max_iters, points_per_fit]`` draws for n points.  Members are summed in ascending index order, and the systems are solved
    by ``np.linalg.solve``: neither is what the reference does."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    out = dict(status=0, vel=np.zeros(dim), err=0.0, kept=len(pts), margin=np.inf, cond=0.0,
               margins=dict(static=np.inf, residual=np.inf, tie=np.inf))
    ymax = np.abs(pts[:, 3]).max() if len(pts) else 0.0
    if len(pts) >= num_close_pts and init is not None:
        r = pts[:, 3] + unit_rows(pts, dim) @ np.asarray(init, dtype=np.float64)
        e = r * r
        band = band_sq(r, band_residual(0.0, ymax, np.abs(init).sum()))
        out["margins"]["static"] = (np.abs(e - static_vel_thresh) / band).min()
        pts = pts[e < static_vel_thresh]
    n = out["kept"] = len(pts)
    if n < num_close_pts:
        out["margin"] = min(out["margins"].values())
        return out
    H, y = unit_rows(pts, dim), pts[:, 3]
    found = []
    for it, drawn in enumerate(np.asarray(draws_of(n))[:max_iters]):
        Hd, yd = H[drawn], y[drawn]
        G = Hd.T @ Hd
        c = np.linalg.solve(G, Hd.T @ yd)
        c1 = np.abs(c).sum()
        band_r = band_residual(band_coef(points_per_fit, cond_bound(G), ymax + c1), ymax, c1)
        r = y - H @ c
        e = r * r
        others = np.ones(n, dtype=bool)
        others[drawn] = False
        out["cond"] = max(out["cond"], cond_bound(G))
        out["margins"]["residual"] = min(out["margins"]["residual"], (np.abs(e - fit_thresh) / band_sq(r, band_r))[others].min(initial=np.inf))
        member = ~others | (e < fit_thresh)
        m = int(member.sum())
        if m > num_close_pts:
            Hm, ym = H[member], y[member]
            G = Hm.T @ Hm
            c2 = np.linalg.solve(G, Hm.T @ ym)
            r = ym - Hm @ c2
            err = (r * r).sum() / m
            c1 = np.abs(c2).sum()
            out["cond"] = max(out["cond"], cond_bound(G))
            band_r = band_residual(band_coef(m, cond_bound(G), ymax + c1), ymax, c1)
            band = band_error(m, band_r, np.abs(r).sum(), (r * r).sum())
            found.append((err, it, c2, band, member))
    if found:
        err, it, c2, band, member = min(found, key=lambda t: (t[0], t[1]))
        for e2, it2, _, band2, member2 in found:
            if it2 != it and not np.array_equal(member, member2):
                out["margins"]["tie"] = min(out["margins"]["tie"], (e2 - err) / (band + band2))
        out.update(status=1, vel=-c2, err=float(err), iter=it, members=np.flatnonzero(member))
    out["margin"] = min(out["margins"].values())
    return out


class Cases:
    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "vehicle_vel.npz"), allow_pickle=False)
        self.cap, self.seed, self.rel_tol = int(g["cap"]), int(g["seed"]), float(g["rel_tol"])
        self.names = [str(n) for n in g["case_names"]]
        self.counts = g["case_counts"]
        off = np.cumsum(self.counts) - self.counts
        self.points = [g["case_points"][o:o + c] for o, c in zip(off, self.counts)]
        self.init = {2: g["case_init"][:2].copy(), 3: g["case_init"].copy()}
        # [n_cases, dim + 2] rows and [n_cases] status, without and with the initial estimate
        self.rows = {(d, w): g[f"case_rows_{d}_{w}"] for d in (2, 3) for w in ("free", "init")}
        self.status = {(d, w): g[f"case_status_{d}_{w}"] for d in (2, 3) for w in ("free", "init")}
        self.seq_counts = g["seq_counts"]
        off = np.cumsum(self.seq_counts) - self.seq_counts
        self.seq = [g["seq_points"][o:o + c] for o, c in zip(off, self.seq_counts)]
        self.seq_rows = {d: g[f"seq_rows_{d}"] for d in (2, 3)}
        self.seq_status = {d: g[f"seq_status_{d}"] for d in (2, 3)}
        self.table_n = g["table_n"].tolist()
        self.table_draws = g["table_draws"]

    def draws_of(self, n):
        return self.table_draws[self.table_n.index(int(n))]

    def device_table(self, n_max):
        """The d_draws argument from the STORED draws: row N - 7 serves N, -1 where no draws are stored."""
        ppf = PARAMS["points_per_fit"]
        tab = np.full((max(n_max - ppf + 1, 1), PARAMS["max_iters"], ppf), -1, dtype=np.int32)
        for n, d in zip(self.table_n, self.table_draws):
            if ppf <= n <= n_max:
                tab[n - ppf] = d
        return tab


_cases = None


def cases() -> Cases:
    global _cases
    if _cases is None:
        _cases = Cases()
    return _cases


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0
