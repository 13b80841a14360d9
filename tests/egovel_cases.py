"""The ego-velocity fixture (tests/golden/egovel_cases.npz, written by tests/golden/make_golden_egovel.py) unpacked once for
the host and the GPU tests."""
import os

import numpy as np

from conftest import GOLDEN

DEGENERATE = ("one_bearing", "range_zero")     # the frames the kernel must hand back (rank-deficient, a point at range 0)


class Cases:
    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "egovel_cases.npz"), allow_pickle=False)
        self.cap, self.thr, self.rel_tol = int(g["cap"]), float(g["thr"]), float(g["rel_tol"])
        self.names = [str(n) for n in g["case_names"]]
        self.counts = g["case_counts"]
        off = np.cumsum(self.counts) - self.counts
        self.points = [g["case_points"][o:o + c] for o, c in zip(off, self.counts)]
        self.fits = {d: dict(coef=g[f"case_coef_{d}"], r2=g[f"case_r2_{d}"], share=g[f"case_share_{d}"],
                             mask=[g[f"case_mask_{d}"][o:o + c] for o, c in zip(off, self.counts)]) for d in (2, 3)}
        self.seq_counts = g["seq_counts"]
        off = np.cumsum(self.seq_counts) - self.seq_counts
        self.seq = [g["seq_points"][o:o + c] for o, c in zip(off, self.seq_counts)]
        self.track = {k: g[f"seq_track_{k}"] for k in ("standard", "ods")}
        self.stats = {k: g[f"seq_stats_{k}"] for k in ("standard", "ods")}
        self.table_n = g["table_n"]
        self.table_subsets = g["table_subsets"]
        sizes = self.table_n + 1
        off = np.cumsum(sizes) - sizes
        self.table_trials = [g["table_trials"][o:o + s] for o, s in zip(off, sizes)]

    def tables_for(self, counts):
        """The table arguments of mmw_ego_velocity_ransac from the STORED draws (no scikit-learn)."""
        row = np.full(len(counts), -1, dtype=np.int32)
        for f, n in enumerate(counts):
            if n >= 10:
                row[f] = int(np.nonzero(self.table_n == n)[0][0])
        sizes = self.table_n + 1
        return (np.ascontiguousarray(self.table_subsets, dtype=np.int32), row,
                np.ascontiguousarray(np.concatenate(self.table_trials), dtype=np.int32),
                np.ascontiguousarray(np.cumsum(sizes) - sizes, dtype=np.int32))


_cases = None


def cases() -> Cases:
    global _cases
    if _cases is None:
        _cases = Cases()
    return _cases


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) if want.size else 0.0


class Geometry:
    """All an estimator reads of its config manager."""

    def __init__(self, array_geometry):
        self.array_geometry = array_geometry
