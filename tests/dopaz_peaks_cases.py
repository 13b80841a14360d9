"""Crafted Doppler-azimuth maps for the peak pickers, shared by tests/test_doppler_azimuth_peaks_host.py and
tests/test_gpu_doppler_azimuth_peaks.py (not a test module): seeded random maps with plateaus, ties, zero rows, short frames and
narrow column intervals; maps whose comparisons sit at a chosen multiple of MMW_DOPAZ_PEAK_BAND; and the host pickers of
DopplerAzimuthProcessor turned into the index tables the C entries write."""
import copy
import json
import os

import numpy as np

from conftest import GOLDEN
from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.config_managers import ConfigManager
from mmwave_radar_processing_amd.processors import DopplerAzimuthProcessor

TAU = _lib.DOPAZ_PEAK_BAND
NONE, UNDECIDED = _lib.DOPAZ_PEAK_NONE, _lib.DOPAZ_PEAK_UNDECIDED
A = 64


def make_proc(name="6843_RadVel_ods_20Hz.cfg", **kw):
    with open(os.path.join(GOLDEN, "cfg_scalars.json")) as fh:
        ent = json.load(fh)[name]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(ent["lines"]) + "\n")
    return DopplerAzimuthProcessor(cm, **kw)


class Case:
    """One call of the entries: maps float32 [n_sets][F][n_rows][64], groups int32 [G][2], m int32 [F] or None."""

    def __init__(self, maps, groups, m, a_lo, a_hi, a_zero, thr, label=""):
        self.maps = np.ascontiguousarray(maps, dtype=np.float32)
        self.groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1, 2)
        self.m = None if m is None else np.ascontiguousarray(m, dtype=np.int32)
        self.a_lo, self.a_hi, self.a_zero, self.thr, self.label = int(a_lo), int(a_hi), int(a_zero), float(thr), label
        self.n_sets, self.F, self.n_rows = self.maps.shape[:3]
        self.G = len(self.groups)

    def rows_of(self, f):
        return self.n_rows if self.m is None else int(self.m[f])

    def group_map(self, g, f):
        """float64 [m_f, n_valid]: what the host pickers are given (the reference's (resp_1 + resp_2) / 2 on float64 maps)."""
        s1, s2 = self.groups[g]
        x = self.maps[s1, f].astype(np.float64)
        if s2 >= 0:
            x = (x + self.maps[s2, f].astype(np.float64)) / 2
        return x[:self.rows_of(f), self.a_lo:self.a_hi]


def ip(a):
    return None if a is None else a.ctypes.data_as(_lib._ip)


def run_host_entry(case, prominence_dB=4.0):
    lib = _lib.load_library()
    row = np.full((case.G, case.F, case.n_rows), -7, dtype=np.int32)
    zero = np.full((case.G, case.F), -7, dtype=np.int32)
    rc = lib.mmw_diag_doppler_azimuth_peaks_host(case.maps.ctypes.data, case.n_sets, case.F, case.n_rows, A, ip(case.groups), case.G,
                                                 ip(case.m), case.a_lo, case.a_hi, case.a_zero, case.thr, prominence_dB,
                                                 row.ctypes.data, zero.ctypes.data)
    assert rc == _lib.MMW_OK, lib.mmw_last_error()
    return row, zero


def host_pickers(proc, case, g, f):
    """(row entries [n_rows], zero entry) of one (group, frame) from detect_peaks_rows / detect_peak_zero_az."""
    nc, m = case.a_hi - case.a_lo, case.rows_of(f)
    row = np.full(case.n_rows, NONE, dtype=np.int32)
    if m == 0:
        return row, NONE               # np.max of an empty map raises on the host; the entries define "no peak"
    p = copy.copy(proc)
    p.valid_angle_bins = (np.arange(nc) - (case.a_zero - case.a_lo)) * 0.01         # |.| smallest at the zero column
    resp = case.group_map(g, f)
    vel = np.arange(m, dtype=np.float64)
    with np.errstate(all="ignore"):
        peaks = p.detect_peaks_rows(resp.copy(), vel, case.thr)
        z = p.detect_peak_zero_az(resp.copy(), vel, case.thr)
    for ang, v in peaks:
        row[int(v)] = int(round(ang / 0.01)) + (case.a_zero - case.a_lo)
    return row, (int(z[1]) if z.shape[0] > 0 else NONE)


def host_tables(proc, case):
    row = np.empty((case.G, case.F, case.n_rows), dtype=np.int32)
    zero = np.empty((case.G, case.F), dtype=np.int32)
    for g in range(case.G):
        for f in range(case.F):
            row[g, f], zero[g, f] = host_pickers(proc, case, g, f)
    return row, zero


def random_case(seed, n_rows, F=3, thr=30.0, width=None, quantised=True):
    """Four sets, groups (0, 1), (2,), (3, 2).  Quantised: multiples of 1/4 on a bump, so plateaus and ties abound and every
    difference is a multiple of 1/8 -- nothing comes near the band.  Frame 1 is cut short (m < n_rows) with data behind m; one
    row per frame is zero; one set of the last frame is all zero."""
    rng = np.random.default_rng(seed)
    width = int(rng.integers(3, A + 1)) if width is None else width
    a_lo = int(rng.integers(0, A - width + 1))
    a_hi = a_lo + width
    a_zero = int(rng.integers(a_lo, a_hi))
    cols = np.arange(A)
    bump = 6.0 * np.exp(-0.5 * ((cols - rng.integers(a_lo, a_hi)) / max(2.0, width / 5)) ** 2)
    maps = rng.random((4, F, n_rows, A)) * 6.0 + bump * rng.random((4, F, n_rows, 1))
    maps[rng.random(maps.shape) < 0.1] *= 4.0
    if quantised:
        maps = np.round(maps * 4) / 4
    for f in range(F):
        maps[:, f, int(rng.integers(0, n_rows))] = 0.0
    maps[3, F - 1] = 0.0
    m = np.full(F, n_rows, dtype=np.int32)
    if F > 1:
        m[1] = max(1, n_rows - max(1, n_rows // 3)) if n_rows > 1 else 0
        maps[:, 1, m[1]:] += 50.0         # larger than anything inside: must raise neither the floor nor a peak at row m - 1
    return Case(maps, [[0, 1], [2, -1], [3, 2]], m, a_lo, a_hi, a_zero, thr, f"seed {seed} rows {n_rows} width {width} thr {thr}")


def random_cases(n_rows_list=(1, 2, 33, 70)):
    cases, seed = [], 100
    for n_rows in n_rows_list:
        for thr in (30.0, 10.0, 3.0):
            for width in (None, None, 1, 2, 3, 64):
                for quantised in ((True, False) if width is None else (True,)):
                    cases.append(random_case(seed, n_rows, thr=thr, width=width, quantised=quantised))
                    seed += 1
    return cases


def pair_for(y):
    """float32 (m1, m2) whose average, widened as the entries do, gives |avg| + 1e-12 as close to y as float32 allows: the
    second map supplies the fine offset."""
    t = y - 1e-12
    m1 = np.float32(2 * t)
    m2 = np.float32(2 * t - float(m1))
    return m1, m2


def y_of(m1, m2):
    return abs((float(m1) + float(m2)) / 2) + 1e-12


def band_case(scale):
    """One pair-averaged group, 5 rows, columns [7, 12), zero column 9; frame by frame one comparison of each kind placed at
    ``scale * MMW_DOPAZ_PEAK_BAND`` relative distance, above and below.  Returns (case, notes) with notes[f] =
    (kind, rows whose entry hangs on the comparison, whether the zero entry does)."""
    d0 = scale * TAU
    lo, nc, zc = 7, 5, 2
    frames, notes = [], []

    def blank():
        return np.zeros((2, 5, A), dtype=np.float32)

    def put(x, r, c, y):
        x[0, r, lo + c], x[1, r, lo + c] = pair_for(y)
        got = y_of(x[0, r, lo + c], x[1, r, lo + c])
        assert abs(got - y) <= 1e-14 * y, (got, y)
        return got

    for sign in (+1.0, -1.0):
        d = sign * d0
        # neighbour against neighbour: a plateau of two, or a strict step
        x = blank()
        put(x, 1, 0, 1.0), put(x, 1, 1, 4.0), put(x, 1, 2, 4.0 * (1 + d)), put(x, 1, 3, 1.0)
        frames.append(x), notes.append(("neighbour", [1], False))
        # the floor test, 20 dB below a maximum of 8: the cell is a peak of the zero column when it stays above the floor
        x = blank()
        ymax = put(x, 4, 0, 8.0)
        put(x, 1, zc, ymax * 10 ** (-20.0 / 20) * (1 + d))
        frames.append(x), notes.append(("floor", [1], True))
        # peak against base * 10^(4 / 20): walls of 9 on the first and last column, a base of 2
        x = blank()
        put(x, 2, 0, 9.0), put(x, 2, 1, 2.0), put(x, 2, 3, 2.0), put(x, 2, 4, 9.0)
        base = y_of(x[0, 2, lo + 1], x[1, 2, lo + 1])
        put(x, 2, 2, base * 10 ** (4.0 / 20) * (1 + d))
        frames.append(x), notes.append(("prominence", [2], False))
        # candidate against candidate, down the zero column (no prominence walk there)
        x = blank()
        put(x, 1, zc, 4.0), put(x, 3, zc, 4.0 * (1 + d))
        frames.append(x), notes.append(("candidate", [], True))
    return np.stack(frames, axis=1), notes              # [2][F][5][64]


def band_cases(scale):
    """The frames of ``band_case`` as calls of one floor each (the floor frames need 20 dB, the others run at 30 dB)."""
    maps, notes = band_case(scale)
    out = []
    for thr in (20.0, 30.0):
        keep = [f for f, n in enumerate(notes) if (n[0] == "floor") == (thr == 20.0)]
        out.append((Case(maps[:, keep], [[0, 1]], None, 7, 12, 9, thr, f"band x{scale} thr {thr}"), [notes[f] for f in keep]))
    return out


def nonfinite_case():
    """Frame 0: a NaN in set 0; frame 1: an Inf in set 1, inside its m rows; frame 2: NaN only behind its m rows and Inf only
    outside the valid columns -- that frame is decided."""
    case = random_case(7, 9, F=3, width=20)
    maps = case.maps.copy()
    maps[0, 0, 3, case.a_lo + 1] = np.nan
    maps[1, 1, 0, case.a_hi - 1] = np.inf
    m = np.array([9, 6, 5], dtype=np.int32)
    maps[:, 2, 5:] = np.nan
    if case.a_lo > 0:
        maps[:, 2, :, case.a_lo - 1] = np.inf
    if case.a_hi < A:
        maps[:, 2, :, case.a_hi] = np.inf
    return Case(maps, [[0, 1], [2, -1], [1, -1]], m, case.a_lo, case.a_hi, case.a_zero, 30.0, "non-finite")
