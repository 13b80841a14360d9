"""Crafted range profiles for the ground detector's peak picker (k_ground_peaks / pick_peaks, mmw_ground.h).

The reference is the host path the pipeline falls back to: ``RangeProcessor.find_peaks(20 * np.log10(p), bins, max_peaks)`` with
``bins = np.arange(S)``, so candidates are peak indices.  Profiles are built in linear units, p = 10 ** (y / 20), and every crafted
decision is then MEASURED on 20 * np.log10(p) (``Case.dist``, in dB): nothing here assumes that the distance asked for is the
distance made.  A decision comes in up to five variants:

  equal     bitwise equal p (where the decision compares two samples)
  near-/+   the measured distance within a quarter of PEAK_BAND_DB, on either side: the device must hand the row to the host
  far-/+    the measured distance eight bands away, on either side: the device must decide, and decide as scipy does

(1/4 band and 8 bands are the ratios tests/lsq_band_cases.py uses.)  tests/test_ground_pick_cases_host.py proves the builders
without a GPU; tests/test_gpu_ground_pick.py runs the rows through mmw_diag_ground_pick.
"""
from dataclasses import dataclass, field

import numpy as np

from mmwave_radar_processing_amd.processors.range_resp import RangeProcessor

BAND = 1e-9                     # PEAK_BAND_DB of mmw_ground.h
LOG10_BOUND = 1e-12             # |y_dev - y_host|, stated at the top of mmw_ground.h
PEAK_LIST = 512                 # peaks one workgroup keeps
NEAR, FAR = BAND / 8, 8 * BAND  # what the builders ask for; the host test checks what they got: <= BAND / 4, 7 .. 9 bands
VARIANTS = {"equal": 0.0, "near-": -NEAR, "near+": NEAR, "far-": -FAR, "far+": FAR}
S0 = 64


@dataclass
class Case:
    name: str                   # "<decision>/<variant>"
    p: np.ndarray               # linear profile, float64 [S]
    max_peaks: tuple = (2, 3)   # the max_peaks values the row is run with
    flagged: bool = False       # the device must answer -1 (near rows, ties among the peaks returned, more than PEAK_LIST peaks)
    dist: float = None          # measured distance of the crafted decision in dB (None: the row crafts no distance)
    nonfinite: bool = False     # NaN / Inf cells: flagged or decided as the reference, never decided differently
    changes: bool = True        # the two far sides of this decision give two different answers
    dists: np.ndarray = field(default=None, repr=False)   # every measured distance of a tiled row

    @property
    def decision(self):
        return self.name.split("/")[0]

    @property
    def variant(self):
        return self.name.split("/")[1] if "/" in self.name else "plain"

    @property
    def S(self):
        return len(self.p)


def to_db(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(p)


def to_lin(y):
    return 10.0 ** (np.asarray(y, dtype=np.float64) / 20.0)


def reference(y_db, max_peaks):
    """Peak indices, strongest first, as float64: what mmw_diag_ground_pick writes for bins = arange(S)."""
    y_db = np.asarray(y_db)
    with np.errstate(invalid="ignore"):
        return np.asarray(RangeProcessor.find_peaks(None, y_db, np.arange(len(y_db), dtype=np.float64), max_peaks)[0], dtype=np.float64)


def floor(S=S0, level=0.0):
    return np.full(S, float(level))


def _variants(decision, build, measure, equal=True, flag_equal=False, changes=True, max_peaks=(2, 3)):
    """build(delta_dB) -> y; measure(20 log10 p) -> the distance the decision sees."""
    out = []
    for v, delta in VARIANTS.items():
        if v == "equal" and not equal:
            continue
        p = to_lin(build(delta))
        out.append(Case(f"{decision}/{v}", p, max_peaks, flagged=v.startswith("near") or (v == "equal" and flag_equal),
                        dist=float(measure(to_db(p))), changes=changes))
    return out


def _peaks_row(levels, S=S0, first=8, step=8):
    """Isolated one-sample peaks of the given dB levels at first, first + step, ... on a 0 dB floor."""
    y = floor(S)
    for k, lv in enumerate(levels):
        y[first + k * step] = lv
    return y


# ------------------------------------------------------------------------------------------------ the decisions, S = 64
def neighbour_cases():
    def rise(d):            # d > 0: the peak is sample 20; d < 0: sample 19; equal: the plateau 19..20, midpoint 19
        y = floor()
        y[19], y[20] = 30.0, 30.0 + d
        return y

    def fall(d):            # the same pair with the crafted sample on the left: sample 20 compares against a peak at 19
        y = floor()
        y[19], y[20] = 30.0 + d, 30.0
        return y
    return (_variants("rise", rise, lambda yy: yy[20] - yy[19]) + _variants("fall", fall, lambda yy: yy[19] - yy[20]))


def plateau_cases():
    out = []
    for n in (2, 3, 4):     # midpoint (i + r - 1) / 2 = 20, 21, 21
        y = floor()
        y[20:20 + n] = 30.0
        out.append(Case(f"plateau{n}/equal", to_lin(y), dist=0.0))

    def tail(d):            # 20..22 equal, sample 23 off by d: below, the plateau 20..22 (peak 21); above, the peak is 23
        y = floor()
        y[20:23], y[23] = 30.0, 30.0 + d
        return y
    out += _variants("plateau_tail", tail, lambda yy: yy[23] - yy[22], equal=False)
    for name, sl in (("plateau_first", slice(0, 3)), ("plateau_last", slice(S0 - 3, S0))):
        y = floor()
        y[sl] = 30.0        # runs into sample 0 / S - 1: never a peak
        out.append(Case(name, to_lin(y)))
    y = floor()
    y[1], y[S0 - 2] = 30.0, 25.0
    out.append(Case("maxima_at_1_and_S-2", to_lin(y)))
    return out


def prominence_walk_cases():
    out = []

    def blocker(d):
        # P = 30 dB at 30 on a 27 dB shelf (22..29); beyond the shelf a sample B = 30 + d at 21, then the 0 dB floor.  B above P
        # stops P's walk on the shelf: prominence 3 dB, only B is a peak.  B below P does not stop it, and P stops B's: only P is
        # a peak.  B equal to P stops neither walk: two equal peaks, a tie, flagged.
        y = floor()
        y[22:30], y[30], y[21] = 27.0, 30.0, 30.0 + d
        return y
    out += _variants("walk_stop", blocker, lambda yy: yy[21] - yy[30], flag_equal=True)

    y = floor()             # two bitwise-equal minima left of the peak (10 and 15): the nearer is kept; one on the right
    y[30], y[10], y[15], y[40] = 30.0, -5.0, -5.0, -5.0
    out.append(Case("equal_minima/equal", to_lin(y), dist=0.0))

    def bases(d):           # left minimum 10 + d against right minimum 10: whichever is the base, the peak stands
        y = floor(level=20.0)
        y[30], y[25], y[35] = 40.0, 10.0 + d, 10.0
        return y
    out += _variants("lb_rb", bases, lambda yy: yy[25] - yy[35], changes=False)

    for name, left, right in (("higher_base_left", 26.0, 0.0), ("higher_base_right", 0.0, 26.0)):
        y = floor(level=28.0)   # the higher base is 4 dB down (no peak); the lower one would make it a peak
        y[30], y[25], y[35] = 30.0, left, right
        out.append(Case(name, to_lin(y)))
    return out


def threshold_cases():
    def prom(d):            # one peak of 6 + d dB over a 3 dB floor
        y = floor(level=3.0)
        y[30] = 9.0 + d
        return y

    def cut(d):             # the second peak against the strongest - 20 dB
        y = floor()
        y[20], y[40] = 40.0, 20.0 + d
        return y
    return (_variants("prominence_6dB", prom, lambda yy: (yy[30] - yy[29]) - 6.0, equal=False)
            + _variants("cut_20dB", cut, lambda yy: yy[40] - (yy[20] - 20.0), equal=False))


def ordering_cases():
    out = []
    for m in (2, 3):
        lead = [40.0, 38.0, 36.0][:m - 1]                 # m - 1 distinct peaks in front

        def last_in(d, lead=lead):                        # peak m - 1 against peak m (0-based): which one is returned
            return _peaks_row(lead + [33.0, 33.0 + d])
        k = 8 + 8 * (m - 1)
        out += _variants(f"order_last_in_m{m}", last_in, lambda yy, k=k: yy[k + 8] - yy[k], flag_equal=True, max_peaks=(m,))

        def top(d, m=m):                                  # peak 0 against peak 1
            return _peaks_row([40.0, 40.0 + d, 30.0, 29.0][:m + 1])
        out += _variants(f"order_top_m{m}", top, lambda yy: yy[16] - yy[8], flag_equal=True, max_peaks=(m,))
        # peaks m and m + 1 bitwise equal: not among those returned, NOT flagged
        out.append(Case(f"order_tie_behind_m{m}/equal", to_lin(_peaks_row([40.0, 38.0, 36.0][:m] + [33.0, 33.0])), (m,), dist=0.0))
    return out


def no_peak_cases():
    return [Case("constant", to_lin(floor(level=7.0))),
            Case("monotone", to_lin(np.linspace(0.0, 40.0, S0))),
            Case("three_without", to_lin([0.0, 10.0, 20.0])),
            Case("three_with", to_lin([0.0, 30.0, 0.0]))]


def zero_cases():
    y = floor()
    y[30] = 30.0
    p = to_lin(y)
    p[25:30] = 0.0          # -inf dB on both sides of the peak: the prominence is +inf
    p[31:36] = 0.0
    q = p.copy()
    q[31:36] = 1.0          # zeros on one side only: the base is the 0 dB floor
    return [Case("zeros_both_bases", p), Case("zeros_left_base", q), Case("all_zero", np.zeros(S0))]


def nonfinite_cases():
    base = _peaks_row([40.0, 35.0, 30.0])
    out = []
    for name, idx, val in (("nan_on_floor", 50, np.nan), ("nan_beside_peak", 9, np.nan), ("nan_peak", 16, np.nan),
                           ("inf_peak", 40, np.inf), ("inf_beside_peak", 17, np.inf), ("minus_inf", 50, -np.inf),
                           ("nan_first", 0, np.nan), ("nan_last", S0 - 1, np.nan)):
        p = to_lin(base)
        p[idx] = val
        out.append(Case(name, p, nonfinite=True))
    return out


def s64_cases():
    return (neighbour_cases() + plateau_cases() + prominence_walk_cases() + threshold_cases() + ordering_cases()
            + [c for c in no_peak_cases() if c.S == S0] + zero_cases() + nonfinite_cases() + [generic(S0)])


# ------------------------------------------------------------------------------------------------ other row lengths
def generic(S, seed=1):
    """A noisy floor (0 .. 5 dB: hundreds of local maxima short of 6 dB prominence) with peaks of 40, 37, 33 and 15 dB (the last
    under the cut), the first at sample 1 and the second at S - 2 when the row has room."""
    rng = np.random.default_rng(1000 * seed + S)
    y = rng.uniform(0.0, 5.0, S)
    if S >= 16:
        for idx, lv in zip((1, S - 2, S // 2, S // 3), (40.0, 37.0, 33.0, 15.0)):
            y[idx] = lv
    else:
        y[S // 2] = 30.0
    return Case(f"generic_S{S}" + (f"_seed{seed}" if seed != 1 else ""), to_lin(y))


def sawtooth(n_peaks):
    """n_peaks one-sample peaks of 30 .. 35.12 dB, all different and in shuffled order, over 0 dB valleys: S = 2 n_peaks + 1, the
    smallest row that holds them.  512 peaks are decided; 513 are more than the workgroup keeps: flagged."""
    S = 2 * n_peaks + 1
    y = floor(S)
    y[1::2] = 30.0 + 0.01 * np.random.default_rng(n_peaks).permutation(n_peaks)
    return Case(f"sawtooth_{n_peaks}", to_lin(y), flagged=n_peaks > PEAK_LIST)


def tiled(variant, S=3072):
    """The S = 64 rise/<variant> row 48 times, tile t raised by 0.1 t dB so that the 48 peaks differ: the crafted pair of every tile
    keeps its distance (measured per tile in ``dists``)."""
    y64 = floor()
    y64[19], y64[20] = 30.0, 30.0 + VARIANTS[variant]
    n = S // S0
    y = np.concatenate([y64 + 0.1 * t for t in range(n)])
    yy = to_db(to_lin(y))
    d = yy[20::S0] - yy[19::S0]
    return Case(f"tiled_rise_S{S}/{variant}", to_lin(y), dist=float(d[np.argmin(np.abs(d))]), dists=d)


def cases_by_length():
    """{S: [Case, ...]}: every row of one length goes to the device in one launch."""
    out = {S0: s64_cases(), 3: [c for c in no_peak_cases() if c.S == 3] + [generic(3)]}
    for S in (255, 256, 257):
        out[S] = [generic(S), generic(S, seed=2)]
    out[2 * PEAK_LIST + 1] = [sawtooth(PEAK_LIST), generic(2 * PEAK_LIST + 1)]
    out[2 * PEAK_LIST + 3] = [sawtooth(PEAK_LIST + 1), generic(2 * PEAK_LIST + 3)]
    out[3072] = [tiled("far-"), tiled("far+"), generic(3072)]
    return out


def all_cases():
    return [c for rows in cases_by_length().values() for c in rows]


def perturbed(p, seed):
    """20 log10(p) moved by +-LOG10_BOUND dB, the same way for equal p (log10 is a function on either side)."""
    yy = to_db(p)
    uniq, inv = np.unique(p, return_inverse=True)
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], len(uniq)) if seed >= 0 else np.where(np.arange(len(uniq)) % 2, 1.0, -1.0)
    with np.errstate(invalid="ignore"):
        return yy + sign[inv] * LOG10_BOUND
