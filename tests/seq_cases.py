"""Inputs and NumPy references for the sequential detector's edge tests (test_seq_cases_host.py, test_gpu_seq_edges.py).

Three kernels are driven straight through the C ABI:

  mmw_seq_rows          range CFAR on a caller's float64 profiles -> ascending row lists      (profile_frames, rows_cases)
  mmw_seq_detect        the row kernel on a caller's row lists                               (cube_batch, shape_lists, ...)
  mmw_seq_detect_plane  the full-plane route on the same lists (k_cfar1d_gated's list search)
  mmw_cfar1d_rows       the list search alone on a caller's float64 planes                   (plane_lists)

The CFAR reference is cfar_cases.ref_cfar1d (held bit-exact against k_cfar1d by test_gpu_cfar_edges.py); the value reference is
oracle_np.range_doppler in complex128.
"""
import math
import warnings

import numpy as np

import cfar_cases as cc
from oracle import oracle_np as O

ROW_POISON, DET_POISON = -99, -7777                # int32 words the outputs hold before a call
MAG_POISON = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]      # a NaN no kernel produces
GUARD_WORDS = 64
SEQ_RPT = 4                                        # csrc/mmw_seq.h
SEQ_LDS_MAX = 160 * 1024
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------------------------------------- mirrors
def pass_rows(C):
    """seq_pass_rows of csrc/mmw_seq.h: selected rows one pass of k_seq_detect takes."""
    return SEQ_RPT * (256 // min(C, 256))


def lds_bytes(S, C):
    """seq_lds_bytes: both twiddle tables, then per pass range bins (16 B), magnitudes (8 B) and flags (1 B) per cell."""
    return 16 * (S + C) + pass_rows(C) * C * 25


def ref1d(x, kind, T, G, scale, k=0):
    """cfar_cases.ref_cfar1d; with no training cells (T = 0) the mean of nothing is NaN, and NumPy warns of it."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return cc.ref_cfar1d(x, kind, T, G, scale, k)


# ----------------------------------------------------------------------------------------------------------- mmw_seq_rows
ROWS_S = (1, 5, 255, 256, 257, 1301, 3072)
ROWS_SCALES = (1.0, cc.JUST_BELOW_ONE)


def rows_windows(S):
    """(T, G): the three windows of the issue, one without training cells, one longer than the row."""
    return [(1, 0), (4, 2), (8, 2), (0, 2), (4, S)]


def rows_kinds(T):
    """(kind, k_rank): OS at its lowest, a middle and its highest rank; no OS without training cells (the entry refuses it)."""
    out = [(cc.CA, 0), (cc.GO, 0), (cc.SO, 0)]
    if T > 0:
        out += [(cc.OS, k) for k in sorted({1, T, 2 * T})]
    return out


def profile_frames(S, T, G):
    """Four profiles of one mmw_seq_rows call: quantised; constant (every valid cell on its threshold: no hits at scale 1);
    a ramp (on its CA threshold everywhere) with a spike in the first and in the last valid cell; non-finite."""
    half = T + G
    q = cc.quantised(S, 6, 100 + S + T)
    edge = cc.ramp(S) + 1.0
    if S >= 2 * half + 1:
        edge[half] = edge[S - half - 1] = 1e6
    try:
        nf = cc.nonfinite(S, 200 + S + T, half)[0]
    except ValueError:                               # no room for the plants: a NaN and an infinity where they fit
        nf = np.random.default_rng(200 + S + T).exponential(1.0, S) * 1e3
        nf[S // 2] = np.nan
        if S > 1:
            nf[0] = np.inf
    return np.stack([q, cc.constant(S), edge, nf])


def rows_reference(prof, kind, T, G, scale, k):
    """(thresholds [F][S], masks [F][S]) of the profiles."""
    out = [ref1d(p, kind, T, G, scale, k) for p in prof]
    return np.stack([o[0] for o in out]), np.stack([o[2] for o in out])


def rows_cases(S):
    """Every (T, G, kind, k_rank, scale) of one S."""
    return [(T, G, kind, k, scale) for T, G in rows_windows(S) for kind, k in rows_kinds(T) for scale in ROWS_SCALES]


def rows_case_is_empty(S, T, G, kind):
    """Deliberately empty: no valid cell (the window is longer than the row) or no training cells (the threshold is NaN)."""
    return S < 2 * (T + G) + 1 or T == 0


# ----------------------------------------------------------------------------------------------------------- cubes and lists
SHAPES = ((3, 32, 128), (2, 24, 100), (2, 20, 50), (1, 16, 127), (2, 12, 3), (1, 9, 1), (2, 1, 8), (1, 8, 257), (1, 8, 300),
          (1, 300, 16), (1, 1024, 512))
BIG_SHAPE = (1, 1024, 512)                         # more than 64 KiB of LDS; at most MAX_BIG_ROWS rows per list
MAX_BIG_ROWS = 8
ROUTE_SHAPES = ((3, 32, 128), (2, 24, 100), (1, 8, 300))       # C divides 256, does not, exceeds it
UNSERVED = (3000, 1024)                            # S, C: 166 784 B of LDS
N_FRAMES = 6
DET_WINDOWS = ((1, 0), (4, 2))
DET_SCALE = 2.0
ROW_KERNEL, FULL_PLANE = 0, 1                      # the two routes: mmw_seq_detect, mmw_seq_detect_plane


def det_kinds(T):
    return [(cc.CA, 0), (cc.OS, T), (cc.GO, 0), (cc.SO, 0)]


def tones(shape, f):
    """(range row, Doppler frequency, amplitude) of frame f: rows 1, S / 2 and S - 2, so that the list of odd rows, the list of
    the first rows and the single-row lists each hold some tone rows and miss others."""
    _, S, C = shape
    rows = (1 % S, S // 2, (S - 2) % S)
    bins = ((5 + f) % C, (C // 2 + 3) % C, (C - 7 - f) % C)
    amps = (40.0 + f, 25.0, 15.0 + 2 * f)
    return list(zip(rows, bins, amps))


_CUBES = {}


def cube_batch(shape, n_frames=N_FRAMES, seed=0):
    """[F][V][S][C] complex64 with integer-valued parts: three tones of distinct amplitudes per frame, Gaussian noise of sigma 3
    in every antenna, another phase and other noise in every antenna.  Cached; callers copy before they write."""
    key = (shape, n_frames, seed)
    if key not in _CUBES:
        V, S, C = shape
        rng = np.random.default_rng(1000 * S + C + seed)
        s, c = np.arange(S)[:, None], np.arange(C)[None, :]
        out = np.empty((n_frames,) + tuple(shape), np.complex64)
        for f in range(n_frames):
            x = rng.normal(0.0, 3.0, shape) + 1j * rng.normal(0.0, 3.0, shape)
            for t, (r, k, amp) in enumerate(tones(shape, f)):
                wave = amp * np.exp(2j * np.pi * (r * s / S + k * c / C))
                for v in range(V):
                    x[v] += wave * np.exp(0.7j * v * (t + 1))
            out[f] = np.round(x.real) + 1j * np.round(x.imag)
        out.setflags(write=False)
        _CUBES[key] = out
    return _CUBES[key]


def shape_lists(shape):
    """The six lists of the first call: empty, [0], [S - 1], every row, every other row from 1, the first min(RB + 1, S) rows.
    BIG_SHAPE keeps every list at MAX_BIG_ROWS rows or fewer (spread rows for 'every row')."""
    _, S, C = shape
    every, odd = np.arange(S), np.arange(1, S, 2)
    if shape == BIG_SHAPE:
        every = np.unique(np.linspace(0, S - 1, MAX_BIG_ROWS).round().astype(int))
        odd = odd[:: max(1, len(odd) // MAX_BIG_ROWS)][:MAX_BIG_ROWS]
    return [np.zeros(0, int), np.array([0]), np.array([S - 1]), every, odd, np.arange(min(pass_rows(C) + 1, S))]


def pass_lists(shape):
    """The lists of the second call: RB - 1, RB and 2 RB rows drawn from all S (those lengths that S and BIG_SHAPE's limit allow)."""
    _, S, C = shape
    rb = pass_rows(C)
    limit = MAX_BIG_ROWS if shape == BIG_SHAPE else S
    rng = np.random.default_rng(S + C)
    return [np.sort(rng.choice(S, n, replace=False)) for n in (rb - 1, rb, 2 * rb) if 0 < n <= limit]


def pack_lists(lists, S, n_frames=None):
    """(rows [F][S] int32, poisoned behind each list; nrows [F] int32)."""
    F = len(lists) if n_frames is None else n_frames
    rows = np.full((F, S), ROW_POISON, np.int32)
    nrows = np.zeros(F, np.int32)
    for f, lst in enumerate(lists):
        rows[f, :len(lst)] = lst
        nrows[f] = len(lst)
    return rows, nrows


def close_cells(x, thr):
    """Valid cells (finite threshold) within 4 ulp of their threshold: there np.mean and another summation order may decide
    differently."""
    with np.errstate(invalid="ignore"):
        near = np.isfinite(thr) & (np.abs(x - thr) <= 4.0 * np.spacing(np.abs(thr)))
    return int(near.sum())


def expected_dets(rows, mags, kind, T, G, scale, k=0):
    """The (row, d) pairs, rows in list order and d ascending, of ref_cfar1d on the float64 rows mags[j] of range bin rows[j];
    and the number of cells too close to their threshold to call."""
    pairs, close = [], 0
    for r, x in zip(rows, mags):
        thr, _, mask = ref1d(x, kind, T, G, scale, k)
        close += close_cells(x, thr)
        pairs += [(int(r), int(d)) for d in np.flatnonzero(mask)]
    return np.array(pairs, np.int32).reshape(-1, 2), close


def oracle_plane(cube):
    """|range-Doppler| of antenna 0 in float64 from the complex128 oracle."""
    return np.abs(O.range_doppler(cube[:1].astype(np.complex128))[0])


def value_bound(cube):
    """Bound on |device row - oracle row| of one frame [V][S][C].  A device value is a direct sum of S terms, then of C terms, in
    float64 with tables rounded to 1 ulp, so its error is at most (S + C + 16) 2^-52 L1 with
    L1 = sum_s sum_c hann(S)[s] hann(C)[c] (|re| + |im|) of antenna 0; the oracle's own FFTs add 2 log2(S C) 2^-52 L1."""
    _, S, C = cube.shape
    x = cube[0].astype(np.complex128)
    l1 = float(np.sum(np.hanning(S)[:, None] * np.hanning(C)[None, :] * (np.abs(x.real) + np.abs(x.imag))))
    return (S + C + 16 + 2.0 * math.log2(S * C)) * EPS * l1


def margin_violations(cube, rows, kind, T, G, scale, k):
    """Valid cells of the listed oracle rows that lie within 10 x value_bound x (1 + scale) of their threshold: where a device
    row within the bound of the oracle's could decide otherwise."""
    plane, need = oracle_plane(cube), 10.0 * value_bound(cube) * (1.0 + scale)
    bad = 0
    for r in rows:
        thr = ref1d(plane[r], kind, T, G, scale, k)[0]
        valid = np.isfinite(thr)
        bad += int(np.sum(np.abs(plane[r][valid] - thr[valid]) <= need))
    return bad


# ----------------------------------------------------------------------------------------------------------- mmw_cfar1d_rows
PLANE_SHAPES = ((45, 70), (7, 300), (32, 72))       # R * D = 3150 and 2100 (no multiple of 256), 2304 = 9 * 256
PLANE_WINDOW = (3, 1)                              # (T, G); k_rank 4 for OS; scale 1.0, so ties decide


def plane_lists(R):
    """empty, [0], [R - 1], all rows, alternating rows, two rows (the shortest list the binary search has to split)."""
    return [np.zeros(0, int), np.array([0]), np.array([R - 1]), np.arange(R), np.arange(0, R, 2), np.array([R // 3, R - 2])]


def planes_for_lists(shape):
    """name -> [6][R][D] float64, one plane per list: quantised, constant, non-finite."""
    R, D = shape
    half = sum(PLANE_WINDOW)
    return {"quantised": np.stack([cc.quantised(shape, 6, 60 + f + R) for f in range(6)]),
            "constant": np.stack([cc.constant(shape)] * 6),
            "nonfinite": np.stack([cc.nonfinite(shape, 70 + f + R, (0, half))[0] for f in range(6)])}


def plane_reference(planes, lists, kind, scale=1.0):
    """mask [F][R][D]: ref_cfar1d on the listed rows, 0 elsewhere."""
    T, G = PLANE_WINDOW
    mask = np.zeros(planes.shape, np.uint8)
    for f, lst in enumerate(lists):
        for r in lst:
            mask[f, r] = ref1d(planes[f, r], kind, T, G, scale, 4 if kind == cc.OS else 0)[2]
    return mask
