"""Inputs and NumPy references for the CFAR edge tests (test_cfar_cases_host.py, test_gpu_cfar_edges.py).

The builders make float64 inputs on which a cell can EQUAL its threshold (quantised, constant), on which every
comparison of a sort has a strict answer (ramp), and which hold every kind of float64 a kernel can mishandle
(nonfinite).  The references take `scale` and `k_rank` directly, as the C ABI does, and are written with the very
NumPy expressions of oracle/oracle_np.py (test_cfar_cases_host.py asserts that they agree with it).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

CA, OS, GO, SO = 0, 1, 2, 3                      # MMW_CFAR_* of include/mmwgpu.h
KIND_NAMES = {CA: "ca", OS: "os", GO: "go", SO: "so"}
NEG_NAN = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]      # the NaN x86 arithmetic produces
JUST_BELOW_ONE = float(np.nextafter(1.0, 0.0))


# ----------------------------------------------------------------------------------------------------------- inputs
def _shape2(shape):
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    return shape, ((1,) + shape if len(shape) == 1 else shape)


def quantised(shape, levels, seed):
    """Integer-valued cells in 0..levels-1, a few dozen of them times 4.  With scale 1.0 or 2.0 every product of the OS
    detectors is exact, so X == T really occurs, and so do equal cells."""
    shape, _ = _shape2(shape)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, levels, shape).astype(np.float64)
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, min(40, max(1, flat.size // 20)), replace=False)] *= 4.0
    return x


def constant(shape, value=3.0):
    """Every cell `value`.  N * 3.0 and the division by N are exact, so with scale 1.0 every valid cell sits on its
    threshold for all four kinds, and with JUST_BELOW_ONE every valid cell fires."""
    shape, _ = _shape2(shape)
    return np.full(shape, float(value))


def ramp(shape):
    """r * D + c: all cells distinct, monotone along both axes (negate it for the other sort direction)."""
    shape, s2 = _shape2(shape)
    return np.arange(s2[0] * s2[1], dtype=np.float64).reshape(shape)


PLANT_KINDS = ("pos_inf", "zeros", "negatives", "subnormal", "huge", "neg_inf", "nan", "neg_nan")


def nonfinite(shape, seed, half=(0, 0)):
    """An exponential background times 1e3 with one plant of every PLANT_KINDS entry.  Returns (x, plants); plants maps
    the kind to the index tuple of its first cell.  The plants lie inside the valid region of a window of half-size
    `half` (an int for rows) on a grid that spreads them as far apart as that region allows -- one window and more for
    the small windows, less where the valid region is only a few cells wide."""
    shape, s2 = _shape2(shape)
    half = (0, int(half)) if np.isscalar(half) else tuple(half)
    rng = np.random.default_rng(seed)
    x = rng.exponential(1.0, s2) * 1e3
    R, D = s2
    r_lo, r_hi, c_lo, c_hi = half[0], R - half[0], half[1], D - half[1] - 2       # plants are up to 3 cells wide
    if r_hi <= r_lo or c_hi <= c_lo:
        raise ValueError("no valid region to plant in")
    n = len(PLANT_KINDS)
    n_rows = min(r_hi - r_lo, 3 if R > 1 else 1)
    n_cols = -(-n // n_rows)
    rows = np.linspace(r_lo, r_hi - 1, n_rows).round().astype(int)
    cols = np.linspace(c_lo, c_hi - 1, n_cols).round().astype(int)
    plants = {}
    for i, kind in enumerate(PLANT_KINDS):
        r, c = int(rows[i // n_cols]), int(cols[i % n_cols])
        plants[kind] = (r, c) if len(shape) == 2 else (c,)
        if kind == "pos_inf":
            x[r, c] = np.inf
        elif kind == "neg_inf":
            x[r, c] = -np.inf
        elif kind == "nan":
            x[r, c] = np.nan
        elif kind == "neg_nan":
            x[r, c] = NEG_NAN
        elif kind == "zeros":
            x[r, c], x[r, c + 1] = -0.0, 0.0
        elif kind == "negatives":
            x[r, c:c + 3] = (-1.5, -2e3, -7.0)
        elif kind == "subnormal":
            x[r, c] = 5e-324
        elif kind == "huge":
            x[r, c:c + 3] = 1e308                  # their sum, and 2.0 * x, overflow
    return x.reshape(shape), plants


# ----------------------------------------------------------------------------------------------------------- references
def mask_2d(train, guard):
    tr, td = train
    gr, gd = guard
    wr, wd = 2 * (tr + gr) + 1, 2 * (td + gd) + 1
    mask = np.ones((wr, wd), dtype=bool)
    mask[tr:tr + 2 * gr + 1, td:td + 2 * gd + 1] = False
    return mask, wr, wd


def n_train_2d(train, guard):
    return int(mask_2d(train, guard)[0].sum())


def _finish_2d(X, est, scale, train, guard):
    thr = np.full(X.shape, np.inf)
    noise = np.zeros(X.shape)
    r0, d0 = train[0] + guard[0], train[1] + guard[1]
    with np.errstate(all="ignore"):
        thr[r0:r0 + est.shape[0], d0:d0 + est.shape[1]] = scale * est
    noise[r0:r0 + est.shape[0], d0:d0 + est.shape[1]] = est
    with np.errstate(invalid="ignore"):
        det = X > thr                                # strict
    return thr, noise, det.astype(np.uint8)


def ref_cfar2d(X, kind, train, guard, scale, k_rank=0):
    """(thresholds, noise, mask uint8) of one plane, oracle_np.ca_cfar_2d / os_cfar_2d with scale and k_rank given."""
    X = np.asarray(X, dtype=np.float64)
    mask, wr, wd = mask_2d(train, guard)
    if X.shape[0] < wr or X.shape[1] < wd:
        return np.full(X.shape, np.inf), np.zeros(X.shape), np.zeros(X.shape, np.uint8)
    win = sliding_window_view(X, (wr, wd))
    with np.errstate(all="ignore"):
        if kind == CA:
            n = int(mask.sum())
            est = np.sum(win * mask, axis=(2, 3)) / n
        elif kind == OS:
            cells = win[..., mask]
            est = np.partition(cells, k_rank - 1, axis=-1)[..., k_rank - 1]
        else:
            raise ValueError("2-D CFAR kind must be CA or OS")
    return _finish_2d(X, est, scale, train, guard)


def side_means_1d(x, T, G):
    win = sliding_window_view(np.asarray(x, dtype=np.float64), 2 * (T + G) + 1)
    with np.errstate(all="ignore"):
        return np.mean(win[:, :T], axis=1), np.mean(win[:, T + 2 * G + 1:], axis=1)


def ref_cfar1d(x, kind, T, G, scale, k_rank=0):
    """(thresholds, noise, mask uint8) of one row, the four 1-D functions of oracle_np with scale and k_rank given."""
    x = np.asarray(x, dtype=np.float64)
    L, w, half = len(x), 2 * (T + G) + 1, T + G
    thr, noise = np.full(L, np.inf), np.zeros(L)
    if L >= w:
        win = sliding_window_view(x, w)
        with np.errstate(all="ignore"):
            if kind == CA:
                m = np.ones(w, dtype=bool)
                m[T:T + 2 * G + 1] = False
                est = np.mean(win[:, m], axis=1)
            elif kind == OS:
                cells = np.concatenate((win[:, :T], win[:, T + 2 * G + 1:]), axis=1)
                est = np.partition(cells, k_rank - 1, axis=1)[:, k_rank - 1]
            else:
                l, r = side_means_1d(x, T, G)
                est = np.maximum(l, r) if kind == GO else np.minimum(l, r)
            thr[half:half + len(est)] = scale * est
        noise[half:half + len(est)] = est
    with np.errstate(invalid="ignore"):
        det = x > thr                                # strict
    return thr, noise, det.astype(np.uint8)


def tie_stats(X, thr, mask):
    """(cells with X == T, detections, cells that miss only because the rule is strict) over the finite thresholds."""
    valid = np.isfinite(thr)
    ties = int(np.sum(valid & (X == thr)))
    with np.errstate(invalid="ignore"):
        lost = int(np.sum(valid & (X >= thr) & (mask == 0)))
    return ties, int(mask.sum()), lost


# ----------------------------------------------------------------------------------------------------------- cases
PLANE_A, PLANE_B = (45, 70), (70, 45)
OS_WINDOWS = [((5, 5), (3, 2)), ((4, 4), (2, 2)), ((2, 2), (1, 1)), ((1, 1), (0, 0)), ((0, 3), (0, 1)), ((8, 8), (2, 2))]
OS_SPECIALISED = OS_WINDOWS[:2]                  # windows with a k_cfar2d_os_mask_v instance
# (train, guard, plane): the last four reach the CA half of k_cfar2d and / or the Wd > 128 pairwise recursion
CA_WINDOWS = [((4, 4), (2, 2), PLANE_A), ((1, 1), (0, 0), PLANE_B), ((2, 9), (1, 3), PLANE_A),
              ((25, 25), (4, 4), (75, 67)), ((1, 62), (0, 2), (9, 150)), ((3, 60), (0, 4), (12, 150)),
              ((1, 126), (0, 4), (5, 300))]
WINDOWS_1D = [(3, 1), (10, 2), (70, 2), (140, 3), (300, 4), (512, 0)]
ROW_LEN = 1301
# quantisation levels per OS window (test_cfar_cases_host.py asserts the tie floors they give)
OS_LEVELS = {((5, 5), (3, 2)): 8, ((4, 4), (2, 2)): 8, ((2, 2), (1, 1)): 8, ((1, 1), (0, 0)): 8, ((0, 3), (0, 1)): 8,
             ((8, 8), (2, 2)): 8}


OS_SEED = 7


def os_ranks_1d(T):
    """1, T, 2T and the two ranks just below the top: with the two NaNs of the non-finite row in one window those are
    the largest numbers, +inf among them."""
    return sorted({1, T, 2 * T, max(1, 2 * T - 1), max(1, 2 * T - 2)})


def os_plane_shape(train, guard):
    """45 x 70 and 70 x 45 alternate over the windows."""
    return PLANE_B if (train[0] + guard[1]) % 2 else PLANE_A


def os_ranks_2d(train, guard):
    """1, 2, N/2, N-1, N and the two ranks either side of a coarse bucket edge of k_cfar2d's fast path: its first probe
    counts the training cells whose rank in the 16 x 16 tile + halo is below 8 * npad / 16, which for a window of N
    training cells is about N * (npad / 2) / n_tile of them -- k <= that count takes the lower half, k above the upper."""
    n = n_train_2d(train, guard)
    n_tile = (16 + 2 * (train[0] + guard[0])) * (16 + 2 * (train[1] + guard[1]))
    npad = 1 << (n_tile - 1).bit_length()
    edge = min(n - 1, max(1, n * (npad // 2) // n_tile))
    return sorted({1, min(2, n), max(1, n // 2), max(1, n - 1), n, edge, edge + 1})


def planes_2d(shape, levels, seed, half, negate_ramp=False):   # OS cases: seed = OS_SEED
    """The four frames of one mmw_cfar2d call: quantised, constant, ramp (or its negation), non-finite."""
    rp = ramp(shape)
    return np.stack([quantised(shape, levels, seed), constant(shape), -rp if negate_ramp else rp,
                     nonfinite(shape, seed + 1, half)[0]])


def rows_1d(T, G, levels=6, seed=0, n_rows=5, L=ROW_LEN):
    """Five rows of one mmw_cfar1d call, each from another builder: quantised, constant, ramp, negated ramp, non-finite."""
    rows = [quantised(L, levels, seed + T), constant(L), ramp(L), -ramp(L), nonfinite(L, seed + T + 1, T + G)[0]]
    return np.stack(rows[:n_rows])
