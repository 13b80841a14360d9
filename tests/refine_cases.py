"""Seeded inputs and float64 references for the float64 refinement of mmw_angle_argmax_exact (no GPU needed).

A case is a complex64 cube [F][V][S][C], a detection list dets [F][cap][2] int32 (range bin, fftshifted Doppler index) with
counts [F], and the oracle's answers (oracle/oracle_np.py: range_doppler in complex128, angle_argmax) for any antenna list.

Every evaluation is FLAGGED by construction.  The certainty test of the float32 pass compares the winner's margin with a
bound proportional to the L1 norm of the windowed plane, so the cube is unit-variance complex noise plus one strong
component of amplitude P_TONE per antenna that raises the L1 norm and reaches only the 3 x 3 cells around (r0, k0):

    x[s][c] = noise + P e^(j phi[f][v]) e^(2 pi j (r0 s / S + k0 c / C)) g_S[s] g_C[c],   g_N[n] = u_N[n] / np.hanning(N)[n],
    u_N[n]  = 1 - cos(2 pi (n + 1/2) / N) / cos(pi / N)          (g_N = 0 where the window is 0: n = 0 and N - 1)

np.hanning is the SYMMETRIC window: under it a plain on-grid tone leaks 0.17 / m^3 of its peak into bin m of its row and
column, far above the noise at any useful P.  u_N is the first-order trigonometric polynomial with the window's zeros, so
hann(N) * g_N = u_N and the windowed component is an on-grid tone times a raised cosine per axis: it occupies range bins
r0 - 1 .. r0 + 1 and Doppler bins k0 - 1 .. k0 + 1 and nothing else (float32 rounding of the samples aside, which scatters
2^-24 P per sample over all cells like noise).  Detections lie outside that neighbourhood: their cells and margins are
noise-level whatever P is, while the bound grows with P.  Planes with S = 2 or C = 2 have np.hanning = [0, 0]: every
cell is exactly zero, every evaluation is flagged without a tone and the argmax is index 0.

P_TONE: tests/test_gpu_argmax_refine.py asserts n_refined == evaluations before anything else and reports P when that fails;
the measured value is recorded at its definition below.

An evaluation whose float64 angle spectrum has (best - second) / best < 1e-9 is excluded from index comparisons (two correct
float64 evaluations may differ there); a case may exclude at most 1 % of its evaluations (checked for every case by
tests/test_refine_cases_host.py; with noise-level cells the expected number is zero).  A spectrum that is flat bit for bit is
not excluded: all-zero cells, or a list of one antenna, whose every bin is x * W^0 = x exactly; the first maximum is
index 0 in any correct evaluation.
"""
import functools

import numpy as np

from oracle import oracle_np as O

# Measured on an MI355X over every plane and antenna list of this file (both shifts): P = 10 leaves 64 of 70 list / plane pairs
# short of n_refined == evaluations, 100 leaves 10 (the 8 x 10 plane, the 16-antenna list), 1e3 .. 1e7 none.  The cases use
# 100 x the smallest power of ten that passes.  |x| <= 4.1 P + noise: finite in float32 by 32 orders; the float32 rounding
# of the strong component, 2^-24 P g <= 0.025 per sample, stays below the unit noise.
P_TONE = 1e5
MARGIN_MIN = 1e-9
MAX_EXCLUDED_SHARE = 0.01
A_BINS = 64


def taper(N):
    """g_N: hann(N) * g_N = u_N, the raised cosine whose zeros are the window's (n = 0, N - 1)."""
    w = np.hanning(N)
    n = np.arange(N)
    g = np.zeros(N)
    if N >= 3:
        u = 1.0 - np.cos(2 * np.pi * (n + 0.5) / N) / np.cos(np.pi / N)
        g[1:-1] = u[1:-1] / w[1:-1]
    return g


def tone_of(S, C):
    """(r0, k0) of the strong component, None for planes too small to keep detections away from it."""
    if S < 5 or C < 5:
        return None
    return (S // 3 + 1, (C // 4 - C // 2) % C)      # fftshifted Doppler index C // 4: clear of 0, C/2 - 1, C/2 and C - 1


def doppler_index(k, C):
    """fftshifted Doppler index of FFT bin k (np.fft.fftshift moves bin 0 to C // 2)."""
    return (k + C // 2) % C


def allowed_cells(S, C):
    """Boolean [S][C] over (range bin, fftshifted Doppler index): False on the tone's 3 x 3 neighbourhood (cyclic)."""
    ok = np.ones((S, C), dtype=bool)
    t = tone_of(S, C)
    if t is not None:
        r0, d0 = t[0], doppler_index(t[1], C)
        for dr in (-1, 0, 1):
            for dd in (-1, 0, 1):
                ok[(r0 + dr) % S, (d0 + dd) % C] = False
    return ok


def make_cube(seed, F, V, S, C, P=None):
    P = P_TONE if P is None else P
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((F, V, S, C)) + 1j * rng.standard_normal((F, V, S, C))) / np.sqrt(2.0)
    t = tone_of(S, C)
    if t is not None:
        phi = rng.uniform(0, 2 * np.pi, (F, V, 1, 1))
        s, c = np.arange(S)[:, None], np.arange(C)[None, :]
        tone = np.exp(2j * np.pi * (t[0] * s / S + t[1] * c / C)) * taper(S)[:, None] * taper(C)[None, :]
        x = x + P * np.exp(1j * phi) * tone
    return x.astype(np.complex64)


class Case:
    def __init__(self, name, seed, shape, cap, counts, layout="random", P=None):
        self.name, self.seed, self.cap = name, seed, int(cap)
        self.F, self.V, self.S, self.C = shape
        self.counts = np.asarray(counts, dtype=np.int32)
        assert len(self.counts) == self.F
        self.P = P_TONE if P is None else P
        self.tone = tone_of(self.S, self.C)
        if layout == "sparse":         # thousands of frames, a handful with detections: only those hold samples, the rest zeros
            self.cube = np.zeros((self.F, self.V, self.S, self.C), dtype=np.complex64)
            for f in np.nonzero(self.counts)[0]:
                self.cube[f] = make_cube(seed + 3 * int(f) + 2, 1, self.V, self.S, self.C, self.P)[0]
        else:
            self.cube = make_cube(seed, self.F, self.V, self.S, self.C, self.P)
        self.dets = self._dets(layout)
        self._rd = {}

    def listed(self, f):
        return int(min(max(self.counts[f], 0), self.cap))

    @property
    def n_evals(self):
        return sum(self.listed(f) for f in range(self.F))

    def _dets(self, layout):
        rng = np.random.default_rng(self.seed + 1)
        S, C = self.S, self.C
        rr, dd = np.nonzero(allowed_cells(S, C))
        dets = np.full((self.F, max(self.cap, 1), 2), -12345, dtype=np.int32)      # unlisted slots: never to be read
        for f in range(self.F):
            n = self.listed(f)
            if n == 0:
                continue
            m = max(n, self.cap)           # (cap draws whatever the count: cases of one seed share their leading detections)
            pick = rng.choice(len(rr), size=m, replace=m > len(rr))[:n]
            cells = np.stack([rr[pick], dd[pick]], axis=1)
            fixed = []
            if layout == "corners":        # FFT bins k = d - C/2 on both sides of the wrap, first and last range bin
                fixed = [(r, d) for r in (0, S - 1) for d in (0, C // 2 - 1, C // 2, C - 1)]
            elif layout == "duplicates":
                fixed = [tuple(cells[-1])] * 5
            for i, cell in enumerate(fixed[:n]):
                cells[(3 * i) % n if layout == "duplicates" else i] = cell
            dets[f, :n] = cells
        return dets

    def rd(self, f):
        """The oracle's complex128 range-Doppler cube of frame f, [V][S][C] (fftshifted Doppler axis)."""
        if f not in self._rd:
            self._rd[f] = O.range_doppler(self.cube[f])
        return self._rd[f]

    @functools.lru_cache(maxsize=None)
    def expected(self, ants, shift):
        """(idx [F][cap] int32 with -1 on unlisted slots, excluded [F][cap] bool, smallest non-excluded relative margin)."""
        idx = np.full((self.F, max(self.cap, 1)), -1, dtype=np.int32)
        excl = np.zeros(idx.shape, dtype=bool)
        worst = np.inf
        for f in range(self.F):
            n = self.listed(f)
            if n == 0:
                continue
            i, resp = O.angle_argmax(self.rd(f), self.dets[f, :n, 0], self.dets[f, :n, 1], list(ants), A_BINS, bool(shift))
            top = np.sort(resp, axis=1)[:, -2:]
            best, second = top[:, 1], top[:, 0]
            flat = resp.max(axis=1) == resp.min(axis=1)     # zero cells, or ONE antenna (every bin is |x| exactly): index 0
            rel = np.where(flat, np.inf, (best - second) / np.where(best > 0, best, 1.0))
            idx[f, :n] = i
            excl[f, :n] = rel < MARGIN_MIN
            if np.any(~excl[f, :n]):
                worst = min(worst, float(rel[~excl[f, :n]].min()))
        return idx, excl, worst


def antennas(V, n=4):
    return tuple(range(min(n, V)))


# ---- the cases -------------------------------------------------------------------------------------------------------------
DENSE_S = (8, 63, 64, 100, 256, 512, 829)
DIRECT_PLANES = ((63, 100), (254, 50), (16, 320), (32, 256), (8, 10), (127, 2), (2, 5))
LAYOUT_PLANES = ((256, 128), (100, 128))
ANT_LISTS = {
    "len1": (5,), "len3": (0, 1, 2), "len4": (4, 5, 6, 7), "len5": (0, 2, 4, 6, 8), "len8": tuple(range(8)),
    "len9": tuple(range(3, 12)), "len16": tuple(range(16)), "len32": tuple(range(32)),
    "repeated": (3, 3, 7, 1, 3), "descending": (11, 9, 8, 5, 2, 0),
}
# frame counts on both sides of every step of refine_parts(n_frames): 16 slices while 16 F <= 60000, 8 while 8 F <= 60000, ...
PARTS_STEPS = (3750, 3751, 7500, 7501, 15000, 15001)
# ... on the planes whose cubes stay small at 15001 frames (63 x 100, 254 x 50, 16 x 320 and 32 x 256 would take 1.5 to 6 GB there
# and are left out of the frame-count sweep for that reason alone).  8 x 10, 127 x 2 and 2 x 5 fit one slice of 256 cells whatever
# the slice count; 20 x 56 = 1120 cells is here because its slicing CHANGES with it: 16 and 8 slices of 256 cells (five
# hold cells, the last 96), 4 of 512 (three, the last 96), 2 of 768 (768 + 352).
PARTS_PLANES = ((8, 10), (127, 2), (2, 5), (20, 56))


# name -> (seed offset, F, V, cap, counts, layout); the seeds are fixed per case (vetted against the exclusion cap)
_LAYOUTS = {
    "corners": (0, 2, 4, 16, [12, 9], "corners"),
    "duplicates": (7, 2, 4, 16, [11, 16], "duplicates"),
    "n256": (14, 2, 4, 256, [256, 10], "random"),                 # exactly one full chunk of k_cells64
    "n257": (21, 2, 4, 264, [257, 10], "corners"),                # a second chunk of one cell
    "n513": (28, 3, 4, 520, [513, 5, 0], "random"),               # three chunks, two passes of the 512-thread detection scan
    "n700": (35, 3, 4, 704, [0, 700, 0], "duplicates"),           # total <= 256 F: all dense
    "tail": (42, 2, 4, 1024, [600, 300], "random"),               # 900 > dense_cap = 512: the rest takes the direct kernels
    "overcap": (49, 2, 4, 48, [48 + 7, 20], "corners"),
    "alternating": (56, 4, 4, 32, [24, 0, 24, 0], "random"),
}
_LAYOUT_SEED0 = {(256, 128): 2312, (100, 128): 2219}


_SPECS = {}
for _S in DENSE_S + (830,):
    _SPECS[f"plane_{_S}x128"] = (100 + _S, (2, 4, _S, 128), 48, [40, 33], "corners")
for _S, _C in LAYOUT_PLANES:
    for _n, (_off, _F, _V, _cap, _cnt, _lay) in _LAYOUTS.items():
        _SPECS[f"{_n}_{_S}x{_C}"] = (_LAYOUT_SEED0[(_S, _C)] + _off, (_F, _V, _S, _C), _cap, _cnt, _lay)
_SPECS["thr31_64x128"] = (3100, (4, 4, 64, 128), 8, [8, 8, 8, 7], "random")
_SPECS["thr32_64x128"] = (3100, (4, 4, 64, 128), 8, [8, 8, 8, 8], "random")     # same seed: the first 31 are shared
_SPECS["ants_64x128"] = (3200, (2, 32, 64, 128), 24, [24, 17], "corners")
for _S, _C in DIRECT_PLANES:
    _SPECS[f"direct_{_S}x{_C}"] = (4000 + 13 * _S + _C, (3, 4, _S, _C), 24, [min(24, (_S * _C) // 2), 0, 5], "corners")
for _i, (_S, _C) in enumerate(PARTS_PLANES):
    for _F in PARTS_STEPS:
        _cnt = np.zeros(_F, dtype=np.int32)
        _cnt[[0, 1, _F // 2, _F - 1]] = (2, 1, 2, 2)
        _SPECS[f"parts_{_F}_{_S}x{_C}"] = (5000 + 20000 * _i + _F, (_F, 4, _S, _C), 2, _cnt, "sparse")
# value-level (mmw_rd_cells64_at) planes of the dense route beyond the layout planes
for _S in (8, 63, 512):
    _SPECS[f"value_{_S}x128"] = (6000 + _S, (2, 4, _S, 128), 300, [290, 12], "corners")
_SPECS["value_100x128"] = (6100, (2, 4, 100, 128), 300, [290, 12], "corners")
_SPECS["value_256x128"] = (6256, (2, 4, 256, 128), 300, [290, 12], "corners")
NAMES = tuple(_SPECS)


_cases = {}


def case(name, P=None):
    """The case of that name, built once (cubes above 64 MB are built per call and not kept)."""
    if (name, P) in _cases:
        return _cases[(name, P)]
    seed, shape, cap, counts, layout = _SPECS[name]
    c = Case(name, seed, shape, cap, counts, layout, P)
    if c.cube.nbytes <= 64 << 20:
        _cases[(name, P)] = c
    return c


# ---- value level: np.longdouble direct sums and the a-priori error bounds ------------------------------------------------
PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def _phase(N, m):
    """exp(-2 pi j m n / N), n = 0 .. N-1, in np.clongdouble (the angle reduced in integers first)."""
    n = np.arange(N, dtype=np.int64)
    ang = -2 * PI_LD * ((m * n) % N).astype(np.longdouble) / np.longdouble(N)
    return np.cos(ang) + 1j * np.sin(ang)


def longdouble_cells(cube_f, cells, ants):
    """Range-Doppler cells (r, fftshifted d) of antennas `ants` of one frame as np.longdouble direct double sums of the
    windowed float32 cube: (values [n][n_ant] clongdouble, L1w [n_ant] = sum |w_s w_c x|)."""
    V, S, C = cube_f.shape
    ws, wc = np.hanning(S).astype(np.longdouble), np.hanning(C).astype(np.longdouble)
    out = np.zeros((len(cells), len(ants)), dtype=np.clongdouble)
    l1 = np.zeros(len(ants), dtype=np.longdouble)
    ES = np.stack([_phase(S, int(r)) for r, _ in cells]) * ws[None, :]                              # [n][S]
    EC = np.stack([_phase(C, (int(d) - C // 2) % C) for _, d in cells]) * wc[None, :]               # [n][C]
    for j, a in enumerate(ants):
        X = cube_f[a].astype(np.clongdouble)
        out[:, j] = np.sum((ES @ X) * EC, axis=1)
        l1[j] = np.sum(np.abs(X) * ws[:, None] * wc[None, :])
    return out, l1


U = 2.0 ** -53


def refine_parts(n_frames):
    p = 16
    while p > 2 and p * n_frames > 60000:
        p //= 2
    return p


def gamma_dense(S, C=128):
    """|cell error| <= gamma 2^-53 L1w for k_cells64, every rounding lined up (u = 2^-53; a complex product with a table
    entry: 3 u for the product + 1 u for the entry):
      window product  hann(C)[c] * hann(S)[s] (2 entries + 1) and x * w (1)                       4
      16-point register FFT: 4 radix-2 levels of (add 1 + twiddle product 4)                     20
      one inter-level twiddle product                                                             4
      8-point register FFT: 3 levels                                                             15
      range twiddle: entry 1 + up to 7 steps of c = cmul(c, step) at 4                           29
      z * c inside the fused multiply-adds                                                        2
      8 ceil(S / 64) sequential fused multiply-adds per lane                         8 ceil(S / 64)
      3 shuffle adds                                                                              3"""
    return 77 + 8 * -(-S // 64)


def gamma_direct(S, C, n_frames):
    """The same for k_argmax_refine_part + the slice sum:
      two table products  twS * ws, twC * wc (2 entries + 1 each) and their product (3)           9
      x * ph                                                                                      3
      per-thread sequential sum of ceil(per / 256) terms, per = slice length (a multiple of 256)
      6-step wave reduction 6, 4-wave sum 2, sequential sum of the slices: parts"""
    parts = refine_parts(n_frames)
    per = -(-(-(-(S * C) // parts)) // 256) * 256
    return 12 + per // 256 + 6 + 2 + parts


def gamma_numpy(S, C):
    """Yardstick for the oracle's np.fft.fft2 of the windowed cube: two window products (2 each), then per axis and per prime
    factor p of its length (with multiplicity) one radix-p pass: p - 1 adds + a twiddle product at 4, bounded by p + 4."""
    def omega(n):
        tot, p = 0, 2
        while n > 1:
            while n % p == 0:
                tot += p + 4
                n //= p
            p += 1
        return tot
    return 4 + omega(S) + omega(C)
