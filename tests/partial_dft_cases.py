"""Counted rounding bound, exact inputs, float32 restatement and mutants for the partial-DFT kernels k_micro_doppler and
k_sar_slices (mmw_md_core.h, mmw_micro_doppler.h, mmw_sar.h).  NumPy only; nothing here touches the device.

The inequality under test, per output value of one antenna's [S][C] slab x (complex64):

    SAR block element     |dev - X[r][k]|               <=  ulps(S, C)       * 2^-24 * L1
    micro-Doppler column  |dev - max_r |X[r][k]||       <=  ulps(S, C, True) * 2^-24 * L1,      L1 = sum_s sum_c |x[s][c]|

X = the two direct sums in np.longdouble (``reference``; no np.fft: its own error is of the order tested here).  Every twiddle
has magnitude 1, so L1 bounds every partial sum; the micro-Doppler row inherits the bound because
|max_r a_r - max_r b_r| <= max_r |a_r - b_r|.  Both hold while no float32 intermediate leaves the normal range
(``scaling_interval``; include/mmwgpu.h states that as the contract).

test_partial_dft_cases_host.py checks this module against itself on the CPU; test_gpu_partial_dft_bound.py runs the same cases
on the device.  References are built once per case (``reference_of``) and never modified.
"""
import math
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -24
LD = np.longdouble
PI_L = LD("3.14159265358979323846264338327950288")
KTS = (None, 4, 8, 16)                  # the default choice of md_pick_kt and the three forced instantiations
SPEC_TOL = 1e-5                         # the present bar: within 1e-5 of the peak of the frame's full plane


# ------------------------------------------------------------------------------------------------------------ the bound
# u = 2^-24.  An output is Y = sum_c Zh[c] Wh_C^(c k), Zh[c] = sum_s Wh_S^(r s) x[s][c], hats = float32.  Counted from the code:
#
#   1   stage 1's table entry: k_md_twiddle / k_sar_twiddle (mmw_micro_doppler.h:24, mmw_sar.h:40) copy W_S^m from the table
#       make_table rounds from long double (mmw_ctx.h:176-177): each component within u of its value, the entry within u |W|.
#   2 sqrt2 ceil(S / 4)
#       md_cmac along a wave's chain (mmw_md_core.h:37-40, called at mmw_micro_doppler.h:72-73 and mmw_sar.h:84-85; wave w
#       owns s = w, w + 4, ...: at most ceil(S / 4) samples).  A component of the accumulator is a chain of two fmaf per sample,
#       2 ceil(S / 4) roundings on its oldest product, and |re| + |im| terms of one component sum to at most |W| |x| (Cauchy-
#       Schwarz).  Real and imaginary part err independently, so the modulus of the error carries the factor sqrt 2.
#   3   wave 0's combine ((P0 + P1) + P2) + P3 per component (mmw_micro_doppler.h:93-94, mmw_sar.h:105-106): three additions.
#   1   stage 2's table entry W_C^m (mmw_micro_doppler.h:110, mmw_sar.h:121), as above.
#   2 sqrt2 C
#       md_cmac along the C terms of stage 2 (mmw_micro_doppler.h:119-120, mmw_sar.h:121): two fmaf per term and component.
#
# first order:  n = 5 + ceil(2 sqrt2 (ceil(S / 4) + C)).  Every factor is of the form (1 + u)^j, they compound to at most
# (1 + u)^n - 1 <= n u + (n u)^2 for n u <= 1/2 (n <= 2^23), so  ulps = n + ceil(n^2 / 2^24) + 1  covers the second order; the
# last 1 pays for the table's double rounding (long double to float) and for |Wh| <= 1 + u.
#
# The micro-Doppler row adds sqrtf(fmaf(re, re, im * im)) (mmw_micro_doppler.h:127-128, :140): three roundings, a product, the
# fmaf and the root.  Both terms under the root are non-negative, so the first two are relative errors of |Y|^2 and halve under
# the root: (1 + u)^(2/2) (1 + u) -- two ulps of |Y| <= L1 (1 + n u).  The maximum itself is exact.
def first_order(S, C):
    return 5 + math.ceil(2 * math.sqrt(2) * (-(-S // 4) + C))


def ulps(S, C, magnitude=False):
    """Worst-case count of float32 roundings (units of 2^-24 L1) on one output of stage 1 followed by stage 2."""
    n = first_order(S, C) + (2 if magnitude else 0)
    return n + -(-n * n // 2 ** 24) + 1


def l1_of(x):
    return float(np.sum(np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64))))


def fft_bins(cols, C):
    """FFT bin behind column ``cols`` of np.fft.fftshift: (c + C - C/2) mod C, odd C included."""
    return (np.asarray(cols, dtype=np.int64) + C - C // 2) % C


# -------------------------------------------------------------------------------------------------------- the reference
def _unit_ld(num, den):
    """exp(-2 pi i num / den) in long double for integer arrays, the index reduced in integers first."""
    ang = -(LD(2) * PI_L) * (np.asarray(num, dtype=np.int64) % den).astype(LD) / LD(den)
    return np.cos(ang) + 1j * np.sin(ang)


_row_twiddles = {}


def reference(x, rows, bins):
    """X[r][k] = sum_s sum_c x[s][c] W_S^(r s) W_C^(c k) for r in rows, k in bins: two direct sums in long double."""
    S, C = x.shape
    rows, bins = np.asarray(rows, dtype=np.int64), np.asarray(bins, dtype=np.int64)
    xl = x.real.astype(LD) + 1j * x.imag.astype(LD)
    key = (S, rows.tobytes())
    if key not in _row_twiddles:            # the one-hot family asks for the same rows of the same S many times
        _row_twiddles.clear()
        _row_twiddles[key] = _unit_ld(rows[:, None] * np.arange(S)[None, :], S)
    z = _row_twiddles[key] @ xl
    return z @ _unit_ld(np.arange(C)[:, None] * bins[None, :], C)


def micro_doppler_reference(x, lo, hi):
    """max over the window's rows of |X|, at np.fft.fftshift's columns: [C] long double."""
    C = x.shape[1]
    return np.abs(reference(x, np.arange(lo, hi + 1), fft_bins(np.arange(C), C))).max(axis=0)


def sar_reference(x, win):
    r0, r1, c0, c1 = win
    return reference(x, np.arange(r0, r1), fft_bins(np.arange(c0, c1), x.shape[1]))


# -------------------------------------------------------------------------------------- float32 restatement of the kernels
def table(N):
    """make_table<float>(TAB_TWIDDLE, N): W_N^m rounded from long double, quarter turns exact.  (re [N], im [N]) float32."""
    m = np.arange(N, dtype=np.int64)
    ang = (LD(-2) * PI_L * m.astype(LD)) / LD(N)
    c, s = np.cos(ang), np.sin(ang)
    q = np.where((4 * m) % N == 0, (4 * m) // N, -1)
    c = np.where(q == 0, 1, np.where(q == 2, -1, np.where(q >= 0, 0, c)))
    s = np.where(q == 1, -1, np.where(q == 3, 1, np.where(q >= 0, 0, s)))
    return c.astype(np.float32), s.astype(np.float32)


def float_angle_table(num, den):
    """Mutant twiddles: cosf / sinf of the unreduced float32 angle -2 pi num / den."""
    ang = np.float32(-2 * np.pi) * np.asarray(num).astype(np.float32) / np.float32(den)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there (TwoSum gives
    the sign of what was lost), and a round-to-odd double rounds to float32 like the exact value."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
        c = np.broadcast_to(np.asarray(c, dtype=np.float32).astype(np.float64), p.shape)
        s = p + c
        bb = s - p
        t = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(t) & (t != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(t > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


class Track:
    """Binary exponents of the smallest non-zero and the largest float32 intermediate, apart for the values that scale with
    the input (``lin``) and with its square (``sq``); whether any was subnormal or not finite."""

    def __init__(self):
        self.lo = {"lin": None, "sq": None}
        self.hi = {"lin": None, "sq": None}
        self.bad = False

    def see(self, a, kind="lin"):
        a = np.abs(np.asarray(a, dtype=np.float32)).ravel()
        if not np.all(np.isfinite(a)):
            self.bad = True
            a = a[np.isfinite(a)]
        a = a[a != 0]
        if a.size:
            lo, hi = float(a.min()), float(a.max())
            self.bad |= lo < 2.0 ** -126
            self.lo[kind] = lo if self.lo[kind] is None else min(lo, self.lo[kind])
            self.hi[kind] = hi if self.hi[kind] is None else max(hi, self.hi[kind])
        return self


def _cmac(acc, a, b, track):
    """md_cmac: acc += a b, four fmaf in the kernel's order."""
    ax, ay = acc
    ax = fma32(a[0], b[0], ax)
    ay = fma32(a[0], b[1], ay)
    ax = fma32(-a[1], b[1], ax)
    ay = fma32(a[1], b[0], ay)
    if track is not None:
        track.see(ax).see(ay)
    return ax, ay


def stage1(x, rows, mutant=None, track=None):
    """Z[k][c] = sum_s W_S^(rows[k] s) x[s][c] as the kernels add it: wave w the samples s = w, w + 4, ..., then
    ((P0 + P1) + P2) + P3.  (re, im) float32 [K][C]."""
    S, C = x.shape
    rows = np.asarray(rows, dtype=np.int64) % S
    xr, xi = np.ascontiguousarray(x.real, dtype=np.float32), np.ascontiguousarray(x.imag, dtype=np.float32)
    tab = table(S)
    if track is not None:
        track.see(xr).see(xi)
    parts = []
    for w in range(4):
        acc = (np.zeros((len(rows), C), np.float32), np.zeros((len(rows), C), np.float32))
        for s in range(w, S, 4):
            if mutant == "float_angle":
                tw = float_angle_table(rows * s, S)
            else:
                m = (rows * s) % S
                tw = (tab[0][m], tab[1][m])
            acc = _cmac(acc, (tw[0][:, None], tw[1][:, None]), (xr[s][None, :], xi[s][None, :]), track)
        parts.append(acc)
    if mutant == "drop_wave3_tail":
        tail = 64 * (C // 64)
        parts[3][0][:, tail:] = 0
        parts[3][1][:, tail:] = 0
    with np.errstate(all="ignore"):
        zx, zy = parts[0]
        for q in range(1, 4):
            zx, zy = zx + parts[q][0], zy + parts[q][1]
            if track is not None:
                track.see(zx).see(zy)
    return zx, zy


def stage2(z, bins, mutant=None, track=None):
    """Y[k][j] = sum_c Z[k][c] W_C^(c bins[j]), c ascending, the twiddle from the table at (c bin) mod C."""
    zx, zy = z
    K, C = zx.shape
    bins = np.asarray(bins, dtype=np.int64)
    tab = table(C)
    acc = (np.zeros((K, len(bins)), np.float32), np.zeros((K, len(bins)), np.float32))
    for c in range(C - 1 if mutant == "drop_last_term" else C):
        if mutant == "float_angle":
            tw = float_angle_table(c * bins, C)
        else:
            m = (c * bins) % C
            tw = (tab[0][m], tab[1][m])
        acc = _cmac(acc, (zx[:, c:c + 1], zy[:, c:c + 1]), (tw[0][None, :], tw[1][None, :]), track)
    return acc


MUTANTS = ("drop_wave3_tail", "drop_last_term", "padded_rows", "odd_shift", "float_angle", "signed_max")


def kt_fits(kt, C):
    """md_lds_bytes(kt, C) <= MD_LDS_MAX: a forced number of rows in flight that the LDS does not hold is refused."""
    return 3 * kt * 128 * 8 + C * kt * 8 + C * 8 + C * 4 <= 160 * 1024


def pick_kt(K, forced=None):
    """md_pick_kt where every KT fits the LDS (the shapes of this module): least padded rows + 2 passes, the larger on a tie."""
    if forced:
        return forced
    return min((16, 8, 4), key=lambda kt: -(-K // kt) * (kt + 2))


def f32_micro_doppler(x, lo, hi, kt=None, mutant=None, track=None, nan_sign=False):
    """k_micro_doppler on one slab, float32 [C].  nan_sign: every NaN of |Y|^2 carries the sign bit, as an implementation
    may produce it (the sign of a NaN that arithmetic makes is not defined; the kernel's mask makes it irrelevant)."""
    S, C = x.shape
    K = hi - lo + 1
    KT = pick_kt(K, kt)
    rows = lo + np.arange(-(-K // KT) * KT if mutant == "padded_rows" else K)
    yx, yy = stage2(stage1(x, rows, mutant, track), np.arange(C), mutant, track)
    with np.errstate(all="ignore"):
        sq = yy * yy
        v = fma32(yx, yx, sq)
    if track is not None:
        track.see(sq, "sq").see(v, "sq")
    if nan_sign:
        bits = v.view(np.uint32).copy()
        bits[np.isnan(v)] |= np.uint32(0x80000000)
        v = bits.view(np.float32)
    if mutant == "signed_max":
        best = np.maximum(v.view(np.int32).max(axis=0), 0).astype(np.int32).view(np.float32)
    else:
        best = (v.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=0).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        root = np.sqrt(best)
    if track is not None:
        track.see(root)
    out = np.empty(C, np.float32)
    if mutant == "odd_shift":
        out[:] = root[(np.arange(C) + C // 2) % C]
    else:
        out[(np.arange(C) + C // 2) % C] = root
    return out


def f32_sar(x, win, mutant=None, track=None):
    """k_sar_slices on one slab: complex64 [r1 - r0][c1 - c0]."""
    S, C = x.shape
    r0, r1, c0, c1 = win
    cols = np.arange(c0, c1)
    bins = (cols + C // 2) % C if mutant == "odd_shift" else fft_bins(cols, C)
    yx, yy = stage2(stage1(x, np.arange(r0, r1), mutant, track), bins, mutant, track)
    out = np.empty(yx.shape, np.complex64)
    out.real, out.imag = yx, yy
    return out


# ----------------------------------------------------------------------------------------------------------- the checks
def sar_ratio(got, x, win):
    """Worst |got - ref| / (ulps 2^-24 L1) over a block."""
    S, C = x.shape
    err = np.abs((got.real.astype(LD) + 1j * got.imag.astype(LD)) - reference_of(x, ("sar", tuple(win))))
    return float(err.max() / (LD(ulps(S, C)) * LD(EPS) * LD(l1_of(x))))


def md_ratio(got, x, lo, hi):
    S, C = x.shape
    err = np.abs(got.astype(LD) - reference_of(x, ("md", lo, hi)))
    return float(err.max() / (LD(ulps(S, C, True)) * LD(EPS) * LD(l1_of(x))))


_refs = {}


def reference_of(x, what):
    """The long double reference of (slab, window), computed once and shared (keyed by the slab's identity: the case lists
    below own their slabs and never modify them)."""
    key = (id(x), what)
    if key not in _refs:
        ref = sar_reference(x, what[1]) if what[0] == "sar" else micro_doppler_reference(x, what[1], what[2])
        ref.setflags(write=False)
        _refs[key] = (x, ref)               # holds x so that its id stays its own
    return _refs[key][1]


# ------------------------------------------------------------------------------------------------------ the input families
SarCase = namedtuple("SarCase", "name x win")                # x [S][C] complex64, win (row_lo, row_hi, col_lo, col_hi) half open
MdCase = namedtuple("MdCase", "name x lo hi")                # rows lo .. hi inclusive


def _frozen(x):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    x.setflags(write=False)
    return x


def _impulses(S, C, cells):
    x = np.zeros((S, C), np.complex64)
    for s, c, a in cells:
        x[s, c] += a
    return _frozen(x)


A_SHAPES = ((8, 7), (63, 70), (5, 130), (1021, 3))          # 1021 x 3 with every row: r s0 up to 1020^2 >= 2^16


def a_cells(S, C):
    """(s0, c0): s0 = S - 1 ... S - 4, one of each residue mod 4; c0 at the ends of a lane's two columns and of the slab."""
    return [(s0, c0) for s0 in range(S - 1, S - 5, -1) for c0 in sorted({c for c in (0, 63, 64, 127, 128, C - 1) if c < C})]


_built = {}


def _once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def family_a(S, C):
    """One-hot impulses, the full plane as the window: X[r][k] = W_S^(r s0) W_C^(c0 k), every index its own test."""
    return _once(("a", S, C), lambda: [SarCase(f"a-{S}x{C}-s{s0}c{c0}", _impulses(S, C, [(s0, c0, 1)]), (0, S, 0, C))
                                       for s0, c0 in a_cells(S, C)])


B_SHAPES = ((29, 11), (20, 130))
B_KS = (1, 4, 5, 8, 9, 16, 17)
B_AMP = 0.5


def b_cells(S, C, K):
    """Two impulses whose K + 2 rows lo - 1 ... hi + 1 span about one turn of the phase between them, so that in some
    columns the strongest row is lo - 1 and in others hi + 1: (s0, c0), (s1, c1)."""
    ds = max(1, int(round(S / (K + 2))))
    return (2, C - 1), (2 + ds, 2)


def b_closed_form(S, C, K, lo, hi):
    """max_{lo <= r <= hi} |1 + a W_S^(r ds) W_C^(dc k)| per fftshifted column, the phase kept in integers:
    sqrt(1 + a^2 + 2 a cos(2 pi d / (S C))), d the least distance of r ds C + k dc S from a multiple of S C over the rows."""
    (s0, c0), (s1, c1) = b_cells(S, C, K)
    k = fft_bins(np.arange(C), C)
    r = np.arange(lo, hi + 1)
    num = (r[:, None] * (s1 - s0) * C + k[None, :] * (c1 - c0) * S) % (S * C)
    d = np.minimum(num, S * C - num).min(axis=0)
    a = LD(B_AMP)
    return np.sqrt(1 + a * a + 2 * a * np.cos(2 * PI_L * d.astype(LD) / LD(S * C)))


def family_b(S, C):
    def make():
        out = []
        for K in B_KS:
            (s0, c0), (s1, c1) = b_cells(S, C, K)
            out.append(MdCase(f"b-{S}x{C}-K{K}", _impulses(S, C, [(s0, c0, 1), (s1, c1, B_AMP)]), 1, K))
        return out
    return _once(("b", S, C), make)


C_SHAPES = ((1021, 3), (3, 1021), (256, 128))


def _coherent(S, C, r0, k0, amp):
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    w = np.conj(_unit_ld(r0 * s, S) * _unit_ld(k0 * c, C)) * LD(amp)
    return _frozen(w.real.astype(np.float32) + 1j * w.imag.astype(np.float32))


def family_c(S, C):
    """(SarCase, MdCase) pairs on coherent slabs: every term adds in phase at (r0, k0), so L1 equals the peak.  The window holds
    the peak, two rows on either side and up to 33 columns around it."""
    def make():
        out = []
        for r0, k0, amp in ((0, 0, 0.7), (S - 1 if S > 3 else 1, (2 * C) // 3, 1.3)):
            x = _coherent(S, C, r0, k0, amp)
            col = (k0 + C // 2) % C
            lo, hi = max(0, r0 - 2), min(S - 1, r0 + 2)
            win = (lo, hi + 1, max(0, col - 16), min(C, col + 17))
            out.append((SarCase(f"c-{S}x{C}-r{r0}k{k0}", x, win), MdCase(f"c-{S}x{C}-r{r0}k{k0}", x, lo, hi)))
        return out
    return _once(("c", S, C), make)


D_SHAPES = ((64, 32), (63, 20), (40, 23), (8, 130), (16, 1), (1, 8))


def md_windows(S):
    """test_gpu_micro_doppler.windows: a single row, lo == 0, hi == S - 1, the full span, an inner window of three rows."""
    out = {(S // 2, S // 2), (0, min(5, S - 1)), (max(0, S - 20), S - 1), (0, S - 1)}
    if S > 20:
        out.add((S // 3, S // 3 + 2))
    return sorted(out)


def gaussian(S, C):
    def make():
        rng = np.random.default_rng([77, S, C])
        return _frozen(rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
    return _once(("gauss", S, C), make)


def family_d(S, C):
    """Gaussian slabs: the full plane as one SAR window, every window of md_windows for the micro-Doppler row."""
    x = gaussian(S, C)
    return SarCase(f"d-{S}x{C}", x, (0, S, 0, C)), [MdCase(f"d-{S}x{C}-{lo}_{hi}", x, lo, hi) for lo, hi in md_windows(S)]


def full_plane_peak(x):
    """The largest magnitude of the slab's full plane, what the present bar is relative to."""
    S, C = x.shape
    return float(np.abs(reference_of(x, ("sar", (0, S, 0, C)))).max())


# ------------------------------------------------------------------------------------------- family E: powers of two
E_SHAPE, E_MD_WINDOW = (63, 20), (43, 62)


def scaled(x, e):
    """x 2^e, exact while every component stays a normal float32."""
    out = np.empty(x.shape, np.complex64)
    out.real, out.imag = np.ldexp(x.real, e), np.ldexp(x.imag, e)
    return out


def _exp(v):
    return math.frexp(v)[1]             # v = f 2^p, 1/2 <= f < 1


def scaling_interval(track):
    """[e_lo, e_hi]: the powers of two by which the input may be scaled with every intermediate of ``track`` (recorded at
    e = 0) still a normal, finite float32.  A value f 2^p, 1/2 <= f < 1, is finite while p <= 128 and normal while p >= -125;
    the linear ones move by e, the squares by 2 e."""
    e_lo, e_hi = -10 ** 9, 10 ** 9
    for kind, step in (("lin", 1), ("sq", 2)):
        if track.lo[kind] is not None:
            e_lo = max(e_lo, -((125 + _exp(track.lo[kind])) // step))          # ceil((-125 - p) / step)
            e_hi = min(e_hi, (128 - _exp(track.hi[kind])) // step)
    return e_lo, e_hi


def e_case():
    """(slab, micro-Doppler window, SAR window, (e_lo, e_hi) of the micro-Doppler row, (e_lo, e_hi) of the SAR block)."""
    def make():
        x = gaussian(*E_SHAPE)
        S, C = E_SHAPE
        lo, hi = E_MD_WINDOW
        win = (lo, hi + 1, 0, C)
        t_md, t_sar = Track(), Track()
        f32_micro_doppler(x, lo, hi, track=t_md)
        f32_sar(x, win, track=t_sar)
        assert not t_md.bad and not t_sar.bad
        return x, (lo, hi), win, scaling_interval(t_md), scaling_interval(t_sar)
    return _once("e", make)


# ------------------------------------------------------------------------------------------- family F: non-finite slabs
F_SHAPE, F_WINDOW, F_CELL = (2, 40, 23), (3, 11), (17, 5)       # V x S x C, rows lo .. hi, the poisoned cell (s, c)


def f_cubes():
    """Three frames of two antennas, Gaussian, antenna 1 the one that is read."""
    def make():
        V, S, C = F_SHAPE
        rng = np.random.default_rng(91)
        x = (rng.standard_normal((3, V, S, C)) + 1j * rng.standard_normal((3, V, S, C))).astype(np.complex64)
        x.setflags(write=False)
        return x
    return _once("f", make)


def poisoned(cubes, value, frame=1, rx=1, other_antenna_nan=False):
    """``cubes`` with the real part of F_CELL of (frame, rx) set to the float32 ``value`` (given as bits, so that a NaN keeps
    its sign), and, on request, antenna 1 - rx of every frame NaN throughout."""
    out = cubes.copy()
    parts = out.view(np.float32).reshape(cubes.shape + (2,))
    parts[frame, rx, F_CELL[0], F_CELL[1], 0] = np.array([value], np.uint32).view(np.float32)[0]
    if other_antenna_nan:
        parts[:, 1 - rx] = np.nan
    return out


POS_NAN, NEG_NAN, POS_INF = 0x7FC00000, 0xFFC00000, 0x7F800000


# --------------------------------------------------------------------------------------------- the present bar's inputs
def tone_slab(S, C, lo, hi, seed=0, f=0, v=0):
    """test_gpu_micro_doppler.tone_cubes, one slab of it: on-bin tones at rows lo - 1, lo, hi, hi + 1, low noise."""
    rng = np.random.default_rng([seed, S, C, lo, hi])
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    x = 0.02 * (rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C)))
    for i, (row, amp) in enumerate(((lo - 1, 3.0), (lo, 4.0), (hi, 2.0), (hi + 1, 2.5))):
        if 0 <= row < S:
            dop = (1 + 5 * i + 2 * v + f) % C
            x = x + (amp + 0.3 * v) * np.exp(2j * np.pi * (row * s / S + dop * c / C))
    return _frozen(x)
