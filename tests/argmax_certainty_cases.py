"""Seeded evaluations and np.longdouble labels for the certainty decision of mmw_angle_argmax_exact (no GPU needed).

The float32 argmax kernels decide per evaluation whether their first maximum is PROVABLY the float64 one (mmw_argmax.h,
mmw_detect.h).  This module builds evaluations whose answer is known from the design alone and leaves the
kernel's own arithmetic out of the labels:

    cells  x[n_ant] complex64       what the kernel gathers from d_rd at a detection
    l1     [n_ant] float32          the plane norms it reads from d_l1;  e_i = k_fft l1_i,  Be = sum e_i
    c_ang  = k_ang sum (|re x_i| + |im x_i|),   k_fft = ulps(S, C) 2^-24,   k_ang = 4 (n_ant + 4) 2^-24

All label arithmetic is np.longdouble on the float32 values.

must-flag   an admissible perturbation |d_i| <= e_i (1 - 2^-20) changes the exact first maximum.  Found by the first-order
            adversary  d_i = e_i unit(conj(conj(u_k) W^(i k) - conj(u_1) W^(i k_1))),  u = S / |S| recomputed from x + d, six
            iterates from d = 0, for every competitor bin k with m_1 - m_k <= 2 Be (no other bin can be flipped: each
            magnitude moves by at most Be).  A flip is verified exactly: bin k ahead of the winner at x + d in np.argmax order.
            Also: a non-finite cell, all-zero cells, one antenna (a flat spectrum), and a winner that is tied within the
            reference's own precision (2^-58 relative) with another bin.
must-clear  exact margin > 2 (Be + c_ang) + 2 c_ang: the float32 magnitudes lie within c_ang of the exact ones of the same
            cells (the design's claim), so such an evaluation passes the kernel's independent-errors test.
undecided   everything else.

A dispatch (one row of DISPATCHES: angle bins, list length, context options) is a d_rd of F = 4 frames of an 8 x 16 plane with
one evaluation per cell (cap = 128) and one l1 profile per frame: flat, one antenna carrying > 90 % of Be, zero on every
other listed antenna, and all zero.  Inside a frame the cells of every evaluation are scaled so that its exact margin sits
on a rung of the ladder: below the adversary's first-order reach against the runner-up (0.2 .. 0.8 of it), at 0.75 .. 0.95 of
the largest scale at which the iterated adversary still flips some bin (found by bisection: these must-flag rows sit above
1.001 times the first-order term wherever the second-order term decides), and above 2 Be + 4 c_ang (1.03 .. 100 times:
must-clear).  In units of Be the rungs run from Be = margin / 0.6 or more down to Be = margin / 200.

Shapes (kinds): two tones with the second one 1, 17, 31 bins away or off the grid, amplitudes from 0.5 to 1 - 1e-4 of the
first (close ones make the far bin the runner-up, otherwise a neighbour of the peak is); `weak`: one tone and a runner-up far
below it (with the flag rungs m_1 ~ Be and m_k << Be: the regime of the Be^2 / (2 min) term); `noise`: Gaussian cells, the
flat spectra of noise-level detections; `edge`: energy on the first and last antenna only, the sharpest peak a list can have
-- with 1024 and 2048 bins the neighbour of any other peak is inside 4 c_ang and nothing else can be must-clear.
`null`: one on-grid tone with a bin in a zero of its pattern at 1e-3 of the peak (m_k ~ 0; on the frontier rungs m_1 ~ Be).
With l1 = 0 there is no admissible perturbation: the rungs are multiples of 4 c_ang (must-clear); every third row (`ulp`, counted
apart from the caps) has a margin of a float32 ulp of the peak or a few: undecided by definition, but an unflagged answer must
still be the exact argmax of the float32 cells; and `tie` rows (real cells: bins k and A - k are equal) are the only must-flag ones.
"""
import functools
from collections import namedtuple

import numpy as np

import rd_bound_cases as rb

LD, CLD = np.longdouble, np.clongdouble
PI_LD = LD("3.14159265358979323846264338327950288")
S, C, CAP, V, F = 8, 16, 128, 32, 4
COUNTS = (128, 121, 100, 128)
PROFILES = ("flat", "dominant", "half_zero", "zero")
EPS = LD(2) ** -24
SHRINK = 1 - LD(2) ** -20
TIE_TOL = LD(2) ** -58
ITERATIONS = 6
# 8 x 16 goes through the run-time mixed-radix kernel: the structured count (36) + its plan's level lengths 8, 1, 4, 4
# (tests/test_argmax_certainty_cases_host.py ties both to mmw_diag_rd_plan / mmw_diag_detect_plan)
RUNTIME_LEVELS = (8, 1, 4, 4)
ULPS = rb.structured_ulps(S, C) + sum(RUNTIME_LEVELS)
K_FFT = LD(ULPS) * EPS
N_SPECIAL = 6                                       # the first slots of every frame
MUST_FLAG, MUST_CLEAR, UNDECIDED = 1, 2, 0

Dispatch = namedtuple("Dispatch", "name kernel A n_ant options pairwise")
FORM0 = {"MMW_ARGMAX_FORM": 0}
DISPATCHES = (
    [Dispatch(f"dets{N}_n{n}", f"k_angle_argmax_dets<{N}>", 64, n, {}, True) for N, n in ((4, 3), (4, 4), (8, 7), (8, 8), (16, 12), (16, 16))]
    + [Dispatch(f"lanes{N}_onebin_n{n}", f"k_angle_argmax_lanes<{N}> one bin", 64, n, FORM0, True) for N, n in ((4, 4), (8, 8))]
    + [Dispatch(f"lanes{4 if n <= 4 else 8}_A{A}_n{n}", f"k_angle_argmax_lanes<{4 if n <= 4 else 8}> multi-bin", A, n, {}, True)
       for A, n in ((32, 4), (128, 8), (1024, 4), (1024, 8), (48, 4), (48, 8))]
    + [Dispatch(f"generic{n}_A2048", f"k_angle_argmax<{n}> pairwise", 2048, n, {}, True) for n in (4, 8)]
    + [Dispatch("generic16_A128_n12", "k_angle_argmax<16>", 128, 12, {}, False),
       Dispatch("generic32_A64_n20", "k_angle_argmax<32>", 64, 20, {}, False),
       Dispatch("generic32_A64_n32", "k_angle_argmax<32>", 64, 32, {}, False)]
    # the edges of the list length: two antennas, as many antennas as bins
    + [Dispatch("dets4_n2", "k_angle_argmax_dets<4>", 64, 2, {}, True),
       Dispatch("lanes8_A8_n8", "k_angle_argmax_lanes<8> multi-bin, n_ant == A", 8, 8, {}, True),
       Dispatch("generic32_A32_n32", "k_angle_argmax<32>, n_ant == A", 32, 32, {}, False)]
)
# one antenna: every spectrum is flat, every evaluation must be flagged (no ladder, no caps)
FLAT_DISPATCH = Dispatch("dets4_n1", "k_angle_argmax_dets<4>", 64, 1, {}, True)
BY_NAME = {d.name: d for d in DISPATCHES + [FLAT_DISPATCH]}

FLAG_RUNGS = (0.2, 0.35, 0.5, 0.65, 0.8, 0.45)      # of the first-order reach against the runner-up
FRONT_RUNGS = (0.95, 0.9, 0.85, 0.75)               # of the largest scale at which the iterated adversary still flips some bin
CLEAR_RUNGS = (1.03, 1.1, 1.3, 2.0, 5.0, 20.0, 100.0, 1.06, 1.6, 3.0)
ULP_RUNGS = (0.0005, 0.002, 0.01, 0.05)             # l1 = 0: margins of a float32 ulp of the peak and a few, in units of 4 c_ang


def k_ang(n_ant):
    return 4 * LD(n_ant + 4) * EPS


def antennas(n_ant):
    """The antenna list of a dispatch: distinct, unordered, not starting at 0."""
    return tuple((5 + 7 * i) % V for i in range(n_ant))


def twiddles(A):
    """W_A^m = exp(-2 pi j m / A), m < A, np.clongdouble."""
    ang = -2 * PI_LD * np.arange(A).astype(LD) / LD(A)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)


@functools.lru_cache(maxsize=None)
def steering(A, n):
    """[n][A]: W_A^(i k)."""
    return twiddles(A)[np.outer(np.arange(n), np.arange(A)) % A]


def out_index(k, A, shift):
    """Output index of FFT bin k (np.fft.fftshift moves bin 0 to A // 2)."""
    return (k + A // 2) % A if shift else k


def bin_of(kk, A, shift):
    return (kk + A - A // 2) % A if shift else kk


def kinds_of(A):
    base = ("adj", "far17", "far31", "offgrid", "weak", "noise", "null")
    return tuple(k for pair in zip(base, ("edge",) * len(base)) for k in pair) if A >= 1024 else base


def l1_profile(profile, n_ant, rng):
    """float32 [V]: the listed antennas by profile, the unlisted ones 0 or 1e9 in turn (a kernel that reads the norm of an
    antenna outside the list, or of the wrong list position, gets a bound that is wrong by orders)."""
    l1 = np.where(np.arange(V) % 2 == 0, 0.0, 1e9)
    base = 3e4
    ants = antennas(n_ant)
    for i, a in enumerate(ants):
        if profile == "flat":
            l1[a] = base * (1 + 0.1 * rng.random())
        elif profile == "dominant":
            l1[a] = base if i == n_ant // 2 else 0.08 * base / max(n_ant - 1, 1) * (0.5 + rng.random())
        elif profile == "half_zero":
            l1[a] = base * (1 + 0.1 * rng.random()) if i % 2 == 0 else 0.0
        else:
            l1[a] = 0.0
    return l1.astype(np.float32)


# ------------------------------------------------------------------ shapes
def _allowed_bins(A):
    """FFT bins whose output index is not 0 under either shift, and not next to such a bin."""
    bad = {0, (A - A // 2) % A}
    return [k for k in range(A) if all((k + d) % A not in bad for d in (-1, 0, 1))] or [k for k in range(A) if k not in bad]


def _tone(A, n, k):
    """e^(+2 pi j i k / A): the cells whose spectrum peaks at bin k (k may be fractional)."""
    return np.exp(2j * np.pi * np.arange(n) * float(k) / A).astype(CLD)


def _edge(A, n, rng, b):
    """1 on the first antenna, b e^(j theta) on the last, 2 % of that between them: the sharpest peak of a list.  The peak bin is one whose theta is next
    to a multiple of pi / 2, so that sum |re| + |im| (c_ang) is as small as the magnitudes allow."""
    ks = np.array(_allowed_bins(A))
    th = 2 * np.pi * (n - 1) * ks / A
    good = ks[np.argsort(np.abs(np.cos(th)) + np.abs(np.sin(th)), kind="stable")[:8]]
    x = 0.02 * _tone(A, n, int(rng.choice(good)))      # (a little on the antennas between: no grating lobes as high as the peak)
    x[n - 1] *= LD(b) / LD(0.02)
    x[0] = 1.0
    return x


def shape(kind, A, n, rng):
    k1 = int(rng.choice(_allowed_bins(A)))
    if kind == "noise":
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(CLD)
    elif kind == "weak":
        x = _tone(A, n, k1) + 10.0 ** rng.uniform(-4, -2) * np.exp(2j * np.pi * rng.random()) * _tone(A, n, k1 + A / 2 + rng.random())
    elif kind == "null":
        # one on-grid tone and a bin in (or next to) a zero of its pattern forced to 1e-3 of the peak with a drawn phase: m_k ~ 0, and
        # on the front rungs m_1 ~ Be -- what the kernel's Be^2 / (2 min(m_1, m_k)) term is for (first order has no say: u_k is arbitrary)
        x = _tone(A, n, k1)
        kz = (k1 + max(1, round(A / n)) * int(rng.integers(1, max(2, n)))) % A
        wz = steering(A, n)[:, kz]
        x = x - (np.sum(x * wz) - 1e-3 * n * np.exp(2j * np.pi * rng.random())) * np.conj(wz) / n
    elif kind == "edge":
        return _edge(A, n, rng, rng.uniform(0.8, 1.0))
    elif kind == "tie":
        for _ in range(20):                    # real cells (no phase factor) whose two equal peaks are not at output index 0
            kt = int(rng.integers(A // 8 + 1, max(A // 8 + 2, 3 * A // 8)))
            x = (rng.uniform(0.5, 1.0, n) * np.cos(2 * np.pi * np.arange(n) * kt / A + 0.3)).astype(np.float32).astype(CLD)
            if int(np.argmax(np.abs(x @ steering(A, n)))) % (A - A // 2) != 0:
                return x
        return np.zeros(n, dtype=CLD)
    else:
        dk = {"adj": 1, "far17": 17 % A, "far31": 31 % A, "offgrid": 5.37 if A > 12 else 2.37}[kind] or 1
        a2 = 1 - 10.0 ** rng.uniform(-4, np.log10(0.5))
        x = _tone(A, n, k1) + a2 * np.exp(2j * np.pi * rng.random()) * _tone(A, n, k1 + dk)
    x = x * np.exp(2j * np.pi * rng.random())
    # move the peak to an allowed bin (a two-tone peak may sit on the second tone, a noise peak anywhere)
    kmax = int(np.argmax(np.abs(x @ steering(A, n))))
    if kmax not in _allowed_bins(A):
        x = x * _tone(A, n, k1 - kmax)
    return x


def _unit(z):
    m = np.abs(z)
    return np.where(m > 0, z / np.where(m > 0, m, 1), 1).astype(CLD)


def _flips(x, e, A, n_near=8):
    """Does the iterated adversary flip the evaluation (x, e)?  The n_near closest and the n_near smallest competitors only: this
    places rungs, labels() decides with every competitor."""
    W = steering(A, len(x))
    m = np.abs(x @ W)
    k1 = int(np.argmax(m))
    gap = m[k1] - m
    gap[k1] = np.inf
    order = np.argsort(gap)
    ks = np.unique(np.concatenate([order[:n_near], order[-1 - n_near:-1]]))
    ks = ks[gap[ks] <= 2 * e.sum()]
    if not len(ks):
        return False
    return bool(_adversary(x[None, :], e[None, :], W, np.array([k1]), np.zeros(len(ks), dtype=int), ks, A, 0).any())


def _front_scale(x, e, A, mu0):
    """The largest factor s (of 16 bisection steps in log s) at which _flips(s x) holds; None if it never does."""
    be = e.sum()
    hi = 2.2 * be / mu0                        # margin > 2 Be: nothing flips
    lo = hi / 4096
    if not be > 0 or not _flips(x * lo, e, A):
        return None
    for _ in range(16):
        mid = np.sqrt(lo * hi)
        if _flips(x * mid, e, A):
            lo = mid
        else:
            hi = mid
    return lo


def _reach(spec, W, e, k1, kr):
    """First-order reach of the adversary against bin kr: sum e_i |conj(u_kr) W^(i kr) - conj(u_k1) W^(i k1)| (the kernel's lin)."""
    return np.sum(e * np.abs(np.conj(_unit(spec[kr])) * W[:, kr] - np.conj(_unit(spec[k1])) * W[:, k1]))


def _scale_for(x, e, A, rung_kind, rho, kang):
    """The factor that puts the exact margin of s x on the rung; None where the shape cannot reach it."""
    n = len(x)
    W = steering(A, n)
    spec = x @ W
    m = np.abs(spec)
    order = np.argsort(-m, kind="stable")
    k1, kr = int(order[0]), int(order[1])
    mu0 = m[k1] - m[kr]
    be = e.sum()
    s1 = np.sum(np.abs(x.real) + np.abs(x.imag))
    if not mu0 > 0:
        return None
    if rung_kind == "front":
        s = _front_scale(x, e, A, mu0)
        return None if s is None else rho * s
    if rung_kind == "flag":
        reach = _reach(spec, W, e, k1, kr)
        return rho * reach / mu0 if reach > 0 else None
    assert rung_kind == "clear"
    den = mu0 - 4 * rho * kang * s1 * LD(1.03)
    return 2 * rho * be / den if den > 0 and be > 0 else None


def _bisect(family, lo, hi, W, target_rel, kang):
    """family(t) with margin / (4 c_ang) above target_rel at t = lo and below it at hi: the member next to the target, from above."""
    def rel(t):
        x = family(t)
        m = np.sort(np.abs(x @ W))
        return (m[-1] - m[-2]) / (4 * kang * np.sum(np.abs(x.real) + np.abs(x.imag)))

    if rel(lo) < target_rel:
        return None
    for _ in range(30):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if rel(mid) > target_rel else (lo, mid)
    return family(lo)


def _tune_two_tone(A, n, rng, target_rel, kang):
    """l1 = 0: a two-tone shape whose exact margin is target_rel * 4 c_ang, by bisection on the second amplitude; the second
    tone sits where the first has a zero or a low sidelobe so that it is the runner-up once the amplitudes are close."""
    k1 = int(rng.choice(_allowed_bins(A)))
    for _ in range(50):                        # (neither tone at output index 0 under either shift: at a margin of an ulp either may win)
        k1 = int(rng.choice(_allowed_bins(A)))
        dk = max(1, int(round(A / n))) * int(rng.integers(1, max(2, n // 2 + 1))) if n > 1 else 1
        if (k1 + dk) % A not in (0, (A - A // 2) % A):
            break
    W = steering(A, n)
    t1, t2 = _tone(A, n, k1), np.exp(2j * np.pi * rng.random()) * _tone(A, n, (k1 + dk) % A)
    ph = np.exp(2j * np.pi * rng.random())
    seed = int(rng.integers(1 << 30))
    if A >= 1024 and target_rel >= 1:          # only the edge shape reaches multiples of 4 c_ang here: bisection on its second amplitude
        x = _bisect(lambda b: _edge(A, n, np.random.default_rng(seed), b), LD(1), LD(0), W, target_rel, kang)
    else:                                      # the margin falls from the single tone's to ~0 as a2 -> 1
        x = _bisect(lambda a2: (t1 + a2 * t2) * ph, LD(0), LD(1), W, target_rel, kang)
    if x is None:
        return None
    kmax = int(np.argmax(np.abs(x @ W)))
    if kmax not in _allowed_bins(A):
        x = x * _tone(A, n, k1 - kmax)
    return x


def _special(j, A, n, rng):
    """The first slots of a frame: non-finite cells, all-zero cells, a tie."""
    x = (shape("far17", A, n, rng) * 100).astype(np.complex64)
    i = int(rng.integers(0, n))
    if j == 0:
        x[i] = np.complex64(complex(np.nan, 1.0))
    elif j == 1:
        x[i] = np.complex64(complex(np.inf, 0.0))
    elif j == 2:
        x[i] = np.complex64(complex(2.0, -np.inf))
    elif j == 3:
        x[:] = 0
    elif j == 4:
        x = (shape("tie", A, n, rng) * 50).astype(np.complex64)
    elif j == 5:
        x[i] = np.complex64(complex(0.0, np.nan))
    return x


Built = namedtuple("Built", "dispatch ants rd l1 dets counts cells e kind profile rung listed")


@functools.lru_cache(maxsize=None)
def build(name):
    """The device inputs of a dispatch and, per evaluation slot [F * CAP], its cells, error scales, kind, profile and rung."""
    d = BY_NAME[name]
    A, n = d.A, d.n_ant
    rng = np.random.default_rng(9100 + 17 * A + n + (1000 if d.options else 0))
    ants = antennas(n)
    kang = k_ang(n)
    rd = ((rng.standard_normal((F, V, S, C)) + 1j * rng.standard_normal((F, V, S, C))) * 1e3).astype(np.complex64)   # unlisted antennas: garbage
    l1 = np.stack([l1_profile(p, n, rng) for p in PROFILES])
    dets = np.empty((F, CAP, 2), dtype=np.int32)
    cells = np.zeros((F * CAP, n), dtype=np.complex64)
    e = np.zeros((F * CAP, n), dtype=LD)
    kind = np.empty(F * CAP, dtype=object)
    rung = np.empty(F * CAP, dtype=object)
    profile = np.repeat(np.array(PROFILES, dtype=object), CAP)
    kinds = kinds_of(A)
    for f in range(F):
        perm = rng.permutation(S * C)               # the detection list visits the plane's cells in a seeded order
        dets[f, :, 0], dets[f, :, 1] = perm // C, perm % C
        ef = K_FFT * l1[f, list(ants)].astype(LD)
        ladder = [("flag", r) for r in FLAG_RUNGS] + [("front", r) for r in FRONT_RUNGS] + [("clear", r) for r in CLEAR_RUNGS]
        for slot in range(CAP):
            q = f * CAP + slot
            e[q] = ef
            x = _special(slot, A, n, rng) if slot < N_SPECIAL else None
            if x is not None:
                kind[q], rung[q] = "special", ("special", slot)
            else:
                j = slot - N_SPECIAL
                kd = kinds[j % len(kinds)]
                if PROFILES[f] == "zero":
                    step = j // len(kinds)
                    rg = ("ulp", ULP_RUNGS[(step // 3) % len(ULP_RUNGS)]) if step % 3 == 2 else ("clear0", CLEAR_RUNGS[step % len(CLEAR_RUNGS)])
                    xs = _tune_two_tone(A, n, rng, LD(rg[1]) * (LD(1.03) if rg[0] == "clear0" else 1), kang) if n > 1 else None
                    if xs is None:                  # no shape reaches the rung at this many bins: a tie (must-flag) instead
                        xs, rg = shape("tie", A, n, rng), ("tie", 0.0)
                    kd = "ulp" if rg[0] == "ulp" else "l1_zero"
                    s = 10.0 ** rng.uniform(-2, 3)
                else:
                    rg = ladder[(j // len(kinds) + j) % len(ladder)]
                    for _ in range(6 if rg[0] == "clear" and A < 1024 else 1):     # (an unresolved pair may have no margin to speak of: draw again)
                        xs = shape(kd, A, n, rng)
                        s = _scale_for(xs, ef, A, rg[0], LD(rg[1]), kang)
                        if s is not None:
                            break
                    for alt in (1.3, 1.1, 1.03):    # the shape cannot be that far above 4 c_ang at this many bins: a lower rung,
                        if s is None and rg[0] == "clear":
                            s = _scale_for(xs, ef, A, "clear", LD(alt), kang)
                            rg = ("clear", alt) if s is not None else rg
                    if s is None:                   # ... or a must-flag rung instead
                        rg = ("flag", FLAG_RUNGS[j % len(FLAG_RUNGS)])
                        s = _scale_for(xs, ef, A, "flag", LD(rg[1]), kang)
                    if s is None:
                        s = 1.0
                x = (xs * s).astype(np.complex64)
                kind[q], rung[q] = kd, rg
            cells[q] = x
            for i, a in enumerate(ants):
                rd[f, a, dets[f, slot, 0], dets[f, slot, 1]] = x[i]
    listed = (np.arange(CAP)[None, :] < np.array(COUNTS)[:, None]).reshape(-1)
    for arr in (rd, l1, dets, cells):
        arr.setflags(write=False)
    return Built(d, ants, rd, l1, dets, np.array(COUNTS, dtype=np.int32), cells, e, kind, profile, rung, listed)


# ------------------------------------------------------------------ labels
Labels = namedtuple("Labels", "winner label margin be c_ang")


def _first_max(m_out):
    """(first index within TIE_TOL of the row maximum, whether a second bin is that close)."""
    top = m_out.max(axis=1, keepdims=True)
    close = m_out >= top * (1 - TIE_TOL)
    return np.argmax(close, axis=1), close.sum(axis=1) > 1


def _adversary(x, e, W, k1, pairs_q, pairs_k, A, shift):
    """For pairs (evaluation q, competitor bin k): does some iterate put bin k ahead of the winner?  [P] bool."""
    xq, eq = x[pairs_q], e[pairs_q] * SHRINK
    w1, wk = W[:, k1[pairs_q]].T, W[:, pairs_k].T                 # [P][n]
    lower = out_index(pairs_k, A, shift) < out_index(k1[pairs_q], A, shift)
    d = np.zeros_like(xq)
    hit = np.zeros(len(pairs_q), dtype=bool)
    for _ in range(ITERATIONS):
        s1, sk = np.sum((xq + d) * w1, axis=1), np.sum((xq + d) * wk, axis=1)
        g = np.conj(_unit(sk))[:, None] * wk - np.conj(_unit(s1))[:, None] * w1
        d = eq * np.conj(_unit(g)) * (np.abs(g) > 0)
        m1, mk = np.abs(np.sum((xq + d) * w1, axis=1)), np.abs(np.sum((xq + d) * wk, axis=1))
        hit |= (mk > m1) | ((mk == m1) & lower)
    return hit


@functools.lru_cache(maxsize=None)
def labels(name, shift):
    """Per evaluation slot: the exact winner's OUTPUT index (-1: none, the answer is the refinement's 0), the label, and the
    exact margin, Be and c_ang behind it."""
    b = build(name)
    A, n = b.dispatch.A, b.dispatch.n_ant
    E = len(b.cells)
    W = steering(A, n)
    finite = np.isfinite(b.cells.view(np.float32).reshape(E, 2 * n)).all(axis=1)
    x = np.where(finite[:, None], b.cells, 0).astype(CLD)
    m = np.abs(x @ W)                                              # [E][A]
    perm = bin_of(np.arange(A), A, shift)                          # output index -> FFT bin
    win_out, tied = _first_max(m[:, perm])
    k1 = perm[win_out]
    m1 = m[np.arange(E), k1]
    rest = m.copy()
    rest[np.arange(E), k1] = -1
    margin = m1 - rest.max(axis=1) if A > 1 else m1
    be = b.e.sum(axis=1)
    c = k_ang(n) * np.sum(np.abs(x.real) + np.abs(x.imag), axis=1)
    label = np.full(E, UNDECIDED, dtype=np.int8)
    forced = ~finite | (m1 == 0) | tied | (n == 1)
    label[forced] = MUST_FLAG
    label[~forced & (margin > 2 * (be + c) + 2 * c)] = MUST_CLEAR
    todo = np.nonzero((label == UNDECIDED) & (be > 0))[0]
    if len(todo):
        gap = m1[todo, None] - m[todo]                             # [T][A]
        cand = gap <= 2 * be[todo, None]
        cand[np.arange(len(todo)), k1[todo]] = False
        # the closest competitors first; whoever survives them meets the rest
        near = np.argsort(np.where(cand, gap, np.inf), axis=1)[:, :6]
        pq = np.repeat(todo, near.shape[1])
        pk = near.reshape(-1)
        keep = cand[np.repeat(np.arange(len(todo)), near.shape[1]), pk]
        hit = _adversary(x, b.e, W, k1, pq[keep], pk[keep], A, shift)
        label[np.unique(pq[keep][hit])] = MUST_FLAG
        left = label[todo] == UNDECIDED
        tq, tk = np.nonzero(cand & left[:, None])
        for lo in range(0, len(tq), 50000):
            sl = slice(lo, lo + 50000)
            hit = _adversary(x, b.e, W, k1, todo[tq[sl]], tk[sl], A, shift)
            label[np.unique(todo[tq[sl]][hit])] = MUST_FLAG
    winner = np.where(forced, -1, win_out).astype(np.int64)
    return Labels(winner, label, margin, be, c)


def tally(name, shift):
    """{family: (must-flag, must-clear, undecided)} over the listed ladder evaluations: the dispatch, each kind, each profile."""
    b, lab = build(name), labels(name, shift)
    out = {}
    ladder = b.listed & (b.kind != "special") & (b.kind != "ulp")
    groups = [("all", ladder)] + [(f"kind:{k}", ladder & (b.kind == k)) for k in sorted(set(b.kind[ladder]))]
    groups += [(f"l1:{p}", ladder & (b.profile == p)) for p in PROFILES]
    for key, sel in groups:
        out[key] = tuple(int(np.count_nonzero(lab.label[sel] == v)) for v in (MUST_FLAG, MUST_CLEAR, UNDECIDED))
    return out


# ------------------------------------------------------------------ the kernel's two inequalities, restated in float64
def restated_flags(name, shift):
    """[E] bool: what the design's decision gives in float64 on the same cells (no float32 emulation): flagged unless
    best - second > 2 (Be + c_ang), or -- lists with the pairwise pass -- every other bin k passes that or
    m_1 - m_k > 1.001 (sum e_i |t1_i - tk_i| + Be^2 / (2 min(m_1, m_k))) + 2 c_ang."""
    b = build(name)
    A, n = b.dispatch.A, b.dispatch.n_ant
    E = len(b.cells)
    W = steering(A, n).astype(np.complex128)
    e = b.e.astype(np.float64)
    flagged = np.ones(E, dtype=bool)
    with np.errstate(all="ignore"):
        x = b.cells.astype(np.complex128)
        spec = x @ W
        m = np.abs(spec)
        perm = bin_of(np.arange(A), A, shift)
        k1 = perm[np.argmax(m[:, perm], axis=1)]
        m1 = m[np.arange(E), k1]
        be = e.sum(axis=1)
        c = float(k_ang(n)) * np.sum(np.abs(x.real) + np.abs(x.imag), axis=1)
        two_b = 2 * (be + c)
        gap = m1[:, None] - m
        gap[np.arange(E), k1] = np.inf
        flagged = ~(gap.min(axis=1) > two_b)
        if b.dispatch.pairwise:
            for q in np.nonzero(flagged & np.isfinite(m1) & (m1 > 0))[0]:
                u1 = spec[q, k1[q]] / m1[q]
                t1 = np.conj(u1) * W[:, k1[q]]                                   # [n]
                uk = np.where(m[q] > 0, spec[q] / np.where(m[q] > 0, m[q], 1), 0)
                lin = np.sum(e[q][:, None] * np.abs(t1[:, None] - np.conj(uk)[None, :] * W), axis=0)      # [A]
                ok = (gap[q] > two_b[q]) | ((m[q] > 0) & (gap[q] > 1.001 * (lin + be[q] ** 2 / (2 * np.minimum(m1[q], m[q]))) + 2 * c[q]))
                flagged[q] = not ok.all()
    return flagged
