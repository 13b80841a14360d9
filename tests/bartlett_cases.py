"""Inputs and exact references for the Bartlett contraction's edge tests (test_bartlett_cases_host.py, test_gpu_bartlett_edges.py).

The operation (include/mmwgpu.h, mmw_bartlett):

    Y[f] = FFT_S( hann(S) . ( X[f] [S, E]  x  W[f] [E, T] ) ),    W[f][e, t] = hamming(E)[e] exp(2 pi j d_t . p_{f,e} / lambda)

NumPy only; nothing here touches the device.  Four families of inputs:

  A  geometry on a dyadic grid (lambda = 2^-8 m, positions in 2^-12 m, directions in 2^-10): d . p / lambda is then a multiple of
     2^-14 turns that float64 -- and an int64 -- holds exactly, so the reference takes the fraction of a turn in INTEGERS and the
     device's float64 dot product rounds nowhere.  Elements are planted at exactly 0, +-n and n + 1/2 turns and, where the span
     can hold it, beyond 2^11 turns with the 2^-14 bit set.  `steering_f32_mutant` is the kernel the large spans are there to
     catch: the same W with the turns rounded to float32 before the fraction is taken.
  B  power-of-two scalings of one Gaussian operand, the three-way bfloat16 split of csrc/mmw_bf16x3.h restated (`split3`), and an
     operand whose every part is +-(1 - 2^-24).
  C  one-hot operands: X[f] = 1 at (s0, e0), so row s0 of the contraction is column e0 of W and every k index is its own test.
  D/E  are built from A's cases inside the GPU test.
"""
import numpy as np

from oracle import oracle_np as O

SPEC_TOL = 1e-5                          # the project's spectra bar: of the peak magnitude of that frame's float64 reference
LAM_DYADIC = 2.0 ** -8                   # 3.9 mm, the 77 GHz scale; 1 / lambda = 256 exactly
LAM_77 = 299792458.0 / 77e9
P_UNIT, D_UNIT, TURN_UNIT = 2.0 ** -12, 2.0 ** -10, 2.0 ** -14      # P_UNIT * D_UNIT / LAM_DYADIC == TURN_UNIT
SPANS = {"0.05 m": 204, "4 m": 4 << 12, "16 m": 16 << 12}           # half-widths in units of 2^-12 m
LARGE_SPANS = ("4 m", "16 m")
MASKED, FAST = (70, 37, 10), (64, 64, 32)       # (S, E, T): a tail in every dimension / whole chunks and 16-byte rows
N_PLANTS = 7                                    # elements 0..6 and directions 0..1 are planted when E >= 7 and T >= 2


# ------------------------------------------------------------------------------------------------------------ A: geometry
def dyadic_geometry(F, E, T, span, seed):
    """Integer geometry: Pi [F, 3, E] in units of 2^-12 m inside +-span, Di [3, T] in units of 2^-10 inside +-1.  Against
    direction 0 = (1, 0, 0) a position of x units is x / 16 turns; every frame holds (when E >= 7 and T >= 2)
      e = 0   the origin: 0 turns against every direction
      e = 1   +n turns, n = span // 16 - 1          e = 2   -(n - 2) turns
      e = 3   (n - 4) + 1/2 turns                   e = 4   -(n - 5) + 1/2 turns
      e = 5   against direction 1 = (1023, 1023, 1023) / 1024: 1023 (3 span - 5) units of 2^-14 turns, an odd number beyond
              2^11 turns -- planted where the span reaches that far (3 span > 2^11 turns * 2^14 / 1023, the two large spans)
      e = 6   the mirror image of e = 5 (negative turns)."""
    rng = np.random.default_rng(seed)
    Pi = rng.integers(-span, span + 1, (F, 3, E)).astype(np.int64)
    Di = rng.integers(-1024, 1025, (3, T)).astype(np.int64)
    if E >= N_PLANTS and T >= 2:
        n = span // 16 - 1
        Di[:, 0] = (1024, 0, 0)
        Di[:, 1] = (1023, 1023, 1023)
        Pi[:, :, 0] = 0
        Pi[:, 0, 1:5] = (16 * n, -16 * (n - 2), 16 * (n - 4) + 8, -16 * (n - 5) + 8)
        if 1023 * (3 * span - 5) > 1 << 25:
            Pi[:, :, 5] = (span - 1, span - 1, span - 3)
            Pi[:, :, 6] = (-(span - 1), -(span - 3), -(span - 1))
    return Pi, Di


def turn_units(Pi, Di):
    """d_t . p_{f,e} / lambda in units of 2^-14 turns, [F, E, T] int64 (exact: at most 3 * 2^16 * 2^10 < 2^28)."""
    return np.einsum("fce,ct->fet", Pi, Di)


def steering_exact(Pi, Di):
    """W [F, E, T] complex128 with the fraction of a turn taken in integers."""
    frac = (turn_units(Pi, Di) & ((1 << 14) - 1)) * TURN_UNIT
    return np.hamming(Pi.shape[2])[None, :, None] * np.exp(2j * np.pi * frac)


def steering_f32_mutant(P, dirs, lam):
    """W of a kernel that converts the turns to float32 BEFORE it reduces them modulo one turn (P [F, 3, E], dirs [3, T])."""
    turns = (np.einsum("fce,ct->fet", P, dirs) / lam).astype(np.float32).astype(np.float64)
    return np.hamming(P.shape[2])[None, :, None] * np.exp(2j * np.pi * (turns - np.rint(turns)))


def response(X, W):
    """[F, S, T] complex128: the contraction, the Hann window over S, np.fft.fft over S."""
    X = np.asarray(X, dtype=np.complex128)
    return np.fft.fft(np.hanning(X.shape[1])[None, :, None] * (X @ W), axis=1)


def oracle_response(X, P, dirs, lam):
    """oracle.bartlett_response frame by frame, [F, S, T]."""
    d3 = np.asarray(dirs).reshape(3, -1, 1)
    return np.stack([O.bartlett_response(np.asarray(X[f], dtype=np.complex128), P[f], d3, lam)[:, :, 0] for f in range(len(X))])


def gaussian(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def worst_ratio(got, ref):
    """max over frames of max|got - ref| / max|ref|, each frame against its own peak."""
    return max(float(np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max()) for f in range(len(ref)))


def dyadic_case(shape, span_name, F=2, seed=0):
    """Gaussian X on the dyadic geometry of one span: X, P, dirs as the entry takes them, the integer geometry and `ref`."""
    S, E, T = shape
    Pi, Di = dyadic_geometry(F, E, T, SPANS[span_name], seed)
    X = gaussian((F, S, E), seed + 1000)
    return dict(X=X, P=Pi * P_UNIT, dirs=Di * D_UNIT, lam=LAM_DYADIC, Pi=Pi, Di=Di, ref=response(X, steering_exact(Pi, Di)))


def unit_case(shape, F=2, seed=0):
    """The non-dyadic case: unit steering vectors, lambda = c / 77 GHz, positions uniform in +-4 m; `ref` is the oracle."""
    S, E, T = shape
    naz, nel = {10: (5, 2), 32: (16, 2)}[T]
    dirs = O.steering_dirs(np.linspace(-0.9, 0.9, naz), np.linspace(-0.3, 0.3, nel)).reshape(3, T)
    P = np.random.default_rng(seed).uniform(-4.0, 4.0, (F, 3, E))
    X = gaussian((F, S, E), seed + 2000)
    return dict(X=X, P=P, dirs=dirs, lam=LAM_77, ref=oracle_response(X, P, dirs, LAM_77))


# ------------------------------------------------------------------------------------------------------------ B: scaling
SCALE_K = (-30, -8, 13, 27)
F32_TINY, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


def split3(v):
    """split_bf16x3 of csrc/mmw_bf16x3.h: p1 = v with the low 16 bits of its float32 pattern cleared, p2 = (v - p1) cleared
    likewise, p3 = the rest (the device keeps its high 16 bits, which is all of it)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    top = lambda a: (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)    # noqa: E731
    p1 = top(v)
    r = v - p1
    p2 = top(r)
    return p1, p2, r - p2


def parts(z):
    """Real and imaginary parts of a complex array as one flat real array."""
    z = np.ascontiguousarray(z)
    return z.view(z.real.dtype).ravel()


def scaled(z, k):
    """z 2^k in complex64 (exact while nothing leaves the normal range)."""
    return (np.asarray(z, dtype=np.complex64) * np.float32(np.ldexp(1.0, k))).astype(np.complex64)


def scaling_case():
    return dyadic_case(MASKED, "4 m", F=2, seed=11)


def ones_mantissa_case(seed=12):
    """Every real and imaginary part of X is +-(1 - 2^-24), bit pattern 0x3F7FFFFF: all three pieces of the split are full,
    so the three dropped products are as large as they get and share a sign."""
    c = dyadic_case(MASKED, "4 m", F=2, seed=seed)
    one = np.array([0x3F7FFFFF], dtype=np.uint32).view(np.float32)[0]
    sign = np.random.default_rng(seed).choice(np.float32([-1.0, 1.0]), c["X"].shape + (2,))
    c["X"] = np.ascontiguousarray(sign * one).view(np.complex64)[..., 0]
    c["ref"] = response(c["X"], steering_exact(c["Pi"], c["Di"]))
    return c


# ------------------------------------------------------------------------------------------------------------ C: impulses
CG_TM, CG_TN, CG_TK = 128, 64, 16               # csrc/mmw_beamform.h: the tiled GEMM's workgroup tile and K step
MI355X_CUS = 256
IMPULSE_S, IMPULSE_T, IMPULSE_E = 160, 40, (150, 128)
GEMM_FRAMES_PER_CALL = 2


def plan(num_cu, F, S, E, T):
    """(ksplit, kc) of bartlett_plan (csrc/mmw_beamform.h): part kz of the K split multiplies k in [kz kc, (kz + 1) kc)."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    wgs = cdiv(T, CG_TN) * cdiv(S, CG_TM) * F
    ksplit = 1
    if wgs * 2 <= num_cu and E >= 4 * CG_TK:
        ksplit = min(16, E // (2 * CG_TK), num_cu // (2 * wgs))
    if ksplit < 2:
        return 1, E
    kc = cdiv(cdiv(E, ksplit), CG_TK) * CG_TK
    return cdiv(E, kc), kc                      # (no empty part)


# 160 x E x 40 is 2 x 1 workgroup tiles per frame; with at most 2 frames on 256 CUs ksplit = min(16, E // 32, 256 // (2 wgs)) = 4,
# so kc = ceil(ceil(E / 4) / 16) * 16: 48 at E = 150 (parts from 0, 48, 96, 144), 32 at E = 128
KC = {150: 48, 128: 32}


def part_boundaries(E, num_cu=MI355X_CUS):
    """First k of every K-split part but the first, for every call size the GEMM paths are given."""
    out = set()
    for F in range(1, GEMM_FRAMES_PER_CALL + 1):
        ksplit, kc = plan(num_cu, F, IMPULSE_S, E, IMPULSE_T)
        out |= {kz * kc for kz in range(1, ksplit)}
    return sorted(out)


def index_list(E):
    """(s0, e0) per frame: the chunk, group and half-row boundaries of the tile kernels, then both sides of every part boundary."""
    e0 = [0, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, E - 2, E - 1]
    e0 += [k for b in range(KC[E], E, KC[E]) for k in (b - 1, b)]
    return [(IMPULSE_S // 2, e) for e in sorted({e for e in e0 if e < E})]


def row_list(E):
    """Row-tile and MFMA-block boundaries of the 16-, 32- and 128-row tilings."""
    return [(s, 40) for s in (1, 15, 16, 31, 32, 63, 64, 127, 128, IMPULSE_S - 2)]


def impulse_case(E, cells, seed=21):
    """One frame per (s0, e0), geometry of A at +-4 m; `ref` is hann(S)[s0] W[e0, t] exp(-2 pi j s s0 / S) with the product
    s s0 reduced modulo S in integers."""
    S, T, F = IMPULSE_S, IMPULSE_T, len(cells)
    Pi, Di = dyadic_geometry(F, E, T, SPANS["4 m"], seed)
    W = steering_exact(Pi, Di)
    X = np.zeros((F, S, E), dtype=np.complex64)
    ref = np.empty((F, S, T), dtype=np.complex128)
    for f, (s0, e0) in enumerate(cells):
        X[f, s0, e0] = 1.0
        ref[f] = np.hanning(S)[s0] * np.exp(-2j * np.pi * ((np.arange(S) * s0) % S) / S)[:, None] * W[f, e0][None, :]
    return dict(X=X, P=Pi * P_UNIT, dirs=Di * D_UNIT, lam=LAM_DYADIC, Pi=Pi, Di=Di, ref=ref)


# ------------------------------------------------------------------------------------------------------------ E: shapes
DEGENERATE = {"S = 1": (1, 37, 10), "S = 2": (2, 37, 10), "E = 1": (70, 1, 10), "T = 1": (70, 37, 1), "T = 5": (70, 37, 5)}
