"""Adversarial planes for the rounding-error bound of the float32 range-Doppler kernels, and its checker.

The inequality under test (rd_error_ulps in mmw_tu_input.hip, below range_doppler_impl), for every cell of every plane:

    |rd32[cell] - rd64[cell]|  <=  rd_error_ulps(S, C) * 2^-24 * l1(plane),     l1 = sum hann(S) hann(C) (|re| + |im|)

build_planes gives one input family per antenna plane, so one frame covers them all; reference is the oracle's complex128
spectrum and the float64 l1; check returns, per plane, the worst cell's share of the budget.  CASES lists the kernel families
test_gpu_rd_error_bound.py runs (test_rd_bound_cases_host.py walks the same list without a GPU).
"""
from collections import namedtuple

import numpy as np

from oracle import oracle_np as O

EPS = 2.0 ** -24


def _interior(n, want):
    """An index off the zero-weight Hann ends where the axis has an interior (n >= 3), else whatever exists."""
    return int(min(max(want, 1), n - 2)) if n >= 3 else int(min(max(want, 0), n - 1))


def _coherent(rng, S, C, ks, kc):
    """x[s, c] = m[s, c] exp(+2 pi i (ks s / S + kc c / C)), m > 0: every product of bin (ks, kc) adds in phase."""
    m = rng.uniform(0.5, 1.5, (S, C))
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    return m * np.exp(2j * np.pi * ((ks * s % S) / S + (kc * c % C) / C))


def _impulse(S, C, s, c, value):
    x = np.zeros((S, C), dtype=np.complex128)
    x[_interior(S, s), _interior(C, c)] = value
    return x


def _ones_mantissa(rng, shape):
    """+- floats whose 23 mantissa bits are all set, exponents 2^-3 .. 2^3 (the worst operand of a three-way bfloat16 split)."""
    bits = (rng.integers(0, 2, shape).astype(np.uint32) << 31) | (rng.integers(124, 131, shape).astype(np.uint32) << 23) | 0x7FFFFF
    return bits.astype(np.uint32).view(np.float32)


def coherent_bins(S, C):
    """(ks, kc) of the two coherent planes: an interior bin, and the last one (the highest twiddle powers)."""
    return ((S // 3, (2 * C) // 5), (S - 1, C - 1))


def build_planes(S, C, seed):
    """(names, cube [V, S, C] complex64): one adversarial family per antenna plane."""
    rng = np.random.default_rng(seed)
    (ks0, kc0), (ks1, kc1) = coherent_bins(S, C)
    dyn = np.exp2(rng.uniform(-12, 12, (S, C))) * np.exp(2j * np.pi * rng.uniform(0, 1, (S, C)))
    planes = [
        ("gauss", rng.standard_normal((S, C)) + 1j * rng.standard_normal((S, C))),
        ("coherent_interior", _coherent(rng, S, C, ks0, kc0)),
        ("coherent_last", _coherent(rng, S, C, ks1, kc1)),
        ("dc_fullscale", np.full((S, C), 32767 + 32767j)),
        ("impulse_lo", _impulse(S, C, 1, 1, 3 - 4j)),
        ("impulse_mid", _impulse(S, C, S // 2, C // 2, -1.5 + 0.25j)),
        ("impulse_hi", _impulse(S, C, S - 2, C - 2, 0.6 + 0.8j)),
        ("dynamic_range", dyn),
        ("ones_mantissa", _ones_mantissa(rng, (S, C)) + 1j * _ones_mantissa(rng, (S, C))),
        ("real_only", rng.standard_normal((S, C)) + 0j),
    ]
    names = [n for n, _ in planes]
    cube = np.stack([p for _, p in planes]).astype(np.complex64)
    return names, cube


def reference(cube):
    """(rd64 [V, S, C] complex128 of the oracle, l1_64 [V] float64 = sum hann(S) x hann(C) (|re| + |im|))."""
    V, S, C = cube.shape
    w = np.hanning(S)[:, None] * np.hanning(C)[None, :]
    x = cube.astype(np.complex128)
    l1 = np.array([np.sum(w * (np.abs(x[v].real) + np.abs(x[v].imag))) for v in range(V)], dtype=np.float64)
    return O.range_doppler(cube), l1


def check(rd32, rd64, l1, ulps):
    """Per plane: (worst ratio max_cell |rd32 - rd64| / (ulps 2^-24 l1), the (row, fftshifted Doppler column) of that cell)."""
    ratios, cells = [], []
    for v in range(rd64.shape[0]):
        err = np.abs(rd32[v].astype(np.complex128) - rd64[v])
        k = int(np.argmax(err))
        ratios.append(float(err.flat[k] / (float(ulps) * EPS * float(l1[v]))))
        cells.append(tuple(int(i) for i in np.unravel_index(k, err.shape)))
    return np.array(ratios), cells


# ------------------------------------------------------------------ the counting rule of rd_error_ulps, restated
def _prime_factors(n):
    out, p = [], 2
    while n > 1:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out


def structured_ulps(S, C):
    """Windows 8; per prime factor p of either axis one twiddle product (4) plus, for odd p, the real-symmetric DFT
    ((p + 7) / 2 + 1), 88 for the 127-point MFMA level."""
    def level(p):
        return 4 + (0 if p == 2 else 88 if p == 127 else (p + 7) // 2 + 1)
    return 8 + sum(level(p) for p in _prime_factors(S) + _prime_factors(C))


def generic_ulps(S, C):
    """Two-kernel path: windows 8; per axis radix-2 levels (4 each) for a power of two, an N-term direct sum (N + 4) otherwise."""
    def axis(n):
        return 4 * (n.bit_length() - 1) if n & (n - 1) == 0 else n + 4
    return 8 + axis(S) + axis(C)


# ------------------------------------------------------------------ the kernel families
# plan0: what mmw_diag_rd_plan(S, C, 0)[0] reports under default switches (it does not read the MMW_NO_*_RD switches: None
# where they are set); budget: which restatement plan[7] of mmw_diag_detect_plan must equal ("runtime": structured + the
# run-time plan's terms, checked as a lower bound from the plan's radices).
Case = namedtuple("Case", "family S C env options plan0 budget")
GENERIC_ENV = {"MMW_NO_FUSED_RD": "1", "MMW_NO_MIXED_RD": "1"}
CASES = (
    [Case("fused", 256, 128, {}, {}, 0, "structured")]
    # (every plane of this list also has a compile-time mixed-radix instantiation, which range_doppler_impl prefers; the
    #  plan entry names the class, and both kernels book the same structured budget)
    + [Case("lds_pow2", S, C, {}, {}, 1, "structured") for S, C in ((32, 32), (512, 32), (128, 128))]
    + [Case("mixed_ct", S, C, {}, {}, 2, "structured") for S, C in ((63, 100), (63, 115), (120, 126), (200, 40))]
    # (MMW_BIGPRIME_BF16 = 1 is a request: 127 x 32 stand-alone keeps the float32 MFMA form by design, mixct_use_bf)
    + [Case("p127_f32" if form == 0 else "p127_bf16", S, C, {}, {"MMW_BIGPRIME_BF16": form}, 2, "structured")
       for S, C in ((127, 32), (63, 127), (254, 50)) for form in (0, 1)]
    + [Case("mixed_runtime", S, C, {}, {}, 2, "runtime") for S, C in ((13, 11), (37, 41), (96, 23), (25, 49))]
    + [Case("split", S, C, {}, {}, 4, "structured") for S, C in ((512, 64), (256, 256), (1024, 32))]
    + [Case("generic_radix2", 256, 128, GENERIC_ENV, {}, None, "generic"),
       Case("generic_direct", 63, 70, dict(GENERIC_ENV, MMW_NO_SPLIT_RD="1"), {}, None, "generic")]
)
SCALE_CASES = [c for c in CASES if (c.family, c.S, c.C) in (("fused", 256, 128), ("p127_bf16", 63, 127), ("mixed_ct", 63, 100),
                                                             ("generic_direct", 63, 70))]
ENV_SWITCHES = ("MMW_NO_FUSED_RD", "MMW_NO_MIXED_RD", "MMW_NO_SPLIT_RD")


def case_id(c):
    return f"{c.family}-{c.S}x{c.C}"


def seed_of(S, C):
    return 4100 + 131 * S + C


_cache = {}


def planes_and_reference(S, C):
    """(names, cube, rd64, l1_64) of a plane shape: built once, shared by every test that needs it, never modified."""
    if (S, C) not in _cache:
        names, cube = build_planes(S, C, seed_of(S, C))
        rd64, l1 = reference(cube)
        for a in (cube, rd64, l1):
            a.setflags(write=False)
        _cache[(S, C)] = (names, cube, rd64, l1)
    return _cache[(S, C)]
