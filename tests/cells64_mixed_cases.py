"""Cases, the factor table and the a-priori error bound of k_cells64_mixed<C> (mmw_cells64_mixed.h), the dense float64 cell kernel of
the chirp counts other than 128.  No GPU needed.  Cubes, detection lists and oracle answers come from tests/refine_cases.py
(every evaluation is flagged by construction; the exclusion rule is Case.expected's).

FACTORS restates c64m_r2 of mmw_cells64_mixed.h: C -> (R1 points per lane, R2 lanes per row); tests/test_cells64_mixed_host.py
compares it with what mmw_diag_cells64_plan reports.
"""
import numpy as np

import refine_cases as rc

NT = 512                # threads of the workgroup
MUST_COVER = (8, 30, 32, 40, 50, 64, 70, 80, 100, 126)      # chirp counts of the shipped cfgs the kernel must serve
NOT_COVERED = (115, 127)                                     # 5 * 23 and a prime: the direct route
FACTORS = {8: (4, 2), 10: (5, 2), 15: (5, 3), 30: (10, 3), 32: (8, 4), 40: (8, 5), 50: (10, 5), 56: (8, 7), 64: (8, 8),
           70: (10, 7), 80: (10, 8), 100: (10, 10), 126: (9, 14), 128: (8, 16)}
LDS_MAX = 160 * 1024 - 512
KIND_NONE, KIND_128, KIND_MIXED = 0, 1, 2


def rows_per_pass(C):
    return (NT // FACTORS[C][1]) & ~7


def pitch(C):
    return (C + 1) | 1


def lds_bytes(S, C):
    return (rows_per_pass(C) * pitch(C) + S) * 16 + (S + C) * 8 + 256 * 8 + 64


# ---- the error bound --------------------------------------------------------------------------------------------------------
def _spf(n):
    d = 2
    while d * d <= n:
        if n % d == 0:
            return d
        d += 1
    return n


def gamma_regdft(R):
    """|error| <= gamma u L1(input) of RegDFT<R, double> (mmw_dft_small.h), every rounding lined up, following its construction:
      R = 1                 nothing                                                                     0
      R = 2                 one add                                                                     1
      R = 2^k               k radix-2 levels of (add 1 + twiddle product 4), as gamma_dense counts   5 k
      R an odd prime        s_j, d_j = x_j +- x_(R-j) (1); t = x_0 + sum_j c_jk s_j: literal 1 + product 1 per term and
                            H = (R - 1) / 2 sequential adds; t -+ j u (1)                            H + 4
      R = A B coprime       Good-Thomas, no twiddles                                   gamma(A) + gamma(B)
      R = p^m               Cooley-Tukey, one literal twiddle product (3 + 1)       gamma(p) + 4 + gamma(R / p)"""
    if R == 1:
        return 0
    if R == 2:
        return 1
    if R & (R - 1) == 0:
        return 5 * (R.bit_length() - 1)
    p = _spf(R)
    if p == R:
        return (R - 1) // 2 + 4
    A = 1
    n = R
    while n % p == 0:
        n //= p
        A *= p
    if n == 1:
        return gamma_regdft(p) + 4 + gamma_regdft(R // p)
    return gamma_regdft(A) + gamma_regdft(R // A)


def gamma_mixed(S, C):
    """|cell error| <= gamma 2^-53 L1w for k_cells64_mixed<C>, every rounding lined up (u = 2^-53; a complex product with a
    table entry: 3 u for the product + 1 u for the entry), in the kernel's order of operations:
      two window multiplies: hann(C)[c] * hann(S)[s] (2 entries + 1) and x * w (1)                          4
      first level, RegDFT<R1> over the lane's points                                             gamma_regdft(R1)
      one inter-level twiddle product W_C^(n1 k2)                                                           4
      second level, RegDFT<R2> over the row's lanes                                              gamma_regdft(R2)
      range twiddle: table entry 1 + up to min(RPL, 8) - 1 steps of c = cmul(c, W_S^(8 r)) at 4 (the
        recurrence restarts from the table every 8 rows of a lane)                     1 + 4 (min(RPL, 8) - 1)
      z * c inside the fused multiply-adds                                                                  2
      RPL = rows / 8 sequential fused multiply-adds per lane and pass, ceil(S / rows) passes   RPL ceil(S / rows)
      3 shuffle adds over the cell's eight lanes                                                            3"""
    R1, R2 = FACTORS[C]
    rows = rows_per_pass(C)
    rpl = rows // 8
    return 4 + gamma_regdft(R1) + 4 + gamma_regdft(R2) + 1 + 4 * (min(rpl, 8) - 1) + 2 + rpl * -(-S // rows) + 3


# ---- a float64 NumPy model of the kernel's operation order -------------------------------------------------------------------
def _regdft_model(x):
    """RegDFT along the last axis in complex128, built as mmw_dft_small.h builds it (natural order in and out)."""
    R = x.shape[-1]
    if R == 1:
        return x.copy()
    if R == 2:
        return np.stack([x[..., 0] + x[..., 1], x[..., 0] - x[..., 1]], axis=-1)
    if R & (R - 1) == 0:            # radix-2 decimation in frequency
        h = R // 2
        a, b = x[..., :h] + x[..., h:], (x[..., :h] - x[..., h:]) * np.exp(-2j * np.pi * np.arange(h) / R)
        out = np.empty_like(x)
        out[..., 0::2], out[..., 1::2] = _regdft_model(a), _regdft_model(b)
        return out
    p = _spf(R)
    if p == R:
        H = (R - 1) // 2
        j = np.arange(1, H + 1)
        s, d = x[..., j] + x[..., R - j], x[..., j] - x[..., R - j]
        out = np.empty_like(x)
        acc = x[..., 0].copy()
        for i in range(H):
            acc = acc + s[..., i]
        out[..., 0] = acc
        for k in range(1, H + 1):
            t, u = x[..., 0].copy(), np.zeros_like(x[..., 0])
            for i in range(H):
                t = t + s[..., i] * np.cos(2 * np.pi * ((j[i] * k) % R) / R)
                u = u + d[..., i] * np.sin(2 * np.pi * ((j[i] * k) % R) / R)
            out[..., k], out[..., R - k] = t - 1j * u, t + 1j * u
        return out
    A, n = 1, R
    while n % p == 0:
        n //= p
        A *= p
    out = np.empty_like(x)
    if n == 1:                      # Cooley-Tukey: n = Q n1 + n2, k = k1 + P k2
        P, Q = p, R // p
        y = _regdft_model(np.stack([x[..., Q * np.arange(P) + n2] for n2 in range(Q)], axis=-2))       # [..., n2, k1]
        y = y * np.exp(-2j * np.pi * np.outer(np.arange(Q), np.arange(P)) / R)
        z = _regdft_model(np.swapaxes(y, -1, -2))                                                          # [..., k1, k2]
        for k1 in range(P):
            out[..., k1 + P * np.arange(Q)] = z[..., k1, :]
        return out
    B = R // A                      # Good-Thomas: n = (B n1 + A n2) mod R, k = (k1 EA + k2 EB) mod R
    inv = lambda a, m: next(v for v in range(1, m + 1) if (a * v) % m == 1 % m)       # noqa: E731
    EA, EB = B * inv(B % A, A), A * inv(A % B, B)
    y = _regdft_model(np.stack([x[..., (B * np.arange(A) + A * n2) % R] for n2 in range(B)], axis=-2))   # [..., n2, k1]
    z = _regdft_model(np.swapaxes(y, -1, -2))                                                              # [..., k1, k2]
    for k1 in range(A):
        out[..., (k1 * EA + np.arange(B) * EB) % R] = z[..., k1, :]
    return out


def model_cells(plane, cells):
    """The cells (r, fftshifted d) of one complex64 plane [S][C] in float64 arithmetic, level by level as the kernel works:
    window products, RegDFT<R1> over n2 (c = n1 + R2 n2), W_C^(n1 k2), RegDFT<R2> over n1 (k = k2 + R1 k1), then per cell
    eight partial range sums over rows q + 8 t of every pass with the W_S^(8 r) recurrence restarted every 8 steps, added as
    the xor-shuffle tree adds them."""
    S, C = plane.shape
    R1, R2 = FACTORS[C]
    rows = rows_per_pass(C)
    ws, wc = np.hanning(S), np.hanning(C)
    x = plane.astype(np.complex128) * (wc[None, :] * ws[:, None])
    x = x.reshape(S, R1, R2).transpose(0, 2, 1)                        # [s][n1][n2]
    x1 = _regdft_model(x)                                              # [s][n1][k2]
    tw = np.exp(-2j * np.pi * np.outer(np.arange(R2), np.arange(R1)) / C)
    x2 = _regdft_model(np.swapaxes(x1 * tw[None], 1, 2))               # [s][k2][k1]
    Z = x2.transpose(0, 2, 1).reshape(S, C)                            # bin k = k2 + R1 k1
    twS = np.exp(-2j * np.pi * np.arange(S) / S)
    out = np.zeros(len(cells), dtype=np.complex128)
    for i, (r, d) in enumerate(cells):
        r, k = int(r), (int(d) - C // 2) % C
        step = twS[(8 * r) % S]
        part = np.zeros(8, dtype=np.complex128)
        for s0 in range(0, S, rows):
            for q in range(8):
                for t in range(rows // 8):
                    s = s0 + q + 8 * t
                    if t % 8 == 0:
                        if s >= S:
                            break
                        c = twS[(r * s) % S]
                    if s < S:
                        part[q] = part[q] + Z[s, k] * c
                    c = c * step
        for dd in (1, 2, 4):
            part = part + part[np.arange(8) ^ dd]
        out[i] = part[0]
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# value level (mmw_rd_cells64_at, route MMW_CELLS64_DENSE_MIXED): tiny planes of the test-only instantiations (10, 15 odd, 56),
# shipped chirp counts, 254 x 50 (50 = 10 x 5 gives 96 rows per pass: THREE passes of 96, 96 and 62 rows; it would be four
# with the 64 rows per pass of the 128-point kernel), 150 x 100 (48 rows per pass: FOUR passes, the last of 6 rows), 7 x 126 (fewer rows than one lane group;
# 14 lanes per row, 9 of them with a second-level transform),
# 63 x 128 (beside k_cells64<128>).  290 listed detections in frame 0: a second chunk of cells.
VALUE_PLANES = ((8, 10), (16, 15), (20, 56), (64, 30), (63, 100), (100, 70), (254, 50), (7, 126), (63, 128), (150, 100))
UNSUPPORTED_PLANES = ((16, 320), (8, 11))
INDEX_PLANES = ((63, 100), (16, 15))
# name -> (seed offset, F, V, cap, counts, layout): the layouts of refine_cases with the chunk border of this kernel (256 cells)
LAYOUTS = {
    "corners": (0, 2, 4, 16, [12, 9], "corners"),
    "duplicates": (7, 2, 4, 16, [11, 16], "duplicates"),
    "n256": (14, 2, 4, 256, [256, 10], "random"),
    "n257": (21, 2, 4, 264, [257, 10], "corners"),
    "tail": (42, 2, 4, 1024, [600, 300], "random"),                # 900 > dense_cap = 512: the direct kernels take the rest
    "overcap": (49, 2, 4, 48, [48 + 7, 20], "corners"),
    "alternating": (56, 4, 4, 32, [24, 0, 24, 0], "random"),
}
_SEED0 = {(63, 100): 7100, (16, 15): 7300}

_SPECS = {}
for _S, _C in VALUE_PLANES:
    _SPECS[f"value_{_S}x{_C}"] = (8000 + 17 * _S + _C, (2, 4, _S, _C), 300, [290, 12], "corners")
for _S, _C in UNSUPPORTED_PLANES:
    _SPECS[f"unsupported_{_S}x{_C}"] = (8500 + _S + _C, (2, 4, _S, _C), 24, [20, 5], "corners")
for _S, _C in INDEX_PLANES:
    for _n, (_off, _F, _V, _cap, _cnt, _lay) in LAYOUTS.items():
        _SPECS[f"{_n}_{_S}x{_C}"] = (_SEED0[(_S, _C)] + _off, (_F, _V, _S, _C), _cap, _cnt, _lay)
_SPECS["zero_2x10"] = (9000, (3, 4, 2, 10), 24, [10, 0, 5], "corners")        # np.hanning(2) = [0, 0]
NAMES = tuple(_SPECS)

_cases = {}


def case(name):
    if name not in _cases:
        seed, shape, cap, counts, layout = _SPECS[name]
        _cases[name] = rc.Case(name, seed, shape, cap, counts, layout)
    return _cases[name]
