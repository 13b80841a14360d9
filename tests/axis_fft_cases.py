"""Cases, inputs, references, budget and checker for the any-shape axis FFT (csrc/mmw_fft_generic.h, launch_fft_axis).

launch_fft_axis is the fallback under every FFT entry point: k_fft_strided / k_fft_contig for the 8 radix lengths, k_dft_direct
for every other length up to 4096.  expected_kernel restates its choice (radix, tile, quarter tile, the direct DFT's tile) as a
pure function; every GPU case of test_gpu_axis_fft.py asserts the branch it claims from it, and test_axis_fft_cases_host.py
checks it against a table of the header's constants, so a change of the dispatcher shows up without a GPU.

Inputs: one family per inner column (build_columns), the families of rd_bound_cases.build_planes restricted to one axis, every
second column an impulse at a position that walks the input axis with a value of its own -- every input index and every output
twiddle is pinned by some column.  The two-axis entries take a plane whose columns are those families (frame 0) and a plane of
impulse columns (frame 1).

References: numpy complex128 for float32 outputs; for float64 outputs a direct DFT in np.longdouble with integer (n k) mod N
twiddle indices, added as a tree over runs of 32 terms (dft_longdouble; checked against mpmath by the host test).

Budget (the project's counting rule, rd_error_ulps in csrc/mmw_tu_input.hip; not tuned to the kernels), per output cell:

    |got - ref| <= ulps * eps * l1,   l1 = sum of the windowed |re| + |im| along the transformed axes,
    eps = 2^-24 (float32 output) or 2^-53 (float64 output),
    ulps = 4 per window or scale product actually made           (WINDOW_ULPS)
         + per axis 4 log2 N (radix length) or n_in + 4 (direct sum)   (axis_ulps)
         + 4 for a hypot magnitude output (OpenCL's bound, which the device library is built to)    (HYPOT_ULPS)
         + V + 1 for the mean over V antennas of the range profiles (V - 1 additions, the division, and the V magnitudes'
           own error is the hypot term), with l1 averaged over V.
"""
from collections import namedtuple

import numpy as np

import rd_bound_cases as rb

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
WINDOW_ULPS, HYPOT_ULPS = 4, 4
NOMINAL_CU = 256                    # the MI355X; the GPU tests use the device's own count
MAX_DIRECT = 4096
# N -> (R1, R2): the switch of launch_fft_axis
RADIX = {8: (4, 2), 16: (4, 4), 32: (8, 4), 64: (8, 8), 128: (16, 8), 256: (16, 16), 512: (32, 16), 1024: (32, 32)}
F32, F64 = 4, 8                     # sizeof(T)
MAGNITUDE, NO_WINDOW, NO_SHIFT = 1, 2, 4        # the MMW_ANGLE_* flags


# ------------------------------------------------------------------ the dispatcher, restated
def strided_tile(N, elem_bytes):
    return min(32, max(1, 65536 // (N * elem_bytes)))


def contig_tile(R1, R2, elem_bytes):
    return max(1, min(256 // R2, 49152 // (R1 * (R2 + 1) * elem_bytes)))


Kernel = namedtuple("Kernel", "kind N B quarter lds threads blocks")


def expected_kernel(N, contiguous, t_bytes, tin_bytes, inner, outer, n_in, num_cu):
    """What launch_fft_axis<T, TIN>(N, contiguous) launches: kind 'strided' | 'contig' | 'direct', its tile B (columns or rows
    per workgroup), whether that is the quarter tile, dynamic LDS bytes, threads and workgroups.  None beyond 4096."""
    elem = 2 * t_bytes
    if N in RADIX:
        R1, R2 = RADIX[N]
        if contiguous:
            B = contig_tile(R1, R2, elem)
            return Kernel("contig", N, B, False, B * R1 * (R2 + 1) * elem, B * R2, -(-outer // B))
        B, quarter = strided_tile(N, elem), False
        if B >= 16 and t_bytes == 4 and tin_bytes == 4:
            tiles = -(-inner // B)
            if tiles * outer * 2 <= num_cu and inner > B // 4:
                B, quarter = B // 4, True
        return Kernel("strided", N, B, quarter, N * B * elem, B * R2, -(-inner // B) * outer)
    if N > MAX_DIRECT:
        return None
    if contiguous:          # rows become the inner index
        inner, outer = outer, 1
    B = 16
    while B > 1 and n_in * B * elem > 48 * 1024:
        B //= 2
    return Kernel("direct", N, B, False, max(n_in, 1) * B * elem, 256, -(-inner // B) * outer)


def axis_ulps(N, n_in):
    return 4 * (N.bit_length() - 1) if N in RADIX else n_in + 4


# ------------------------------------------------------------------ inputs
FAMILIES = ("gauss", "coherent_interior", "coherent_last", "dc_fullscale", "dynamic_range", "ones_mantissa", "real_only")


def column_kinds(ncols, rot=0):
    """Even columns walk the named families (from family `rot` on), odd columns are impulses."""
    return ["impulse" if i % 2 else FAMILIES[(i // 2 + rot) % len(FAMILIES)] for i in range(ncols)]


def impulse_position(i, n_in, windowed):
    """Input index of impulse column i: (i // 2) walks the axis -- off the zero-weight ends of np.hanning where a window is on and
    the axis has an interior."""
    lo, span = (1, n_in - 2) if windowed and n_in >= 3 else (0, n_in)
    return lo + (i // 2) % span


def impulse_value(i):
    return (1 + (i % 7) / 8) * np.exp(1j * (0.7 + 2.399963 * i))


def build_columns(n_in, N, ncols, seed, windowed, rot=0):
    """(kinds, x [n_in, ncols] complex64): column i of family kinds[i]; coherent columns add in phase at bin N // 3 / N - 1 of an
    N-point transform."""
    rng = np.random.default_rng(seed)
    kinds = column_kinds(ncols, rot)
    n = np.arange(n_in)
    x = np.zeros((n_in, ncols), dtype=np.complex128)
    for i, kind in enumerate(kinds):
        if kind == "impulse":
            x[impulse_position(i, n_in, windowed), i] = impulse_value(i)
        elif kind == "gauss":
            x[:, i] = rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)
        elif kind in ("coherent_interior", "coherent_last"):
            k = N // 3 if kind == "coherent_interior" else N - 1
            x[:, i] = rng.uniform(0.5, 1.5, n_in) * np.exp(2j * np.pi * ((k * n) % N) / N)
        elif kind == "dc_fullscale":
            x[:, i] = 32767 + 32767j
        elif kind == "dynamic_range":
            x[:, i] = np.exp2(rng.uniform(-12, 12, n_in)) * np.exp(2j * np.pi * rng.uniform(0, 1, n_in))
        elif kind == "ones_mantissa":
            x[:, i] = rb._ones_mantissa(rng, (n_in,)) + 1j * rb._ones_mantissa(rng, (n_in,))
        else:
            x[:, i] = rng.standard_normal(n_in)
    return kinds, x.astype(np.complex64)


def hann(n):
    return np.hanning(n)            # hanning(1) = [1], hanning(2) = [0, 0]


def abs1(x):
    return np.abs(x.real) + np.abs(x.imag)


# ------------------------------------------------------------------ references
def longdouble_pi():
    return 4 * np.arctan(np.longdouble(1))


_tw_cache = {}


def twiddles_longdouble(N):
    """W_N^m, m = 0 .. N - 1, in np.clongdouble."""
    if N not in _tw_cache:
        # m / N = q / 4 + r / (4 N) with integers q and |r| <= N / 2: the quarter turns are exact, the rest is an angle within
        # pi / 4, whose rounding (and so the twiddle's error) stays near 2^-64
        m = np.arange(N, dtype=np.int64)
        q = (8 * m + N) // (2 * N)
        phi = (longdouble_pi() / 2) * (4 * m - q * N).astype(np.longdouble) / np.longdouble(N)
        base = (np.cos(phi) - 1j * np.sin(phi)).astype(np.clongdouble)
        _tw_cache[N] = np.choose(q % 4, [base, base.imag - 1j * base.real, -base, -base.imag + 1j * base.real])
    return _tw_cache[N]


def dft_longdouble(x, N):
    """X[k, ...] = sum_n x[n, ...] W_N^((n k) mod N) along axis 0 of x [n_in, ...] (n_in <= N: zero padding), np.clongdouble; runs
    of 32 terms added as a tree, so the rounding error grows with log n_in and not with n_in."""
    x = np.asarray(x, dtype=np.clongdouble)
    n_in, tw = x.shape[0], twiddles_longdouble(N)
    flat = x.reshape(n_in, -1)
    out = np.zeros((N, flat.shape[1]), dtype=np.clongdouble)
    if n_in == 0:
        return out.reshape((N,) + x.shape[1:])

    def tree(kk, n0, n1):
        if n1 - n0 <= 32:
            return tw[(kk[:, None] * np.arange(n0, n1)[None, :]) % N] @ flat[n0:n1]
        mid = (n0 + n1) // 2
        return tree(kk, n0, mid) + tree(kk, mid, n1)

    for k0 in range(0, N, 512):
        kk = np.arange(k0, min(N, k0 + 512), dtype=np.int64)
        out[kk] = tree(kk, 0, n_in)
    return out.reshape((N,) + x.shape[1:])


def transform(x, N, axis, shift, wide):
    """The reference transform of x along `axis`, zero-padded to N, np.fft.fftshift over that axis when shift (odd N too)."""
    x = np.moveaxis(x, axis, 0)
    X = dft_longdouble(x, N) if wide else np.fft.fft(np.asarray(x, dtype=np.complex128), n=N, axis=0)
    if shift:
        X = np.roll(X, N // 2, axis=0)
    return np.moveaxis(X, 0, axis)


def worst(got, ref, l1, ulps, eps):
    """(worst share of the budget over the cells, index of that cell); l1 broadcasts against the cells.  Where l1 == 0 (an all-zero
    windowed input) the output must be exactly zero: such a cell counts 0 when it is, inf when it is not."""
    err = np.abs(np.asarray(got).astype(ref.dtype) - ref).astype(np.float64)
    bud = np.broadcast_to(float(ulps) * eps * np.asarray(l1, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bud > 0, err / bud, np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(r))
    return float(r.flat[k]), tuple(int(i) for i in np.unravel_index(k, r.shape))


_cache = {}


def cached(key, make):
    """Inputs and references are built once, shared by the tests that need them and never modified."""
    if key not in _cache:
        val = make()
        for a in val:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = val
    return _cache[key]


# ------------------------------------------------------------------ mmw_angle_fft (and the angle stage of mmw_chain3d)
AngleCase = namedtuple("AngleCase", "name A V F S C flags kind B quarter")


def _angle(name, A, V, F, S, C, flags=0):
    k = expected_kernel(A, False, F32, F32, S * C, F, V, NOMINAL_CU)
    return AngleCase(name, A, V, F, S, C, flags, k.kind, k.B, k.quarter)


def _wide_bins(A):
    return 27 * strided_tile(A, 8) + 5              # 28 tiles x 5 frames x 2 > 256 compute units, a ragged last tile


ANGLE_CASES = (
    # V = 5: A = 64 goes generic too.  narrow: 2 frames x 21 bins (odd, no multiple of a tile; the quarter tile where it exists)
    [_angle(f"narrow-A{A}", A, 5, 2, 3, 7) for A in RADIX]
    + [_angle(f"wide-A{A}", A, 5, 5, _wide_bins(A), 1) for A in RADIX]
    # inner == B / 4 keeps the full tile, inner == B / 4 + 1 takes the quarter tile (B = 32 at A = 32, B = 16 at A = 512)
    + [_angle(f"edge-A{A}-bins{bins}", A, 5, 2, 1, bins) for A, bins in ((32, 8), (32, 9), (512, 4), (512, 5))]
    # lengths outside the switch: k_dft_direct (A = 1, 2, 4 fall through it as well)
    + [_angle(f"direct-A{A}-V{V}", A, V, 2, 3, 7) for A, V in ((1, 1), (2, 1), (2, 2), (4, 3), (4, 4), (5, 5), (7, 5), (100, 5), (181, 5))]
    + [_angle(f"flags{fl}-A{A}", A, 5, 2, 3, 7, fl) for A in (32, 7) for fl in range(1, 8)]
)
# the same lengths through mmw_chain3d(d_rd kept): V = 4, A != 64 (the chunked serial route into angle_fft_impl)
CHAIN_V, CHAIN_S, CHAIN_C, CHAIN_F = 4, 8, 16, 2
CHAIN_A = [A for A in RADIX if A != 64] + [4, 5, 7, 100, 181]


def angle_ulps(c):
    return (0 if c.flags & NO_WINDOW else WINDOW_ULPS) + axis_ulps(c.A, c.V) + (HYPOT_ULPS if c.flags & MAGNITUDE else 0)


def angle_reference(rd, A, flags):
    """(ref [F, A, bins] complex128, l1 [F, 1, bins]) of rd [F, V, bins]."""
    V = rd.shape[1]
    w = np.ones(V) if flags & NO_WINDOW else hann(V)
    x = rd.astype(np.complex128) * w[None, :, None]
    return transform(x, A, 1, not flags & NO_SHIFT, False), abs1(x).sum(axis=1, keepdims=True)


def angle_data(c):
    """(kinds, rd [F, V, bins] complex64, ref, l1) of an angle case; the flag cases share the input of their window setting."""
    windowed = not c.flags & NO_WINDOW
    bins = c.S * c.C

    def make():
        kinds, x = build_columns(c.V, c.A, c.F * bins, 7000 + 17 * c.A + c.V + bins, windowed)
        return kinds, np.ascontiguousarray(x.reshape(c.V, c.F, bins).transpose(1, 0, 2))

    kinds, rd = cached(("angle_in", c.A, c.V, c.F, bins, windowed), make)
    ref, l1 = cached(("angle_ref", c.A, c.V, c.F, bins, c.flags & 6), lambda: angle_reference(rd, c.A, c.flags))
    return kinds, rd, ref, l1


# ------------------------------------------------------------------ mmw_range_angle
RangeAngleCase = namedtuple("RangeAngleCase", "name A S V rx window chirp")
RA_V, RA_C, RA_F = 6, 3, 2


def _rx_list(kind, A, i):
    """None: all antennas; 'neg': a negative and a repeated index; 'full': n_rx == A.  Every list holds antennas 1, 3 and 4."""
    if kind == "none":
        return None
    if kind == "neg":
        return (-2, 1, 3, 3, 0)
    base = [1, 3, 4, -1, 0, 2, 3, 5]
    return tuple((base * (A // 8 + 1))[:A]) if A >= 8 else None


RANGE_ANGLE_CASES = []
for _i, (_A, _S) in enumerate((A, S) for A in (8, 33, 48, 64, 128) for S in (16, 63, 100, 256)):
    _kind = ("none", "neg", "full")[_i % 3]
    RANGE_ANGLE_CASES.append(RangeAngleCase(f"A{_A}-S{_S}-rx_{_kind}-win{(_i // 3) % 2}-chirp{(-1, 1, -3)[_i % 3]}", _A, _S, RA_V,
                                            _rx_list(_kind, _A, _i), (_i // 3) % 2, (-1, 1, -3)[_i % 3]))


def range_angle_ulps(c):
    n_sel = len(c.rx) if c.rx else c.V
    return (2 * WINDOW_ULPS if c.window else 0) + axis_ulps(c.S, c.S) + axis_ulps(c.A, n_sel) + HYPOT_ULPS


def range_angle_data(c):
    """(cubes [F, V, S, C] complex64, ref [F, S, A] float64 = |.|, l1 [F, 1, 1]).  Frame 0: one family per sample-axis column
    (the columns are the antennas); frame 1: impulses; the chirps that are not asked for hold other data."""
    def make():
        chirp = c.chirp % RA_C
        cubes = np.zeros((RA_F, c.V, c.S, RA_C), dtype=np.complex64)
        for ch in range(RA_C):
            _, a = build_columns(c.S, c.S, c.V, 8100 + 7 * c.S + ch, bool(c.window), rot=ch)
            cubes[0, :, :, ch] = a.T
            cubes[1, :, :, ch] = rb.build_planes(c.V, c.S, 8200 + c.S + ch)[1][4 + (ch + c.S) % 3]        # an impulse plane
        rx = [r % c.V for r in (c.rx if c.rx else range(c.V))]
        x = cubes[..., chirp][:, rx].astype(np.complex128)                  # [F, n_sel, S]
        if c.window:
            x = x * hann(c.V)[rx][None, :, None] * hann(c.S)[None, None, :]
        X = transform(transform(x, c.S, 2, False, False), c.A, 1, True, False)      # [F, A, S]
        return cubes, np.abs(X).transpose(0, 2, 1).copy(), abs1(x).sum(axis=(1, 2)).reshape(-1, 1, 1)

    return cached(("ra", c), make)


# ------------------------------------------------------------------ mmw_range_profile / mmw_range_profile_f64
RP_V, RP_F, RP_C, RP_CHIRP = 2, 2, 3, -2
RP_RADIX = tuple(RADIX)
RP_DIRECT = {F32: (385, 769, 1537, 3073, 4096), F64: (193, 385, 769, 1537, 3073, 4096)}      # the direct DFT's B: 8, 4, 2, 1, 1
RP_CASES = [(t, S) for t in (F32, F64) for S in RP_RADIX + RP_DIRECT[t]]
RP_REFUSED = 4097


def range_profile_ulps(S):
    return WINDOW_ULPS + axis_ulps(S, S) + HYPOT_ULPS + RP_V + 1


def range_profile_data(S, wide):
    """(cubes [F, V, S, C] complex64, ref [F, S], l1 [F, 1] averaged over V): the (frame, antenna) pairs are the columns."""
    def make():
        cubes = np.zeros((RP_F, RP_V, S, RP_C), dtype=np.complex64)
        for ch in range(RP_C):
            _, a = build_columns(S, S, RP_F * RP_V, 9100 + S + ch, True, rot=(S + ch) % len(FAMILIES))
            cubes[:, :, :, ch] = a.T.reshape(RP_F, RP_V, S)
        return (cubes,)

    (cubes,) = cached(("rp_in", S), make)

    def ref():
        x = cubes[:, :, :, RP_CHIRP].astype(np.clongdouble if wide else np.complex128) * hann(S).astype(np.longdouble if wide else np.float64)
        X = transform(x, S, 2, False, wide)
        return np.abs(X).mean(axis=1), abs1(x).sum(axis=2).mean(axis=1).astype(np.float64).reshape(-1, 1)

    return (cubes,) + cached(("rp_ref", S, wide), ref)


# ------------------------------------------------------------------ mmw_range_doppler_mag64, the float64 two-pass route
MAG64_V, MAG64_RX, MAG64_F = 3, 2, 2
MAG64_SHAPES = [(8, 512), (4, 1024), (1024, 4), (512, 64), (256, 256), (1024, 32), (300, 100), (100, 300), (16, 70), (63, 64),
                # small power-of-two planes for the contiguous lengths the list above leaves out (8, 16, 128)
                (32, 8), (32, 16), (32, 128)]
# planes the LDS-resident float64 kernel would take: the two-pass route is reached with MMW_NO_MIXED_RD = 1 (both the entry and
# mmw_diag_rd_plan(.., float64 = 1) read it)
MAG64_NEEDS_SWITCH = {(16, 70), (63, 64)}


def mag64_ulps(S, C):
    return 2 * WINDOW_ULPS + axis_ulps(S, S) + axis_ulps(C, C) + HYPOT_ULPS


def rd_plane_pair(S, C, seed):
    """[2, S, C] complex64: frame 0 one family per column, frame 1 an impulse in every column."""
    _, a = build_columns(S, S, C, seed, True)
    b = np.zeros((S, C), dtype=np.complex64)
    for i in range(C):
        b[impulse_position(2 * i, S, True), i] = impulse_value(i)
    return np.stack([a, b])


def mag64_data(S, C):
    """(cubes [F, V, S, C] complex64, ref [F, S, C] longdouble |RD| of antenna MAG64_RX, l1 [F, 1, 1])."""
    def make():
        cubes = np.stack([rd_plane_pair(S, C, 9500 + 131 * S + C + v) for v in range(MAG64_V)], axis=1)
        x = cubes[:, MAG64_RX].astype(np.clongdouble) * (hann(S)[:, None] * hann(C)[None, :]).astype(np.longdouble)
        X = transform(transform(x, S, 1, False, True), C, 2, True, True)
        return cubes, np.abs(X), abs1(x).sum(axis=(1, 2)).astype(np.float64).reshape(-1, 1, 1)

    return cached(("mag64", S, C), make)


def mag64_kernels(S, C, F, num_cu):
    return (expected_kernel(S, False, F64, F32, C, F, S, num_cu), expected_kernel(C, True, F64, F64, 1, F * S, C, num_cu))


# ------------------------------------------------------------------ mmw_range_doppler, float32, the generic pair (in place)
RD32_ENV = dict(rb.GENERIC_ENV, MMW_NO_SPLIT_RD="1")
# (V, S, C): V = 3 where the rows must not fill the contiguous tile; 10 = every plane of rd_bound_cases.build_planes
RD32_SHAPES = [(3, 8, 64), (3, 16, 32), (10, 16, 70), (10, 63, 64), (10, 1024, 8),
               # the contiguous lengths the list above leaves out
               (3, 8, 16), (3, 8, 128), (3, 8, 256), (3, 8, 512), (3, 8, 1024)]
RD32_SUBSETS = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 0, 4))        # planes of build_planes per call of a V = 3 case


def rd32_kernels(V, S, C, num_cu):
    return (expected_kernel(S, False, F32, F32, C, V, S, num_cu), expected_kernel(C, True, F32, F32, 1, V * S, C, num_cu))


# ------------------------------------------------------------------ what the case list reaches
def launches(num_cu=NOMINAL_CU):
    """Every launch of the case list as (entry, T bytes, TIN bytes, Kernel)."""
    out = []
    for c in ANGLE_CASES:
        out.append(("angle", F32, F32, expected_kernel(c.A, False, F32, F32, c.S * c.C, c.F, c.V, num_cu)))
    for A in CHAIN_A:
        out.append(("chain", F32, F32, expected_kernel(A, False, F32, F32, CHAIN_S * CHAIN_C, CHAIN_F, CHAIN_V, num_cu)))
    for c in RANGE_ANGLE_CASES:
        n_sel = len(c.rx) if c.rx else c.V
        out.append(("range_angle", F32, F32, expected_kernel(c.S, False, F32, F32, 1, RA_F, c.S, num_cu)))
        out.append(("range_angle", F32, F32, expected_kernel(c.A, False, F32, F32, c.S, RA_F, n_sel, num_cu)))
    for t, S in RP_CASES:
        out.append(("range_profile", t, F32, expected_kernel(S, False, t, F32, 1, RP_F * RP_V, S, num_cu)))
    for S, C in MAG64_SHAPES:
        a, b = mag64_kernels(S, C, MAG64_F, num_cu)
        out += [("mag64", F64, F32, a), ("mag64", F64, F64, b)]
    for V, S, C in RD32_SHAPES:
        a, b = rd32_kernels(V, S, C, num_cu)
        out += [("rd32", F32, F32, a), ("rd32", F32, F32, b)]
    return out


# (T, TIN, layout) triples some entry point dispatches; launch_fft_axis is instantiated for <double, float> and <double, double>
# in both layouts, but no caller sends float32 input to the contiguous float64 kernel or float64 input to the strided one
REACHABLE = {(F32, F32, "strided"), (F32, F32, "contig"), (F64, F32, "strided"), (F64, F64, "contig")}


def buffer_bytes():
    """The largest device buffer of every case family (inputs and outputs), for the host test's 64 MiB cap."""
    out = {}
    for c in ANGLE_CASES:
        out[f"angle {c.name}"] = c.F * c.A * c.S * c.C * 8
    for A in CHAIN_A:
        out[f"chain A{A}"] = CHAIN_F * A * CHAIN_S * CHAIN_C * 8
    for c in RANGE_ANGLE_CASES:
        out[f"range_angle {c.name}"] = max(RA_F * c.V * c.S * RA_C * 8, RA_F * c.S * c.A * 4)
    for t, S in RP_CASES:
        out[f"range_profile {t} {S}"] = RP_F * RP_V * S * RP_C * 8
    for S, C in MAG64_SHAPES:
        out[f"mag64 {S}x{C}"] = MAG64_F * MAG64_V * S * C * 8
    for V, S, C in RD32_SHAPES:
        out[f"rd32 {S}x{C}"] = V * S * C * 8
    return out
