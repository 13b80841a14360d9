"""tests/axis_fft_cases.py without a GPU: its references against mpmath, its inputs, its restatement of launch_fft_axis against
the header's constants, and what the case list of test_gpu_axis_fft.py reaches."""
import ctypes
import os

import mpmath
import numpy as np
import pytest

import axis_fft_cases as ac
import rd_bound_cases as rb
from mmwave_radar_processing_amd import _lib

HEADER = os.path.join(os.path.dirname(_lib.LIB_PATH), "mmw_fft_generic.h")


def mpf_of(v):
    """A np.longdouble as an mpf, exactly: its float64 head plus the remainder."""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("N,n_in", [(8, 8), (64, 5), (100, 100), (181, 5), (300, 300), (512, 512), (1024, 1024), (1537, 1537), (4096, 4096)])
def test_longdouble_dft_against_mpmath(N, n_in):
    """A handful of cells per length (first, last, one interior bin; the coherent column's own bin) to 2^-61 of l1: a single
    long double twiddle is good to about 2^-63 (its angle and its cosine / sine each round once), which an impulse column shows
    undiminished."""
    kinds, x = ac.build_columns(n_in, N, 6, 40 + N, False)
    X = ac.dft_longdouble(x, N)
    assert X.dtype == np.clongdouble and X.shape == (N, 6)
    mpmath.mp.prec = 200
    for col in (0, 2, 3):                # gauss, coherent_interior, impulse
        xs = [mpmath.mpc(float(v.real), float(v.imag)) for v in x[:, col]]
        l1 = float(ac.abs1(x[:, col].astype(np.complex128)).sum())
        for k in sorted({0, 1 % N, N // 3, N - 1}):
            want = mpmath.fsum(xs[n] * mpmath.expjpi(mpmath.mpf(-2 * ((n * k) % N)) / N) for n in range(n_in))
            got = mpmath.mpc(mpf_of(X[k, col].real), mpf_of(X[k, col].imag))
            assert abs(got - want) <= 2.0 ** -61 * l1, (N, kinds[col], k, float(abs(got - want)) / l1)


def test_complex128_transform_is_numpy_fft_with_fftshift():
    rng = np.random.default_rng(3)
    for N, n_in in ((7, 5), (33, 33), (64, 12)):
        x = rng.standard_normal((3, n_in, 4)) + 1j * rng.standard_normal((3, n_in, 4))
        want = np.fft.fftshift(np.fft.fft(x, n=N, axis=1), axes=1)
        assert np.array_equal(ac.transform(x, N, 1, True, False), want)
        wide = ac.transform(x, N, 1, True, True)
        assert np.max(np.abs(wide.astype(np.complex128) - want)) <= 1e-13 * np.abs(want).max()


def test_every_reference_has_a_scale_or_is_all_zero():
    """l1 > 0 for every column / plane, except the columns of the V = 2 angle case with the window on (np.hanning(2) = [0, 0]),
    whose reference is exactly zero."""
    for c in ac.ANGLE_CASES:
        kinds, rd, ref, l1 = ac.angle_data(c)
        assert rd.shape == (c.F, c.V, c.S * c.C) and ref.shape == (c.F, c.A, c.S * c.C) and np.isfinite(ref).all()
        if c.V == 2 and not c.flags & ac.NO_WINDOW:
            assert not l1.any() and not ref.any(), c.name
        else:
            assert (l1 > 0).all(), c.name
        assert "impulse" in kinds and (c.F * c.S * c.C < 14 or set(ac.FAMILIES) <= set(kinds)), c.name
    for c in ac.RANGE_ANGLE_CASES:
        cubes, ref, l1 = ac.range_angle_data(c)
        assert ref.shape == (ac.RA_F, c.S, c.A) and (l1 > 0).all() and np.isfinite(ref).all(), c.name
    for S in ac.RP_RADIX + (385, 769):
        cubes, ref, l1 = ac.range_profile_data(S, False)
        assert ref.shape == (ac.RP_F, S) and (l1 > 0).all()
    for S, C in ((8, 512), (16, 70), (32, 8)):
        cubes, ref, l1 = ac.mag64_data(S, C)
        assert ref.shape == (ac.MAG64_F, S, C) and ref.dtype == np.longdouble and (l1 > 0).all()


def test_impulse_columns_pin_every_input_index():
    for n_in, windowed in ((5, True), (5, False), (12, True), (1, True), (2, True)):
        kinds, x = ac.build_columns(n_in, 32, 2 * n_in + 2, 5, windowed)
        cols = [i for i, k in enumerate(kinds) if k == "impulse"]
        hit = {int(np.flatnonzero(x[:, i])[0]) for i in cols}
        assert all(np.count_nonzero(x[:, i]) == 1 for i in cols)
        assert hit == (set(range(1, n_in - 1)) if windowed and n_in >= 3 else set(range(n_in)))
        assert len({complex(x[:, i].sum()) for i in cols}) == len(cols)


# strided_tile / contig_tile of mmw_fft_generic.h, written out: N -> (float32 strided, float32 contig, float64 strided, float64 contig)
TILES = {8: (32, 128, 32, 128), 16: (32, 64, 32, 64), 32: (32, 64, 32, 64), 64: (32, 32, 32, 32), 128: (32, 32, 32, 21),
         256: (32, 16, 16, 11), 512: (16, 11, 8, 5), 1024: (8, 5, 4, 2)}


def test_expected_kernel_reproduces_the_tile_constants():
    for N, (sf, cf, sd, cd) in TILES.items():
        big = 10 ** 6           # so many columns that the quarter tile is out of the question
        assert ac.expected_kernel(N, False, 4, 4, big, 4, N, 256).B == sf
        assert ac.expected_kernel(N, True, 4, 4, 1, big, N, 256).B == cf
        assert ac.expected_kernel(N, False, 8, 4, big, 4, N, 256).B == sd
        assert ac.expected_kernel(N, True, 8, 8, 1, big, N, 256).B == cd
        for t in (4, 8):
            for contig in (False, True):
                k = ac.expected_kernel(N, contig, t, t, 1 if contig else 100, 100, N, 256)
                assert k.lds <= 65536 and k.threads <= 1024 and k.threads == k.B * ac.RADIX[N][1]
    assert ac.expected_kernel(1024, False, 8, 4, 32, 1, 1024, 256).lds == 65536        # k_fft_strided<double, .., 1024>: all 64 KiB
    assert ac.expected_kernel(512, True, 8, 8, 1, 16, 512, 256)[2:6] == (5, False, 5 * 32 * 17 * 16, 80)


def test_expected_kernel_quarter_tile_and_direct_tile():
    q = lambda N, inner, outer, cu=256, t=4, tin=4: ac.expected_kernel(N, False, t, tin, inner, outer, N, cu)
    assert q(32, 9, 2).quarter and q(32, 9, 2).B == 8 and not q(32, 8, 2).quarter
    assert q(512, 5, 2).B == 4 and not q(512, 4, 2).quarter
    assert not q(1024, 8, 1).quarter                                   # B = 8 < 16
    assert q(64, 32, 128).quarter and not q(64, 33, 128).quarter       # tiles * outer * 2 against the CU count
    assert not q(64, 32, 128, cu=255).quarter
    assert not q(256, 9, 2, t=8, tin=4).quarter                        # float32 only
    d = lambda n_in, t: ac.expected_kernel(4095, False, t, 4, 1, 4, n_in, 256).B
    assert [d(n, 4) for n in (384, 385, 768, 769, 1536, 1537, 3072, 3073, 4095)] == [16, 8, 8, 4, 4, 2, 2, 1, 1]
    assert [d(n, 8) for n in (192, 193, 384, 385, 768, 769, 1536, 1537, 4095)] == [16, 8, 8, 4, 4, 2, 2, 1, 1]
    assert ac.expected_kernel(4096, False, 8, 4, 1, 4, 4096, 256).lds == 65536 and ac.expected_kernel(4097, False, 4, 4, 1, 4, 4097, 256) is None
    # the contiguous direct sum: rows become the inner index
    assert ac.expected_kernel(70, True, 4, 4, 1, 30, 70, 256)[:3] == ("direct", 70, 16) and ac.expected_kernel(70, True, 4, 4, 1, 30, 70, 256).blocks == 2


def test_header_still_holds_the_restated_rules():
    """The lines the restatement copies, so that a change of the header shows up here."""
    src = open(HEADER).read()
    for line in ("int b = 65536 / (N * elem_bytes);", "return b > 32 ? 32 : (b < 1 ? 1 : b);", "int b = 256 / R2;",
                 "const int cap = 49152 / (R1 * (R2 + 1) * elem_bytes);", "if constexpr (B >= 16 && sizeof(T) == 4 && sizeof(TIN) == 4) {",
                 "if (tiles * p.outer * 2 <= ctx->num_cu && p.inner > B / 4) return launch_strided_b<T, TIN, N, R1, R2, B / 4>(ctx, p);",
                 "while (B > 1 && (size_t)p.n_in * B * sizeof(cplx<T>) > 48 * 1024) B >>= 1;", 'MMW_REQUIRE(N <= 4096, "fft: axis length %d not supported (max 4096)", N);'):
        assert line in src, line
    for N, (R1, R2) in ac.RADIX.items():
        assert f"case {N}: return launch_pow2<T, TIN, {N}, {R1}, {R2}>(ctx, p, contiguous);" in src


def test_case_list_reaches_every_dispatched_instantiation():
    ls = ac.launches()
    radix = {(t, tin, k.kind, k.N) for _, t, tin, k in ls if k.kind != "direct"}
    assert radix == {(t, tin, kind, N) for (t, tin, kind) in ac.REACHABLE for N in ac.RADIX}, "8 lengths x 4 dispatched (T, TIN, layout)"
    assert {(t, tin, k.kind) for _, t, tin, k in ls if k.kind != "direct"} == ac.REACHABLE
    quarter = {(k.N, k.B) for e, t, tin, k in ls if k.quarter}
    assert quarter == {(N, ac.strided_tile(N, 8) // 4) for N in ac.RADIX if N <= 512}
    assert {(k.N, k.B) for e, t, tin, k in ls if e == "angle" and k.kind == "strided" and not k.quarter} >= {(N, ac.strided_tile(N, 8)) for N in ac.RADIX}
    for t in (4, 8):
        assert {k.B for _, tt, _, k in ls if k.kind == "direct" and tt == t} == {16, 8, 4, 2, 1}
    # both layouts of the direct sum, in both element sizes
    assert {(e, t) for e, t, _, k in ls if k.kind == "direct"} >= {("angle", 4), ("range_angle", 4), ("rd32", 4), ("mag64", 8), ("range_profile", 8)}
    # the float64 kernels the issue names
    d = [(tin, k) for e, t, tin, k in ls if e == "mag64"]
    assert any(tin == 4 and k.N == 1024 and k.lds == 65536 for tin, k in d)
    assert any(tin == 8 and k.kind == "contig" and k.N == 512 and k.B == 5 and k.threads == 80 for tin, k in d)
    assert any(tin == 8 and k.kind == "contig" and k.N == 1024 and k.B == 2 for tin, k in d)
    # wide angle launches leave the quarter tile by the CU count, with a ragged last tile
    for c in ac.ANGLE_CASES:
        if c.name.startswith("wide"):
            bins = c.S * c.C
            assert -(-bins // c.B) * c.F * 2 > ac.NOMINAL_CU and bins % c.B and not c.quarter
        if c.name.startswith("narrow"):
            assert c.quarter == (c.A <= 512)


def test_float64_plans_and_float32_budgets_of_the_range_doppler_cases(monkeypatch):
    lib, plan = _lib.load_library(), (ctypes.c_int * 8)()
    for name in rb.ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for S, C in ac.MAG64_SHAPES:
        assert lib.mmw_diag_rd_plan(S, C, 1, plan) == 0
        assert plan[0] == (2 if (S, C) in ac.MAG64_NEEDS_SWITCH else 3), (S, C)
    assert lib.mmw_diag_rd_plan(64, 128, 1, plan) == 0 and plan[0] == 2        # a power of two of 8192 cells that fits the LDS: single pass
    monkeypatch.setenv("MMW_NO_MIXED_RD", "1")
    for S, C in ac.MAG64_SHAPES:
        assert lib.mmw_diag_rd_plan(S, C, 1, plan) == 0 and plan[0] == 3, (S, C)
    for name, value in ac.RD32_ENV.items():
        monkeypatch.setenv(name, value)
    for V, S, C in ac.RD32_SHAPES:
        assert lib.mmw_diag_detect_plan(S, C, _lib.CFAR_CA, 4, 4, 2, 2, 0, 0, 64, plan) == 0
        assert plan[7] == rb.generic_ulps(S, C) == 8 + ac.axis_ulps(S, S) + ac.axis_ulps(C, C), (S, C)


def test_buffers_stay_small():
    sizes = ac.buffer_bytes()
    assert max(sizes.values()) < 64 << 20, max(sizes, key=sizes.get)
    assert ac.RP_F * ac.RP_V * ac.RP_REFUSED * ac.RP_C * 8 < 1 << 20
