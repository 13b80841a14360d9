"""mmw_micro_doppler and mmw_sar_slices against the counted rounding bound of tests/partial_dft_cases.py, per output value:

    |dev - ref| <= ulps(S, C) 2^-24 L1,   L1 = sum |x[s][c]| of the antenna's slab,   ref = the two direct sums in long double

on one-hot impulses (A, SAR: every row, column and bin its own test), two impulses (B, micro-Doppler: a closed-form row, the
strongest rows planted just outside the window), coherent slabs (C: L1 equals the peak), Gaussian slabs (D, with the present
peak-relative bar next to it), exact power-of-two scalings inside the interval that include/mmwgpu.h states (E) and non-finite
and all-zero slabs (F).  Every family runs with the default rows in flight and with 4, 8 and 16 forced, bit for bit the same.
Every bound test prints the worst ratio it saw; DESIGN.md 4.16 and 4.24 carry the table.  Both entries are called through the C
ABI into poisoned buffers with guard elements (the helpers of test_gpu_micro_doppler.py and test_gpu_sar_range.py)."""
import numpy as np
import pytest

import partial_dft_cases as pc
from mmwave_radar_processing_amd import _lib
from test_gpu_micro_doppler import POISON as MD_POISON, run_abi
from test_gpu_sar_range import run_sar

pytestmark = pytest.mark.gpu


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def md_rows(ctx, cubes, rx, lo, hi):
    """mmw_micro_doppler on [F][V][S][C]: float32 [F][C]; the guard behind the rows is checked."""
    F, C = cubes.shape[0], cubes.shape[3]
    rc, buf = run_abi(ctx, cubes, rx, lo, hi)
    assert rc == _lib.MMW_OK, ctx.lib.mmw_last_error()
    assert np.all(buf[F * C:] == MD_POISON), "a guard element was written"
    return buf[:F * C].reshape(F, C)


def sar_blocks(ctx, cubes, rx, wins):
    rc, blocks = run_sar(ctx, cubes, rx, wins)
    assert rc == _lib.MMW_OK, ctx.lib.mmw_last_error()
    return blocks


def same_bits(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def under_every_kt(ctx, option, run, C):
    """run() with the default rows in flight, then with 4, 8 and 16 forced (those that the LDS holds at C chirps -- 16 rows up to 819,
    8 up to 1832; a forced count that does not fit is refused): the same bits.  Returns the default's result."""
    base = run()
    try:
        for kt in (k for k in (4, 8, 16) if pc.kt_fits(k, C)):
            ctx.set_option(option, kt)
            assert same_bits(run(), base), (option, kt)
    finally:
        ctx.set_option(option, None)
    return base


def md_of_case(ctx, cs):
    return under_every_kt(ctx, "MMW_MD_KT", lambda: md_rows(ctx, cs.x[None, None], 0, cs.lo, cs.hi), cs.x.shape[1])[0]


def sar_of_case(ctx, cs):
    return under_every_kt(ctx, "MMW_SAR_KT", lambda: sar_blocks(ctx, cs.x[None, None], 0, [cs.win]), cs.x.shape[1])[0]


# ------------------------------------------------------------------------------------------------------------- family A
@pytest.mark.parametrize("shape", pc.A_SHAPES, ids=ids(pc.A_SHAPES))
def test_family_a_one_hot_impulses_every_row_column_and_bin(shape):
    ctx = _lib.default_context()
    cases = pc.family_a(*shape)
    cubes = np.stack([c.x for c in cases])[:, None]
    blocks = under_every_kt(ctx, "MMW_SAR_KT", lambda: sar_blocks(ctx, cubes, 0, [c.win for c in cases]), shape[1])
    worst = 0.0
    for cs, blk in zip(cases, blocks):
        r = pc.sar_ratio(blk, cs.x, cs.win)
        worst = max(worst, r)
        assert r <= 1, (cs.name, r)
    print(f"partial DFT bound, A {shape[0]}x{shape[1]} sar ({len(cases)} impulses): worst ratio {worst:.3g}")


@pytest.mark.parametrize("shape", pc.A_SHAPES[:3], ids=ids(pc.A_SHAPES[:3]))
def test_family_a_window_alone_and_inside_a_wider_union(shape):
    """The twiddle table starts at the union's first row and is as long as the union: neither enters a frame's block."""
    ctx = _lib.default_context()
    S, C = shape
    cases = pc.family_a(S, C)
    r0 = S // 3
    win = (r0, r0 + max(1, S // 4), 1, C - 1)
    cubes = np.stack([c.x for c in cases])[:, None]
    alone = sar_blocks(ctx, cubes, 0, [win] * len(cases))
    wide_cubes = np.concatenate([cubes[:1], cubes, cubes[:1]])
    wide = sar_blocks(ctx, wide_cubes, 0, [(0, 1, 0, 1)] + [win] * len(cases) + [(S - 1, S, 0, C)])
    full = sar_blocks(ctx, cubes, 0, [c.win for c in cases])
    assert same_bits(wide[1:-1], alone)
    assert same_bits([b[win[0]:win[1], win[2]:win[3]] for b in full], alone)
    for cs, blk in zip(cases, alone):
        assert np.abs(blk).min() > 0.5                         # written, and an impulse's plane has magnitude 1 everywhere
    assert same_bits(wide[0], full[0][:1, :1]) and same_bits(wide[-1], full[0][S - 1:, :])


# ------------------------------------------------------------------------------------------------------------- family B
@pytest.mark.parametrize("shape", pc.B_SHAPES, ids=ids(pc.B_SHAPES))
def test_family_b_two_impulses_against_the_closed_form_row(shape):
    ctx = _lib.default_context()
    S, C = shape
    worst = 0.0
    for cs in pc.family_b(S, C):
        got = md_of_case(ctx, cs)
        K = cs.hi - cs.lo + 1
        bound = pc.ulps(S, C, True) * pc.EPS * pc.l1_of(cs.x)
        assert float(np.abs(got - pc.b_closed_form(S, C, K, cs.lo, cs.hi)).max()) <= bound, cs.name
        r = pc.md_ratio(got, cs.x, cs.lo, cs.hi)
        worst = max(worst, r)
        assert r <= 1, (cs.name, r)
    print(f"partial DFT bound, B {S}x{C} micro-Doppler (K = {', '.join(map(str, pc.B_KS))}): worst ratio {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------- family C
@pytest.mark.parametrize("shape", pc.C_SHAPES, ids=ids(pc.C_SHAPES))
def test_family_c_coherent_slabs(shape):
    ctx = _lib.default_context()
    worst_sar = worst_md = 0.0
    for sc, mc in pc.family_c(*shape):
        r = pc.sar_ratio(sar_of_case(ctx, sc), sc.x, sc.win)
        worst_sar = max(worst_sar, r)
        assert r <= 1, (sc.name, "sar", r)
        r = pc.md_ratio(md_of_case(ctx, mc), mc.x, mc.lo, mc.hi)
        worst_md = max(worst_md, r)
        assert r <= 1, (mc.name, "micro-Doppler", r)
    print(f"partial DFT bound, C {shape[0]}x{shape[1]}: worst ratio sar {worst_sar:.3g}, micro-Doppler {worst_md:.3g}")


# ------------------------------------------------------------------------------------------------------------- family D
@pytest.mark.parametrize("shape", pc.D_SHAPES, ids=ids(pc.D_SHAPES))
def test_family_d_gaussian_slabs_per_value_and_against_the_peak(shape):
    ctx = _lib.default_context()
    sc, mds = pc.family_d(*shape)
    peak = pc.full_plane_peak(sc.x)
    blk = sar_of_case(ctx, sc)
    worst_sar = pc.sar_ratio(blk, sc.x, sc.win)
    assert worst_sar <= 1, (sc.name, worst_sar)
    old = float(np.abs(blk - pc.reference_of(sc.x, ("sar", sc.win))).max()) / peak
    assert old <= pc.SPEC_TOL, (sc.name, old)
    worst_md = 0.0
    for mc in mds:
        got = md_of_case(ctx, mc)
        r = pc.md_ratio(got, mc.x, mc.lo, mc.hi)
        worst_md = max(worst_md, r)
        assert r <= 1, (mc.name, r)
        old = max(old, float(np.abs(got - pc.reference_of(mc.x, ("md", mc.lo, mc.hi))).max()) / peak)
        assert old <= pc.SPEC_TOL, (mc.name, old)
    print(f"partial DFT bound, D {shape[0]}x{shape[1]}: worst ratio sar {worst_sar:.3g}, micro-Doppler {worst_md:.3g}; "
          f"worst error over the peak {old:.3g} (bar {pc.SPEC_TOL:g})")


# ------------------------------------------------------------------------------------------------------------- family E
def test_family_e_powers_of_two_scale_every_bit_inside_the_stated_interval():
    """include/mmwgpu.h, mmw_micro_doppler and mmw_sar_slices: scaling the input by 2^e scales the output by 2^e bit for bit
    while every float32 intermediate (the partial sums; for the row also im^2 and |Y|^2) stays normal and finite."""
    ctx = _lib.default_context()
    x, (lo, hi), win, md_iv, sar_iv = pc.e_case()
    base_md = under_every_kt(ctx, "MMW_MD_KT", lambda: md_rows(ctx, x[None, None], 0, lo, hi), x.shape[1])
    base_sar = under_every_kt(ctx, "MMW_SAR_KT", lambda: sar_blocks(ctx, x[None, None], 0, [win]), x.shape[1])
    for e in sorted({md_iv[0], md_iv[0] // 2, 0, md_iv[1] // 2, md_iv[1]}):
        got = under_every_kt(ctx, "MMW_MD_KT", lambda: md_rows(ctx, pc.scaled(x, e)[None, None], 0, lo, hi), x.shape[1])
        assert same_bits(got, np.ldexp(base_md, e)), ("micro-Doppler", e)
    for e in sorted({sar_iv[0], md_iv[0], 0, md_iv[1], sar_iv[1]}):
        got = under_every_kt(ctx, "MMW_SAR_KT", lambda: sar_blocks(ctx, pc.scaled(x, e)[None, None], 0, [win]), x.shape[1])
        assert same_bits(got[0].view(np.float32), np.ldexp(base_sar[0].view(np.float32), e)), ("sar", e)
    print(f"partial DFT scaling, {pc.E_SHAPE[0]}x{pc.E_SHAPE[1]}: bit for bit on e in [{md_iv[0]}, {md_iv[1]}] (micro-Doppler), "
          f"[{sar_iv[0]}, {sar_iv[1]}] (sar)")


# ------------------------------------------------------------------------------------------------------------- family F
F_WINS = [(3, 12, 0, 23), (0, 40, 20, 23), (5, 6, 0, 1)]


def f_run(ctx, cubes):
    lo, hi = pc.F_WINDOW
    rows = under_every_kt(ctx, "MMW_MD_KT", lambda: md_rows(ctx, cubes, 1, lo, hi), cubes.shape[3])
    blocks = under_every_kt(ctx, "MMW_SAR_KT", lambda: sar_blocks(ctx, cubes, 1, F_WINS), cubes.shape[3])
    return rows, blocks


@pytest.mark.parametrize("bits", [pc.POS_NAN, pc.NEG_NAN], ids=["nan", "negative-nan"])
def test_family_f_a_nan_poisons_its_frame_and_nothing_else(bits):
    ctx = _lib.default_context()
    clean_rows, clean_blocks = f_run(ctx, pc.f_cubes())
    assert np.all(np.isfinite(clean_rows)) and all(np.all(np.isfinite(b.view(np.float32))) for b in clean_blocks)
    for other in (False, True):                                 # ... and antenna 0, which is not read, NaN throughout
        rows, blocks = f_run(ctx, pc.poisoned(pc.f_cubes(), bits, other_antenna_nan=other))
        assert np.all(np.isnan(rows[1])) and np.all(np.isnan(blocks[1].view(np.float32)))
        for f in (0, 2):
            assert same_bits(rows[f], clean_rows[f]) and same_bits(blocks[f], clean_blocks[f]), f


def test_family_f_an_infinity_leaves_no_finite_output_in_its_frame():
    ctx = _lib.default_context()
    clean_rows, clean_blocks = f_run(ctx, pc.f_cubes())
    rows, blocks = f_run(ctx, pc.poisoned(pc.f_cubes(), pc.POS_INF))
    assert not np.any(np.isfinite(rows[1])) and not np.any(np.isfinite(blocks[1].view(np.float32)))
    for f in (0, 2):
        assert same_bits(rows[f], clean_rows[f]) and same_bits(blocks[f], clean_blocks[f]), f


def test_family_f_an_all_zero_slab_gives_positive_zero():
    ctx = _lib.default_context()
    cubes = pc.f_cubes().copy()
    cubes[1, 1] = 0
    rows, blocks = f_run(ctx, cubes)
    assert not rows[1].view(np.uint32).any() and not blocks[1].view(np.uint32).any()
    assert rows[0].all() and rows[2].all()
