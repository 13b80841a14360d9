"""tests/partial_dft_cases.py checked against itself, without a GPU: the long double reference against np.fft, the float32
restatement of k_micro_doppler / k_sar_slices inside the counted bound on every case, every mutant caught by an assertion that
tests/test_gpu_partial_dft_bound.py makes, the closed forms of the two-impulse family, and the scaling interval at its ends.

What the present bar (1e-5 of the plane's peak on marker tones) does with the mutants is asserted as it is, OLD_BAR below: it
catches the four structural ones, because a tone spreads its energy evenly over every sample and chirp, so a dropped partial sum
or term removes a fixed share of the peak itself (a quarter of tail / C, 1 / C), and the tones at rows lo - 1 and hi + 1 and the
odd chirp counts are there for the other two.  It passes the float-angle twiddles (2.9e-6 of the peak at most: the tones stop at
r s < 2^12), and no test put a non-finite value into a slab."""
import numpy as np
import pytest

import partial_dft_cases as pc

F64_TOL = 64 * 2.0 ** -53               # of L1: np.fft in float64 (Bluestein at the prime lengths) against the long double sums


def sar_cases():
    out = [c for S, C in pc.A_SHAPES for c in pc.family_a(S, C)]
    out += [sc for S, C in pc.C_SHAPES for sc, _ in pc.family_c(S, C)]
    return out + [pc.family_d(S, C)[0] for S, C in pc.D_SHAPES]


def md_cases():
    out = [c for S, C in pc.B_SHAPES for c in pc.family_b(S, C)]
    out += [mc for S, C in pc.C_SHAPES for _, mc in pc.family_c(S, C)]
    return out + [m for S, C in pc.D_SHAPES for m in pc.family_d(S, C)[1]]


def test_the_count_is_the_closed_form():
    assert pc.first_order(256, 128) == 5 + 544 and pc.ulps(256, 128) == 549 + 1 + 1 and pc.ulps(256, 128, True) == 553
    assert pc.ulps(1, 1) == 5 + 6 + 2 and pc.ulps(1021, 3) == 740 and pc.ulps(3, 3444) > pc.first_order(3, 3444) + 2
    # the second-order term is what (1 + u)^n - 1 needs beyond n u
    for S, C in ((8, 7), (256, 128), (1021, 3444)):
        n = pc.first_order(S, C)
        assert np.expm1(n * np.log1p(pc.EPS)) <= pc.ulps(S, C) * pc.EPS


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic: no neighbouring float32 is nearer to a b + c, with and without cancellation."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(600).astype(np.float32), rng.standard_normal(600).astype(np.float32)
    c = rng.standard_normal(600)
    c[:300] = -(a[:300].astype(np.float64) * b[:300]) * (1 + 1e-7 * c[:300])
    c = c.astype(np.float32)
    got = pc.fma32(a, b, c)
    for i in range(600):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        err = abs(Fraction(float(got[i])) - exact)
        for side in (-np.inf, np.inf):
            assert err <= abs(Fraction(float(np.nextafter(got[i], np.float32(side)))) - exact), i
    # 2^37 + 2^14 + 2^13 - 2^-33 lies just below a float32 tie; float64 rounds it onto the tie, and from there to even: wrong
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** 13 * (1 - 2.0 ** -23)), np.float32(2.0 ** 37 + 2.0 ** 14)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 37 + 2.0 ** 15)
    assert pc.fma32(a, b, c) == c


def test_the_reference_agrees_with_np_fft_to_float64_rounding():
    for cs in sar_cases():
        r0, r1, c0, c1 = cs.win
        plane = np.fft.fftshift(np.fft.fft2(cs.x.astype(np.complex128)), axes=1)[r0:r1, c0:c1]
        err = float(np.abs(pc.reference_of(cs.x, ("sar", cs.win)) - plane).max())
        assert err <= F64_TOL * pc.l1_of(cs.x), cs.name
    for cs in md_cases():
        row = np.abs(np.fft.fftshift(np.fft.fft2(cs.x.astype(np.complex128)), axes=1))[cs.lo:cs.hi + 1].max(0)
        err = float(np.abs(pc.reference_of(cs.x, ("md", cs.lo, cs.hi)) - row).max())
        assert err <= F64_TOL * pc.l1_of(cs.x), cs.name


def test_the_float32_restatement_is_inside_the_bound_on_every_case():
    worst = {}
    for cs in sar_cases():
        r = pc.sar_ratio(pc.f32_sar(cs.x, cs.win), cs.x, cs.win)
        worst[cs.name[0] + " sar"] = max(worst.get(cs.name[0] + " sar", 0.0), r)
        assert r <= 1, (cs.name, r)
    for cs in md_cases():
        r = pc.md_ratio(pc.f32_micro_doppler(cs.x, cs.lo, cs.hi), cs.x, cs.lo, cs.hi)
        worst[cs.name[0] + " md"] = max(worst.get(cs.name[0] + " md", 0.0), r)
        assert r <= 1, (cs.name, r)
    print("float32 restatement, worst share of the bound:", {k: f"{v:.3g}" for k, v in sorted(worst.items())})


def test_the_rows_in_flight_do_not_enter_the_restatement():
    cs = pc.family_b(29, 11)[4]                                 # K = 9
    base = pc.f32_micro_doppler(cs.x, cs.lo, cs.hi)
    assert all(np.array_equal(pc.f32_micro_doppler(cs.x, cs.lo, cs.hi, kt=kt), base) for kt in (4, 8, 16))
    assert [pc.pick_kt(K) for K in (1, 4, 5, 8, 9, 16, 17, 25)] == [4, 4, 8, 8, 16, 16, 8, 16]


def test_the_two_impulse_closed_forms_equal_the_reference():
    for S, C in pc.B_SHAPES:
        planted_lo = planted_hi = 0.0
        for cs in pc.family_b(S, C):
            K = cs.hi - cs.lo + 1
            ref = pc.reference_of(cs.x, ("md", cs.lo, cs.hi))
            assert float(np.abs(pc.b_closed_form(S, C, K, cs.lo, cs.hi) - ref).max()) <= 2.0 ** -58, cs.name
            # the pattern differs by column, by a hundred times the bound at the least
            assert ref.max() - ref.min() > 100 * pc.ulps(S, C, True) * pc.EPS * pc.l1_of(cs.x)
            # a window off by one row on either side changes the row
            planted_lo = max(planted_lo, float((pc.b_closed_form(S, C, K, cs.lo - 1, cs.hi) - ref).max()))
            planted_hi = max(planted_hi, float((pc.b_closed_form(S, C, K, cs.lo, cs.hi + 1) - ref).max()))
        assert planted_lo > 0.5 and planted_hi > 0.5             # of values between 0.5 and 1.5: the order of the value itself


# ------------------------------------------------------------------------------------------------------------ the mutants
def sar_of(name):
    return next(c for c in sar_cases() if c.name == name)


def md_of(name):
    return next(c for c in md_cases() if c.name == name)


def nan_rows(mutant, nan_sign):
    """The micro-Doppler rows of the three frames of family F with a NaN in frame 1, restated."""
    V, S, C = pc.F_SHAPE
    cubes = pc.poisoned(pc.f_cubes(), pc.NEG_NAN if nan_sign else pc.POS_NAN)
    return [pc.f32_micro_doppler(cubes[f, 1], *pc.F_WINDOW, mutant=mutant, nan_sign=nan_sign) for f in range(3)]


# mutant: (the case, the assertion of the GPU test it violates)
CAUGHT_BY = {
    "drop_wave3_tail": ("a-63x70-s59c64", "family A within the bound (sample 59 is wave 3's, column 64 is in the tail)"),
    "drop_last_term": ("a-5x130-s4c129", "family A within the bound (the impulse sits in the last term)"),
    "padded_rows": ("b-29x11-K5", "family B within the bound (5 rows run as 1 x 8: rows hi + 1 .. hi + 3 are padding)"),
    "odd_shift": ("a-8x7-s7c6", "family A within the bound (7 chirps)"),
    "float_angle": ("a-1021x3-s1020c2", "family A within the bound (r s0 up to 1020^2)"),
    "signed_max": ("f-negative-nan", "family F: every output of the frame with the NaN is NaN"),
}


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_every_mutant_violates_an_assertion_of_the_gpu_test(mutant):
    name, _ = CAUGHT_BY[mutant]
    if mutant == "signed_max":
        good, bad = nan_rows(None, True), nan_rows(mutant, True)
        assert np.all(np.isnan(good[1])) and not np.all(np.isnan(bad[1]))
        assert np.all(np.isnan(nan_rows(None, False)[1]))
        assert all(np.array_equal(good[f], bad[f]) and np.all(np.isfinite(good[f])) for f in (0, 2))
    elif name.startswith("b-"):
        cs = md_of(name)
        assert pc.md_ratio(pc.f32_micro_doppler(cs.x, cs.lo, cs.hi), cs.x, cs.lo, cs.hi) <= 1
        assert pc.md_ratio(pc.f32_micro_doppler(cs.x, cs.lo, cs.hi, mutant=mutant), cs.x, cs.lo, cs.hi) > 1
    else:
        cs = sar_of(name)
        assert pc.sar_ratio(pc.f32_sar(cs.x, cs.win), cs.x, cs.win) <= 1
        assert pc.sar_ratio(pc.f32_sar(cs.x, cs.win, mutant=mutant), cs.x, cs.win) > 1


# what the present bar says of each mutant on the marker tones of the existing tests (True: within 1e-5 of the peak everywhere)
OLD_BAR = {"drop_wave3_tail": False, "drop_last_term": False, "padded_rows": False, "odd_shift": False, "float_angle": True}
TONE_SHAPES = ((64, 32), (40, 23), (8, 130))


@pytest.mark.parametrize("mutant", sorted(OLD_BAR))
def test_what_the_present_bar_says_of_the_mutants_on_the_marker_tones(mutant):
    worst = clean = 0.0
    for S, C in TONE_SHAPES:
        for lo, hi in pc.md_windows(S):
            x = pc.tone_slab(S, C, lo, hi)
            plane = np.abs(np.fft.fftshift(np.fft.fft2(x.astype(np.complex128)), axes=1))
            want, peak = plane[lo:hi + 1].max(0), plane.max()
            worst = max(worst, float(np.abs(pc.f32_micro_doppler(x, lo, hi, mutant=mutant) - want).max() / peak))
            clean = max(clean, float(np.abs(pc.f32_micro_doppler(x, lo, hi) - want).max() / peak))
    print(f"{mutant}: worst error {worst:.3g} of the peak on the marker tones (unmutated {clean:.3g}, bar {pc.SPEC_TOL:g})")
    assert clean <= pc.SPEC_TOL
    assert (worst <= pc.SPEC_TOL) == OLD_BAR[mutant]


# ---------------------------------------------------------------------------------------------------------- family E
def test_the_scaling_interval_is_exact_at_both_ends():
    x, (lo, hi), win, md_iv, sar_iv = pc.e_case()
    assert md_iv[0] < 0 < md_iv[1] and sar_iv[0] < md_iv[0] and md_iv[1] < sar_iv[1]      # the squares narrow it
    base_md, base_sar = pc.f32_micro_doppler(x, lo, hi), pc.f32_sar(x, win)
    for iv, run, base in ((md_iv, lambda y, t: pc.f32_micro_doppler(y, lo, hi, track=t), base_md),
                          (sar_iv, lambda y, t: pc.f32_sar(y, win, track=t), base_sar)):
        for e in iv:
            t = pc.Track()
            got = run(pc.scaled(x, e), t)
            assert not t.bad, e
            parts = got.view(np.float32)
            assert np.array_equal(parts, np.ldexp(base.view(np.float32), e)), e
        for e in (iv[0] - 1, iv[1] + 1):
            t = pc.Track()
            run(pc.scaled(x, e), t)
            assert t.bad, e
