"""The ground detector's peak picker and zoom spectrum at their edges, straight through the C ABI.

Picker: the crafted rows of tests/ground_pick_cases.py through mmw_diag_ground_pick (k_ground_peaks on a caller's profile), all rows
of one length in one launch and each row alone.  A row whose crafted decision lies inside the rounding band, or ties two of the
peaks it would return, must come back flagged (count -1, nothing written); every other row must be decided, bit for bit as
RangeProcessor.find_peaks decides it.  Flagged is never accepted for a row eight bands away.

Zoom spectrum: mmw_ground_zoom_candidates on uploaded candidate lists.  d_spec against a direct DFT in np.longdouble (f0 and df in
float64 by the expressions of RangeProcessor.zoom_fft, everything after them in extended precision), within
32 * S * 2^-53 * L1 with L1 = mean_v sum_i hann_i (|re| + |im|): in units of S * 2^-53 * L1 the two roundings of fk = f0 + k df give
<= 4 pi, the rounding of fk * i gives <= 2 pi, the summation <= 1, about 20 together; the rest is for sincospi, hypot and the mean.
The picks against RangeProcessor.find_peaks on the DOWNLOADED spectrum, and batches whose single tone sits on each interior bin of a
clipped-low, an interior and a clipped-high window against np.linspace, bit for bit.
"""
import time

import numpy as np
import pytest

import ground_pick_cases as G
from scipy.signal import find_peaks

from mmwave_radar_processing_amd import _lib
from mmwave_radar_processing_amd.processors.range_resp import RangeProcessor

pytestmark = pytest.mark.gpu

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, ("the spectrum reference needs an extended-precision np.longdouble (64-bit mantissa); "
                                         f"this platform's has eps {np.finfo(LD).eps}")
PI_LD = LD(4) * np.arctan(LD(1))
POISON, POISON_I, GUARD = -777.25, -99, 16
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


# ------------------------------------------------------------------------------------------------------------- picker
def run_pick(ctx, rows, m, expect=_lib.MMW_OK, S=None):
    """mmw_diag_ground_pick on rows [n][S] with poisoned outputs and guard words behind them: (cand [n][3], counts [n])."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    n, S = rows.shape[0], (rows.shape[1] if S is None else S)
    bins = np.arange(max(S, 1), dtype=np.float64)
    bufs = [ctx.alloc(rows.nbytes), ctx.alloc(bins.nbytes), ctx.alloc((n * 3 + GUARD) * 8), ctx.alloc((n + GUARD) * 4)]
    try:
        bufs[0].upload(rows)
        bufs[1].upload(bins)
        bufs[2].upload(np.full(n * 3 + GUARD, POISON))
        bufs[3].upload(np.full(n + GUARD, POISON_I, np.int32))
        rc = ctx.lib.mmw_diag_ground_pick(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, S, m)
        assert rc == expect, (rc, expect, S, m)
        cand, counts = bufs[2].download((n * 3 + GUARD,), np.float64), bufs[3].download((n + GUARD,), np.int32)
        assert np.all(cand[n * 3:] == POISON) and np.all(counts[n:] == POISON_I), "guard words overwritten"
        return cand[:n * 3].reshape(n, 3), counts[:n]
    finally:
        for b in bufs:
            b.free()


def check_row(case, m, cand, count):
    tag = f"{case.name} S {case.S} max_peaks {m}"
    want = G.reference(G.to_db(case.p), m)
    if case.flagged:
        assert count == -1 and np.all(cand == POISON), (tag, count, cand)
    elif case.nonfinite and count == -1:
        assert np.all(cand == POISON), (tag, cand)
    else:
        assert count == len(want), (tag, count, cand, want)                 # never flagged, never a different answer
        assert cand[:count].tobytes() == want.tobytes() and np.all(cand[count:] == POISON), (tag, cand, want)


@pytest.mark.parametrize("S", sorted(G.cases_by_length()))
def test_picker_rows_in_one_launch_and_alone(ctx, S):
    cases = G.cases_by_length()[S]
    for m in (2, 3):
        rows = [c for c in cases if m in c.max_peaks]
        cand, counts = run_pick(ctx, np.stack([c.p for c in rows]), m)
        for k, c in enumerate(rows):
            check_row(c, m, cand[k], counts[k])
            one_cand, one_count = run_pick(ctx, c.p[None], m)
            assert one_count[0] == counts[k] and one_cand[0].tobytes() == cand[k].tobytes(), (c.name, m)   # no state between workgroups
        must = [c for c in rows if not c.flagged and not c.nonfinite]
        n_flag = sum(int(counts[k] == -1) for k, c in enumerate(rows) if not c.flagged and not c.nonfinite)
        print(f"picker S {S} max_peaks {m}: {len(rows)} rows, {sum(c.flagged for c in rows)} must flag, {len(must)} must decide "
              f"({n_flag} of them flagged), non-finite rows flagged: "
              f"{[c.name for k, c in enumerate(rows) if c.nonfinite and counts[k] == -1]}")
        assert n_flag == 0


def test_flag_all_flags_every_row(ctx):
    rows = [c for c in G.cases_by_length()[G.S0] if 3 in c.max_peaks]
    ctx.set_option("MMW_GROUND_FLAG_ALL", 1)
    try:
        cand, counts = run_pick(ctx, np.stack([c.p for c in rows]), 3)
    finally:
        ctx.set_option("MMW_GROUND_FLAG_ALL", None)
    assert np.all(counts == -1)
    _, counts = run_pick(ctx, np.stack([c.p for c in rows]), 3)
    assert np.any(counts >= 0)


def test_picker_refusals_leave_the_outputs_untouched(ctx):
    for S, m in ((2, 3), (3073, 3), (64, 4), (64, 1)):
        cand, counts = run_pick(ctx, np.ones((2, 3073)), m, expect=_lib.MMW_ERR_INVALID, S=S)
        assert np.all(cand == POISON) and np.all(counts == POISON_I), (S, m)
    cand, counts = run_pick(ctx, np.ones((2, 3072)), 2)                          # the largest row still runs
    assert counts.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------- zoom spectrum
RANGE_RES = 0.1


def zoom_params(S):
    bins = np.arange(S) * RANGE_RES
    return dict(half=8 * RANGE_RES, hi_cap=float(bins.max() - 1e-6), fs=1 / RANGE_RES, range_max=S * RANGE_RES)


def window(c, half, hi_cap):
    return max(1e-6, c - half), min(hi_cap, c + half)                       # Altimeter._look_zoom


def f0_df(lo, hi, S, fs, range_max):
    fstart, fstop = lo * fs / range_max, hi * fs / range_max                # RangeProcessor.zoom_fft, float64
    return fstart / fs, (fstop - fstart) / S / fs


def candidates(S):
    """Clipped low (c - half < 1e-6), interior, clipped high (c + half > hi_cap), in metres."""
    edge = min(4.0, S / 4)
    return [edge * RANGE_RES, (S / 2) * RANGE_RES, (S - 1 - edge) * RANGE_RES]


def tones_cube(rng, V, S, C, tones, noise=3):
    """Integer-valued complex64 [V][S][C]: chirp 0 holds the tones (range in metres, amplitude) plus integer noise; the other
    chirps hold noise ten times the strongest tone, which a wrong stride would pick up."""
    i = np.arange(S)
    x = np.zeros((V, S), np.complex128)
    for r, a in tones:
        x += a * np.exp(1j * (2 * np.pi * (r / (S * RANGE_RES)) * i[None, :] + rng.uniform(0, 2 * np.pi, (V, 1))))
    cube = rng.integers(-10000, 10001, (V, S, C)) + 1j * rng.integers(-10000, 10001, (V, S, C))
    cube[:, :, 0] = np.round(x.real) + 1j * np.round(x.imag) + rng.integers(-noise, noise + 1, (V, S)) + 1j * rng.integers(-noise, noise + 1, (V, S))
    return cube.astype(np.complex64)


def spectrum_ref(x0, lo, hi, S, fs, range_max):
    """mean over antennas of |sum_i hann_i x_i exp(-2 pi j fk i)|, fk = f0 + k df, in np.longdouble; and L1."""
    f0, df = f0_df(lo, hi, S, fs, range_max)
    w = np.hanning(S).astype(LD)
    xr, xi = x0.real.astype(LD) * w, x0.imag.astype(LD) * w                                    # [V][S]
    fk, i = LD(f0) + np.arange(S, dtype=LD) * LD(df), np.arange(S, dtype=LD)
    out = np.empty(S, LD)
    for k0 in range(0, S, 256):
        t = fk[k0:k0 + 256, None] * i[None, :]
        ang = LD(-2) * PI_LD * (t - np.rint(t))
        cs, sn = np.cos(ang), np.sin(ang)
        mag = np.hypot(cs @ xr.T - sn @ xi.T, sn @ xr.T + cs @ xi.T)                           # [k][V]
        acc = np.zeros(mag.shape[0], LD)
        for v in range(mag.shape[1]):
            acc += mag[:, v]                                                                   # antennas added in order
        out[k0:k0 + 256] = acc / LD(mag.shape[1])
    l1 = float(np.mean(np.sum(np.abs(xr) + np.abs(xi), axis=1)))
    return out, l1


def run_zoom(ctx, cubes, cand, counts, S, expect=_lib.MMW_OK, **par):
    F, V, _, C = cubes.shape
    n_spec, n_zc, n_cnt = F * 3 * S, F * 3 * 2, F * 3
    bufs = [ctx.alloc(cubes.nbytes), ctx.alloc(cand.nbytes), ctx.alloc(counts.nbytes), ctx.alloc((n_spec + GUARD) * 8),
            ctx.alloc((n_zc + GUARD) * 8), ctx.alloc((n_cnt + GUARD) * 4)]
    try:
        for b, a in zip(bufs, (cubes, cand, counts, np.full(n_spec + GUARD, POISON), np.full(n_zc + GUARD, POISON),
                               np.full(n_cnt + GUARD, POISON_I, np.int32))):
            b.upload(a)
        rc = ctx.lib.mmw_ground_zoom_candidates(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr,
                                                F, V, S, C, par["half"], par["hi_cap"], par["fs"], par["range_max"])
        assert rc == expect, (rc, expect)
        spec, zc, zn = (bufs[3].download((n_spec + GUARD,), np.float64), bufs[4].download((n_zc + GUARD,), np.float64),
                        bufs[5].download((n_cnt + GUARD,), np.int32))
        assert np.all(spec[n_spec:] == POISON) and np.all(zc[n_zc:] == POISON) and np.all(zn[n_cnt:] == POISON_I), "guard words overwritten"
        return spec[:n_spec].reshape(F, 3, S), zc[:n_zc].reshape(F, 3, 2), zn[:n_cnt].reshape(F, 3)
    finally:
        for b in bufs:
            b.free()


FLAGGED_WINDOWS = []


def decision_within(spec, width):
    """Does RangeProcessor.find_peaks on 20 log10(spec) make a decision whose two sides differ by no more than `width` dB: unequal
    neighbours, a prominence against 6 dB, or -- among the strongest three -- a value against max - 20 dB or against the next."""
    y = 20 * np.log10(spec)
    d = np.abs(np.diff(y))
    if np.any((np.diff(spec) != 0) & (d <= width)):
        return True
    idx, props = find_peaks(y, prominence=0)
    if np.any(np.abs(props["prominences"] - 6.0) <= width):
        return True
    top = np.sort(y[idx[props["prominences"] >= 6.0]])[::-1][:3]
    return bool(len(top) and (np.any(np.abs(top - (top[0] - 20.0)) <= width) or np.any(np.abs(np.diff(top)) <= width)))


def check_picks(spec, lo, hi, zcand, zcount, tag, may_flag=False):
    S = len(spec)
    want = np.asarray(RangeProcessor.find_peaks(None, 20 * np.log10(spec), np.linspace(lo, hi, S), 2)[0], dtype=np.float64)
    if zcount == -1 and may_flag and decision_within(spec, 2 * G.BAND):
        FLAGGED_WINDOWS.append(tag)                                     # the host decides this one: nothing written
        assert np.all(zcand == POISON), (tag, zcand)
        return
    assert zcount >= 0, (tag, "flagged: the tones were chosen so that no window holds a decision inside the band")
    assert zcount == len(want) and zcand[:zcount].tobytes() == want.tobytes() and np.all(zcand[zcount:] == POISON), (tag, zcand, want)


# (V, S, C, counts per frame): every count of -1, 0, 1, 2, 3 where the reference is cheap; S = 2048 costs a second per window.
# np.hanning(3) is (0, 1, 0): with one antenna the spectrum of S = 3 is |x[1]| on every bin, equal up to the rounding of sincospi and
# hypot -- bitwise equal (no peak) or a neighbour decision inside the band (flagged, rightly).  That shape has ONE live window, the
# only one of this file that may come back flagged.
ZOOM_SHAPES = [(1, 3, 1, (1, -1, 0)), (12, 64, 3, (3, -1, 0, 1, 2)), (16, 255, 2, (3, -1, 0, 1, 2)), (17, 64, 1, (3, -1, 0, 1, 2)),
               (33, 64, 1, (3, -1, 0, 1, 2)), (12, 512, 1, (3, -1, 0, 1, 2)), (3, 257, 2, (3, -1, 0, 1, 2)), (2, 2048, 1, (-1, 1))]


@pytest.mark.parametrize("V,S,C,counts", ZOOM_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_zoom_spectrum_and_picks(ctx, V, S, C, counts):
    par = zoom_params(S)
    rng = np.random.default_rng(1000 * V + S)
    lo_c, mid_c, hi_c = candidates(S)
    F = len(counts)
    # every frame lists the three windows in another order, so each kind is also the only live one of some frame
    cand = np.array([np.roll([lo_c, mid_c, hi_c], -f) for f in range(F)])
    if S == 2048:
        cand[:, 0] = hi_c                                               # the largest fk * i: the worst case of the phase rounding
    tones = [(c + d * RANGE_RES, a) for c in (lo_c, mid_c, hi_c) for d, a in ((-2.3, 1000.0), (3.1, 400.0))]
    cubes = np.stack([tones_cube(rng, V, S, C, tones) for _ in range(F)])
    counts = np.array(counts, np.int32)
    spec, zcand, zcounts = run_zoom(ctx, cubes, cand, counts, S, **par)
    worst, n_win = 0.0, 0
    for f in range(F):
        for j in range(3):
            tag = f"V {V} S {S} C {C} frame {f} window {j}"
            if j >= counts[f]:
                assert zcounts[f, j] == 0 and np.all(spec[f, j] == POISON) and np.all(zcand[f, j] == POISON), tag
                continue
            lo, hi = window(cand[f, j], par["half"], par["hi_cap"])
            ref, l1 = spectrum_ref(cubes[f, :, :, 0], lo, hi, S, par["fs"], par["range_max"])
            ratio = float(np.max(np.abs(spec[f, j].astype(LD) - ref))) / (32 * S * 2.0 ** -53 * l1)
            worst, n_win = max(worst, ratio), n_win + 1
            assert ratio <= 1.0, (tag, ratio)
            check_picks(spec[f, j], lo, hi, zcand[f, j], zcounts[f, j], tag, may_flag=(S == 3))
            if S >= 64:
                assert zcounts[f, j] >= 1, tag                             # the strong tone of the window is found
    kinds = {(window(c, par["half"], par["hi_cap"])[0] == 1e-6, window(c, par["half"], par["hi_cap"])[1] == par["hi_cap"])
             for f in range(F) for c in cand[f, :max(counts[f], 0)]}
    assert S == 2048 or kinds >= ({(True, True)} if S == 3 else {(True, False), (False, False), (False, True)})
    print(f"zoom V {V} S {S} C {C}: {n_win} windows, worst |dev - ref| / (32 S 2^-53 L1) = {worst:.3e}")


def test_zoom_refuses_more_bins_than_it_has_threads_for(ctx):
    S = 2049
    cubes = np.zeros((1, 1, S, 1), np.complex64)
    spec, zcand, zcounts = run_zoom(ctx, cubes, np.full((1, 3), 1.0), np.array([1], np.int32), S, expect=_lib.MMW_ERR_INVALID,
                                    **zoom_params(S))
    assert np.all(spec == POISON) and np.all(zcand == POISON) and np.all(zcounts == POISON_I)


def test_zoom_bins_equal_linspace_on_every_bin_that_can_hold_a_peak(ctx):
    """(2, 64, 1), one frame per (window, bin k = 1 .. 62): a single tone on bin k of a clipped-low, an interior and a clipped-high
    window, narrow (half = 8 range cells) and wide (0.45 range_max).  Where the strongest peak is k, zcand[0] must be
    np.linspace(lo, hi, 64)[k] bit for bit; every reported bin is compared with np.linspace in any case.  A Hann main lobe falls by
    6 dB one range cell from its top, and scipy asks for 6 dB of prominence inside the window, so a bin closer to the window's end
    than one cell (5.4 bins in the narrow windows, 1.3 in the wide ones) cannot be a peak: the narrow windows must serve k = 8 .. 55,
    the wide ones k = 2 .. 61.  Bins 1 and 62 would need a window of the whole range."""
    V, S, C = 2, 64, 1
    par = zoom_params(S)
    rng = np.random.default_rng(64)
    ks = np.arange(1, S - 1)
    for name, half, cs, k_lo, k_hi in (("narrow", par["half"], candidates(S), 8, 55),
                                       ("wide", 0.45 * par["range_max"], [f * par["range_max"] for f in (0.3, 0.5, 0.7)], 2, 61)):
        wins = [window(c, half, par["hi_cap"]) for c in cs]
        assert wins[0][0] == 1e-6 and wins[2][1] == par["hi_cap"] and wins[1] == (cs[1] - half, cs[1] + half)
        assert wins[0][1] < par["hi_cap"] and wins[2][0] > 1e-6
        cubes, cand = [], []
        for j, (lo, hi) in enumerate(wins):
            f0, df = f0_df(lo, hi, S, par["fs"], par["range_max"])
            for k in ks:
                cubes.append(tones_cube(rng, V, S, C, [((f0 + k * df) * par["range_max"], 1000.0)], noise=1))   # frequency f -> range f * range_max
                cand.append([cs[j], POISON, POISON])
        F = len(cubes)
        spec, zcand, zcounts = run_zoom(ctx, np.stack(cubes), np.array(cand), np.ones(F, np.int32), S, **dict(par, half=half))
        for j, (lo, hi) in enumerate(wins):
            served = []
            for n, k in enumerate(ks):
                f, tag = j * len(ks) + n, f"{name} window {j} bin {k}"
                check_picks(spec[f, 0], lo, hi, zcand[f, 0], zcounts[f, 0], tag)
                assert np.argmax(spec[f, 0]) == k, (tag, np.argmax(spec[f, 0]))
                if zcounts[f, 0] >= 1 and zcand[f, 0, 0].tobytes() == np.linspace(lo, hi, S)[k].tobytes():
                    served.append(int(k))
            print(f"linspace {name} window {j} [{lo:.6g}, {hi:.6g}]: bins {served[0]} .. {served[-1]} ({len(served)}) bitwise np.linspace")
            assert set(range(k_lo, k_hi + 1)) <= set(served), (name, j, served)


def test_at_most_one_window_of_this_file_was_flagged():
    print(f"flagged zoom windows: {FLAGGED_WINDOWS}")
    assert len(FLAGGED_WINDOWS) <= 1


def test_total_time_of_this_file():
    print(f"tests/test_gpu_ground_pick.py: {time.perf_counter() - T0:.2f} s from import to the last test")
