"""The inputs and references of tests/cfar_cases.py, checked without a GPU.

1. The local references (explicit scale / k_rank, as the C ABI takes them) equal oracle/oracle_np.py's when the scale and
   the rank are the ones the oracle derives from pfa / rho.
2. The inputs really hold what test_gpu_cfar_edges.py needs them for, by the reference alone: cells that EQUAL their
   threshold (so a `>=` for the strict `>` or an off-by-one rank changes the mask), and windows whose order statistic
   is a NaN, is finite beside a NaN, is +inf, or whose two side means are NaN on one side only.
"""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import cfar_cases as cc
from oracle import oracle_np as O

TIE_FLOOR, DET_FLOOR, LOST_FLOOR = 16, 8, 8


def _dets(mask):
    return [tuple(map(int, t)) for t in zip(*np.where(mask))]


def test_references_equal_the_oracle_2d():
    rng = np.random.default_rng(11)
    X = rng.exponential(1.0, (45, 70)) * 1e3
    X[rng.integers(0, 45, 12), rng.integers(0, 70, 12)] *= 40
    for train, guard in cc.OS_WINDOWS + [w[:2] for w in cc.CA_WINDOWS[:3]]:
        n = cc.n_train_2d(train, guard)
        for pfa in (1e-3, 1e-5):
            ref = O.ca_cfar_2d(X, train, guard, pfa)
            thr, noise, mask = cc.ref_cfar2d(X, cc.CA, train, guard, O.alpha_ca(n, pfa))
            np.testing.assert_array_equal(thr, ref[0])
            np.testing.assert_array_equal(noise, ref[1])
            assert _dets(mask) == ref[2]
        for rho, alpha in ((0.7, 3.0), (0.5, 2.0)):
            ref = O.os_cfar_2d(X, train, guard, rho, alpha)
            thr, noise, mask = cc.ref_cfar2d(X, cc.OS, train, guard, alpha, O.os_k_rank(rho, n))
            np.testing.assert_array_equal(thr, ref[0])
            np.testing.assert_array_equal(noise, ref[1])
            assert _dets(mask) == ref[2]
    assert len(O.ca_cfar_2d(X, (4, 4), (2, 2), 1e-3)[2]) > 0


def test_references_equal_the_oracle_1d():
    rng = np.random.default_rng(12)
    x = rng.exponential(1.0, 700)
    x[rng.integers(0, 700, 9)] *= 30
    for T, G in cc.WINDOWS_1D[:5] + [(5, 3)]:
        for kind, fn, n in ((cc.CA, O.ca_cfar_1d, 2 * T), (cc.GO, O.go_cfar_1d, T), (cc.SO, O.so_cfar_1d, T)):
            ref = fn(x, T, G, 1e-3)
            thr, noise, mask = cc.ref_cfar1d(x, kind, T, G, O.alpha_ca(n, 1e-3))
            np.testing.assert_array_equal(thr, ref[0])
            np.testing.assert_array_equal(noise, ref[1])
            assert np.where(mask)[0].tolist() == ref[2]
        ref = O.os_cfar_1d(x, T, G, 0.6, 2.5)
        thr, noise, mask = cc.ref_cfar1d(x, cc.OS, T, G, 2.5, O.os_k_rank(0.6, 2 * T))
        np.testing.assert_array_equal(thr, ref[0])
        np.testing.assert_array_equal(noise, ref[1])
        assert np.where(mask)[0].tolist() == ref[2]
    # a row shorter than the window: nothing valid
    thr, noise, mask = cc.ref_cfar1d(x[:8], cc.CA, 3, 1, 1.0)
    assert np.all(np.isinf(thr)) and not noise.any() and not mask.any()


@pytest.mark.parametrize("train,guard", cc.OS_WINDOWS)
def test_quantised_planes_hold_ties_2d(train, guard):
    """The tie case of every OS window: the quantised plane at the median rank with scale 1.0."""
    shape = cc.os_plane_shape(train, guard)
    X = cc.quantised(shape, cc.OS_LEVELS[(train, guard)], cc.OS_SEED)
    k = max(1, cc.n_train_2d(train, guard) // 2)
    assert k in cc.os_ranks_2d(train, guard)
    thr, _, mask = cc.ref_cfar2d(X, cc.OS, train, guard, 1.0, k)
    ties, dets, lost = cc.tie_stats(X, thr, mask)
    print(train, guard, "k", k, "ties", ties, "detections", dets, "lost to strictness", lost)
    assert ties >= TIE_FLOOR and dets >= DET_FLOOR and lost >= LOST_FLOOR


@pytest.mark.parametrize("T,G", cc.WINDOWS_1D)
def test_quantised_rows_hold_ties_1d(T, G):
    x = cc.rows_1d(T, G)[0]
    thr, _, mask = cc.ref_cfar1d(x, cc.OS, T, G, 1.0, T)
    ties, dets, lost = cc.tie_stats(x, thr, mask)
    print(T, G, "ties", ties, "detections", dets, "lost to strictness", lost)
    assert ties >= TIE_FLOOR and dets >= DET_FLOOR and lost >= LOST_FLOOR


def test_constant_inputs_sit_on_the_threshold_for_every_kind():
    for train, guard, shape in cc.CA_WINDOWS:
        X = cc.constant(shape)
        n_valid = (shape[0] - 2 * (train[0] + guard[0])) * (shape[1] - 2 * (train[1] + guard[1]))
        thr, noise, mask = cc.ref_cfar2d(X, cc.CA, train, guard, 1.0)
        assert cc.tie_stats(X, thr, mask) == (n_valid, 0, n_valid)
        thr, noise, mask = cc.ref_cfar2d(X, cc.CA, train, guard, cc.JUST_BELOW_ONE)
        assert int(mask.sum()) == n_valid
    for train, guard in cc.OS_WINDOWS:
        shape = cc.os_plane_shape(train, guard)
        X = cc.constant(shape)
        n_valid = (shape[0] - 2 * (train[0] + guard[0])) * (shape[1] - 2 * (train[1] + guard[1]))
        for k in cc.os_ranks_2d(train, guard):
            thr, noise, mask = cc.ref_cfar2d(X, cc.OS, train, guard, 1.0, k)
            assert cc.tie_stats(X, thr, mask) == (n_valid, 0, n_valid)
            assert int(cc.ref_cfar2d(X, cc.OS, train, guard, cc.JUST_BELOW_ONE, k)[2].sum()) == n_valid
    for T, G in cc.WINDOWS_1D:
        x = cc.constant(cc.ROW_LEN)
        n_valid = cc.ROW_LEN - 2 * (T + G)
        for kind in (cc.CA, cc.OS, cc.GO, cc.SO):
            thr, noise, mask = cc.ref_cfar1d(x, kind, T, G, 1.0, T)
            assert cc.tie_stats(x, thr, mask) == (n_valid, 0, n_valid)
            assert int(cc.ref_cfar1d(x, kind, T, G, cc.JUST_BELOW_ONE, T)[2].sum()) == n_valid


def _os_conditions(noise_by_rank, has_nan):
    """Which of (k-th is NaN, k-th finite beside a NaN, k-th is +inf) some window meets at some rank."""
    met = [False, False, False]
    for est in noise_by_rank:
        met[0] |= bool(np.any(np.isnan(est)))
        met[1] |= bool(np.any(np.isfinite(est) & has_nan))
        met[2] |= bool(np.any(est == np.inf))
    return met


@pytest.mark.parametrize("train,guard", cc.OS_WINDOWS)
def test_nonfinite_plane_reaches_every_os_condition_2d(train, guard):
    shape = cc.os_plane_shape(train, guard)
    hr, hd = train[0] + guard[0], train[1] + guard[1]
    X, plants = cc.nonfinite(shape, cc.OS_SEED + 1, (hr, hd))
    assert set(plants) == set(cc.PLANT_KINDS)
    for r, c in plants.values():                  # every plant is a cell under test of this window
        assert hr <= r < shape[0] - hr and hd <= c < shape[1] - hd
    assert np.signbit(X[plants["neg_nan"]]) and np.isnan(X[plants["neg_nan"]]) and not np.signbit(X[plants["nan"]])
    mask, wr, wd = cc.mask_2d(train, guard)
    has_nan = np.isnan(sliding_window_view(X, (wr, wd))[..., mask]).any(axis=-1)
    ests = [cc.ref_cfar2d(X, cc.OS, train, guard, 1.0, k)[1][hr:shape[0] - hr, hd:shape[1] - hd]
            for k in cc.os_ranks_2d(train, guard)]
    assert _os_conditions(ests, has_nan) == [True, True, True]


@pytest.mark.parametrize("T,G", cc.WINDOWS_1D)
def test_nonfinite_row_reaches_every_condition_1d(T, G):
    x = cc.rows_1d(T, G)[4]
    half, L = T + G, cc.ROW_LEN
    win = sliding_window_view(x, 2 * half + 1)
    has_nan = np.isnan(np.concatenate((win[:, :T], win[:, T + 2 * G + 1:]), axis=1)).any(axis=1)
    ests = [cc.ref_cfar1d(x, cc.OS, T, G, 1.0, k)[1][half:L - half] for k in cc.os_ranks_1d(T)]
    assert _os_conditions(ests, has_nan) == [True, True, True]
    ml, mr = cc.side_means_1d(x, T, G)
    one_side = np.isnan(ml) != np.isnan(mr)
    assert one_side.any()
    for kind in (cc.GO, cc.SO):                      # and there the reference's estimate is the NaN, not the number
        est = cc.ref_cfar1d(x, kind, T, G, 1.0)[1][half:L - half]
        assert np.all(np.isnan(est[one_side]))


def test_nonfinite_guard_cells_poison_the_2d_ca_sum():
    train, guard = (4, 4), (2, 2)
    X, plants = cc.nonfinite(cc.PLANE_A, 5, (6, 6))
    thr, noise, mask = cc.ref_cfar2d(X, cc.CA, train, guard, 2.0)
    for kind in ("pos_inf", "neg_inf", "nan", "neg_nan"):
        assert np.isnan(noise[plants[kind]]) and mask[plants[kind]] == 0
    assert np.isfinite(noise[plants["subnormal"]])
    assert np.any(np.isinf(thr[6:-6, 6:-6]))          # the 1e308 cluster overflows a sum or scale * est


def test_builders_are_seeded_and_exact():
    a, b = cc.quantised((45, 70), 8, 3), cc.quantised((45, 70), 8, 3)
    np.testing.assert_array_equal(a, b)
    assert np.all(a == np.round(a)) and a.min() == 0 and a.max() <= 28
    r = cc.ramp((5, 7))
    assert r[2, 3] == 2 * 7 + 3 and len(np.unique(r)) == 35
    assert cc.rows_1d(3, 1).shape == (5, cc.ROW_LEN)
    assert cc.planes_2d((45, 70), 8, 1, (6, 6)).shape == (4, 45, 70)
