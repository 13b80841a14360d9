"""The crafted picker rows of tests/ground_pick_cases.py, proved without a GPU: every variant's MEASURED distance lies where its
name says, the reference alone decides every row the device must decide (its answer survives a +-1e-12 dB change of 20 log10 p,
the device / host log10 bound of mmw_ground.h), the two far sides of a decision give two different answers, and the rows hold
what their builders promise (plateau midpoints, 512 / 513 peaks, no peak at all)."""
import numpy as np
import pytest
from scipy.signal import find_peaks

import ground_pick_cases as G
from mmwave_radar_processing_amd import _lib

CASES = G.all_cases()
BY_NAME = {c.name: c for c in CASES}


def test_names_are_unique_and_every_decision_has_its_variants():
    assert len(BY_NAME) == len(CASES)
    for d in ("rise", "fall", "walk_stop", "lb_rb", "order_last_in_m2", "order_last_in_m3", "order_top_m2", "order_top_m3"):
        assert {c.variant for c in CASES if c.decision == d} == set(G.VARIANTS), d
    for d in ("plateau_tail", "prominence_6dB", "cut_20dB"):                # no bitwise-equal form of these
        assert {c.variant for c in CASES if c.decision == d} == set(G.VARIANTS) - {"equal"}, d
    assert sorted(G.cases_by_length()) == [3, 64, 255, 256, 257, 1025, 1027, 3072]


@pytest.mark.parametrize("case", [c for c in CASES if c.dist is not None], ids=lambda c: c.name)
def test_measured_distance_lies_where_the_variant_says(case):
    d = np.atleast_1d(case.dists if case.dists is not None else case.dist) / G.BAND
    v = case.variant
    if v == "equal":
        assert np.all(d == 0.0)
    elif v.startswith("near"):
        assert np.all(np.abs(d) <= 0.25) and np.all(np.sign(d) == (1 if v[-1] == "+" else -1)), d
        assert case.flagged
    else:
        assert np.all((np.abs(d) >= 7.0) & (np.abs(d) <= 9.0)) and np.all(np.sign(d) == (1 if v[-1] == "+" else -1)), d
        assert not case.flagged


def test_the_band_leaves_room_for_the_variants():
    assert 8e-9 * np.log(10) / 20 > 1e6 * np.finfo(np.float64).eps              # a far step in p is far above one ulp
    assert G.LOG10_BOUND * 1000 == pytest.approx(G.BAND) and G.NEAR < G.BAND / 4 < G.BAND < G.FAR


@pytest.mark.parametrize("case", [c for c in CASES if not c.flagged and not c.nonfinite], ids=lambda c: c.name)
def test_reference_alone_decides_every_unflagged_row(case):
    for m in case.max_peaks:
        want = G.reference(G.to_db(case.p), m)
        for seed in (-1, 0, 1, 2):
            np.testing.assert_array_equal(G.reference(G.perturbed(case.p, seed), m), want, err_msg=f"{case.name} m {m} seed {seed}")


def test_far_sides_give_two_different_answers():
    decisions = sorted({c.decision for c in CASES if c.variant == "far-"})
    assert len(decisions) >= 11
    for d in decisions:
        lo, hi = BY_NAME[f"{d}/far-"], BY_NAME[f"{d}/far+"]
        for m in lo.max_peaks:
            a, b = G.reference(G.to_db(lo.p), m), G.reference(G.to_db(hi.p), m)
            assert np.array_equal(a, b) != lo.changes, (d, m, a, b)
    assert [d for d in decisions if not BY_NAME[f"{d}/far-"].changes] == ["lb_rb"]    # the base changes, the peak does not


def idx(name, m=3):
    return G.reference(G.to_db(BY_NAME[name].p), m).tolist()


def test_rows_hold_what_their_builders_promise():
    assert [idx(f"plateau{n}/equal") for n in (2, 3, 4)] == [[20], [21], [21]]             # (i + r - 1) / 2
    assert idx("rise/equal") == [19] and idx("rise/far+") == [20] and idx("rise/far-") == [19]
    assert idx("fall/far+") == [19] and idx("fall/far-") == [20]
    assert idx("plateau_tail/far-") == [21] and idx("plateau_tail/far+") == [23]
    assert idx("plateau_first") == idx("plateau_last") == []
    assert idx("maxima_at_1_and_S-2") == [1, 62]
    assert idx("walk_stop/far+") == [21] and idx("walk_stop/far-") == [30]
    assert idx("equal_minima/equal") == [30] and idx("lb_rb/equal") == [30]
    assert idx("higher_base_left") == idx("higher_base_right") == []
    assert idx("prominence_6dB/far-") == [] and idx("prominence_6dB/far+") == [30]
    assert idx("cut_20dB/far-") == [20] and idx("cut_20dB/far+") == [20, 40]
    assert idx("order_last_in_m2/far-", 2) == [8, 16] and idx("order_last_in_m2/far+", 2) == [8, 24]
    assert idx("order_last_in_m3/far-") == [8, 16, 24] and idx("order_last_in_m3/far+") == [8, 16, 32]
    assert idx("order_top_m2/far-", 2) == [8, 16] and idx("order_top_m3/far+") == [16, 8, 24]
    assert idx("order_tie_behind_m2/equal", 2) == [8, 16] and idx("order_tie_behind_m3/equal") == [8, 16, 24]
    for name in ("constant", "monotone", "three_without", "all_zero"):
        assert idx(name) == [], name
    assert idx("three_with") == [1]
    assert idx("zeros_both_bases") == idx("zeros_left_base") == [30]                        # scipy on -inf: a base like any other
    for n, S in ((512, 1025), (513, 1027)):
        c = BY_NAME[f"sawtooth_{n}"]
        peaks, props = find_peaks(G.to_db(c.p), prominence=6)
        assert c.S == S and len(peaks) == n and props["prominences"].min() >= 30.0 and c.flagged == (n > G.PEAK_LIST)
    assert len(idx("sawtooth_512")) == 3
    for v, at in (("far-", 19), ("far+", 20)):
        c = BY_NAME[f"tiled_rise_S3072/{v}"]
        peaks, _ = find_peaks(G.to_db(c.p), prominence=6)
        assert c.S == 3072 and peaks.tolist() == list(range(at, 3072, 64)) and len(c.dists) == 48
        assert idx(c.name) == [47 * 64 + at, 46 * 64 + at, 45 * 64 + at]
    for S in (255, 256, 257, 1025, 1027, 3072):
        assert idx(f"generic_S{S}") == [1, S - 2, S // 2] and idx(f"generic_S{S}", 2) == [1, S - 2]
        # the noisy floor holds many local maxima, none of them close to the 6 dB prominence or to a neighbour
        y = G.to_db(BY_NAME[f"generic_S{S}"].p)
        _, props = find_peaks(y, prominence=0)
        assert len(props["prominences"]) > S // 5 and np.min(np.abs(props["prominences"] - 6.0)) > 1e-3
        assert np.min(np.abs(np.diff(y))) > 100 * G.BAND
    ties = [c.name for c in CASES if c.flagged and c.variant == "equal"]
    assert sorted(ties) == ["order_last_in_m2/equal", "order_last_in_m3/equal", "order_top_m2/equal", "order_top_m3/equal",
                            "walk_stop/equal"]
    assert sum(c.nonfinite for c in CASES) == 8 and all(not np.all(np.isfinite(c.p)) for c in CASES if c.nonfinite)


def test_entry_is_declared_bound_and_leaves_the_abi_revision():
    assert "mmw_diag_ground_pick" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_diag_ground_pick"]) == 8
    lib = _lib.load_library()
    assert hasattr(lib, "mmw_diag_ground_pick") and lib.mmw_abi_version() == _lib.ABI_VERSION == 7
