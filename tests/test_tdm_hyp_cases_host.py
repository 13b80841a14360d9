"""TDM-MIMO velocity unwrapping without a GPU: the ABI, the hypothesis table and its duplicates, the physics of the
decision over the whole extended Doppler range, the host twin of the float64 stage against the NumPy oracle
(tests/tdm_hyp_cases.py), crafted ties, the integer rules and the validation of the options."""
import os
import re

import numpy as np
import pytest

import tdm_cases as tc
import tdm_hyp_cases as hc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib, batch

from test_tdm_cases_host import FakeContext, host_twin as tdm_host_twin, make_cm

ENTRIES = {"mmw_angle_argmax_tdm_hyp": 21, "mmw_angle_argmax_cells64_tdm_hyp": 13, "mmw_diag_angle_argmax_tdm_hyp_host": 12,
           "mmw_tdm_unwrap_velocity": 10}
SENTINEL = -7


def host_twin(cells, cols, table, A, shift, given=None):
    """(indices, hypotheses) of mmw_diag_angle_argmax_tdm_hyp_host; given: the hypotheses handed in (they come back untouched)."""
    lib = _lib.load_library()
    cells = np.ascontiguousarray(cells, dtype=np.complex128)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.complex128)
    idx = np.full(cells.shape[0], SENTINEL, dtype=np.int32)
    hyp = np.full(cells.shape[0], SENTINEL, dtype=np.int32) if given is None else np.ascontiguousarray(given, dtype=np.int32).copy()
    _lib.check(lib.mmw_diag_angle_argmax_tdm_hyp_host(cells.ctypes.data, cols.ctypes.data, table.ctypes.data, table.shape[0],
                                                      idx.ctypes.data, hyp.ctypes.data, int(given is not None), cells.shape[0],
                                                      cells.shape[1], table.shape[2], A, int(shift)))
    return idx, hyp


# ------------------------------------------------------------------ ABI
def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    make = open(os.path.join(ROOT, "mmwave_radar_processing_amd", "csrc", "Makefile")).read()
    lib = _lib.load_library()
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, f"{name} is not declared in include/mmwgpu.h"
        assert decl.group(1).count(",") + 1 == n_args == len(_lib._SIGNATURES[name])
        assert name in _lib.EXPORTED and getattr(lib, name).argtypes == _lib._SIGNATURES[name]
    assert re.search(r"^UNITS = .*\bmmw_tu_tdm_hyp\b", make, flags=re.M)
    assert re.search(r"^build/mmw_tu_tdm_hyp\.o: CXXFLAGS \+= -ffp-contract=off", make, flags=re.M)


# ------------------------------------------------------------------ table
@pytest.mark.parametrize("V,num_rx,C", [(12, 4, 16), (12, 4, 7), (8, 4, 10), (12, 4, 128)])
def test_table_is_the_formula_and_hypothesis_zero_is_the_phase_table(V, num_rx, C):
    slots, n_slots = tc.default_slots(V, num_rx)
    ant = list(range(V)) + [-1]
    t = batch.tdm_hypothesis_table(ant, slots, n_slots, C)
    assert t.dtype == np.complex128 and t.shape == (n_slots, len(ant), C) and t.flags.c_contiguous
    assert t[0].tobytes() == batch.tdm_phase_table(ant, slots, n_slots, C).tobytes()
    if C <= 16:
        assert t.tobytes() == hc.hypothesis_formula(ant, slots, n_slots, C).tobytes()
    assert np.all(t[:, :num_rx] == 1.0)                      # slot 0 under every hypothesis
    assert t[:, -1].tobytes() == t[:, -2].tobytes()          # -1 is the last antenna
    M = n_slots * C
    exact = np.exp(-2j * np.pi * ((np.arange(C) - C // 2)[None, None, :] + np.arange(n_slots)[:, None, None] * C) *
                   np.asarray(slots)[ant][None, :, None] / M)
    assert np.max(np.abs(t - exact)) <= 1e-12                # (the unreduced phase, to what its size costs)


def test_table_with_a_gap_in_the_slot_list():
    slots = [0, 0, 2, 2, 3, 3]                               # n_slots = 4, slot 1 unused
    for C in (7, 16):
        t = batch.tdm_hypothesis_table(range(6), slots, 4, C)
        assert t[0].tobytes() == batch.tdm_phase_table(range(6), slots, 4, C).tobytes()
        assert t.tobytes() == hc.hypothesis_formula(list(range(6)), slots, 4, C).tobytes()


def test_duplicates():
    slots, n_slots = tc.default_slots(12, 4)
    # a list inside one slot: every hypothesis is a common phase, one distinct hypothesis
    for ant in ([8, 9, 10, 11], [4, 5], [0, 1, 2, 3], [7]):
        t = batch.tdm_hypothesis_table(ant, slots, n_slots, 16)
        assert batch.tdm_distinct_hypotheses(t) == [0, 0, 0] == hc.representatives(t)
    # lists over two and three slots: all three distinct
    for ant in (list(range(8)), list(range(12)), [3, 8]):
        t = batch.tdm_hypothesis_table(ant, slots, n_slots, 16)
        assert batch.tdm_distinct_hypotheses(t) == [0, 1, 2] == hc.representatives(t)
    # slots {0, 2} of four: h = 2 duplicates h = 0 (and h = 3 duplicates h = 1) bit for bit
    slots4 = [0, 0, 1, 1, 2, 2, 3, 3]
    for C in (7, 16):
        t = batch.tdm_hypothesis_table([0, 1, 4, 5], slots4, 4, C)
        assert t[2].tobytes() == t[0].tobytes() and t[3].tobytes() == t[1].tobytes() and t[1].tobytes() != t[0].tobytes()
        assert batch.tdm_distinct_hypotheses(t) == [0, 1, 0, 1] == hc.representatives(t)
        cells, cols = random_case(3, 50, 4, C)
        idx, hyp = host_twin(cells, cols, t, 16, 1)
        assert set(np.unique(hyp)) <= {0, 1}
        # a given duplicate is evaluated as the hypothesis it duplicates
        for h in (0, 1):
            a, _ = host_twin(cells, cols, t, 16, 1, given=np.full(50, h))
            b, _ = host_twin(cells, cols, t, 16, 1, given=np.full(50, h + 2))
            assert np.array_equal(a, b)


# ------------------------------------------------------------------ physics
@pytest.mark.parametrize("loops", [16, 10, 7])
def test_every_true_bin_of_the_extended_range_is_recovered(loops):
    """4 rx x 3 tx, S = 16, azimuth list [0..7], one noiseless target on every true Doppler bin of [-M // 2, M - M // 2) and three
    spatial frequencies: the oracle and the host twin both return k' = the true bin and an angle bin within 1 of truth, and the
    oracle excludes none (the smallest gap between the best and the second hypothesis measured on this rig is 0.12)."""
    num_rx, num_tx, S, A = 4, 3, 16, 64
    slots, n_slots = tc.default_slots(num_rx * num_tx, num_rx)
    az = list(range(8))
    table = batch.tdm_hypothesis_table(az, slots, n_slots, loops)
    M = num_tx * loops
    cells, cols, truth, bins = [], [], [], []
    for seed in (40, 41, 42):
        for kd in range(-(M // 2), M - M // 2):
            cube, det, true_bin = hc.physics_scene(seed, kd, num_rx, num_tx, S, loops, A=A, shift=True)
            cells.append(tc.cells_of(cube, [det])[0, az])
            cols.append(det[1])
            truth.append(kd)
            bins.append(true_bin)
    cells, cols, truth, bins = np.array(cells), np.array(cols), np.array(truth), np.array(bins)
    idx, hyp, decided = hc.oracle(cells, cols, table, A, True)
    assert decided.all()
    t_idx, t_hyp = host_twin(cells, cols, table, A, True)
    for got_idx, got_hyp in ((idx, hyp), (t_idx, t_hyp)):
        assert np.array_equal(batch.tdm_unwrapped_bin(cols, got_hyp, n_slots, loops), truth)
        d = np.abs(got_idx - bins)
        assert np.all(np.minimum(d, A - d) <= 1)
    # without the hypotheses a folded target gets the wrong factor: bearings off for many of them
    plain, _ = tc.oracle_argmax(cells, cols, table[0], A, True)
    folded = hyp != 0
    assert folded.sum() >= len(truth) // 2 and np.mean(plain[folded] != idx[folded]) >= 0.5


# ------------------------------------------------------------------ host twin == oracle
def random_case(seed, n_rows, n_ant, C):
    rng = np.random.default_rng(seed)
    cells = rng.standard_normal((n_rows, n_ant)) + 1j * rng.standard_normal((n_rows, n_ant))
    cells *= 10.0 ** rng.uniform(-3, 3, (n_rows, 1))
    return cells, rng.integers(0, C, n_rows)


@pytest.fixture(scope="module", params=[(12, 16, 16), (12, 16, 7)], ids=lambda s: "x".join(map(str, s)))
def noisy_cells(request):
    """complex128 cells (N, 12) and columns of random detection lists over noisy scenes with folded targets."""
    shape = request.param
    cubes = hc.noisy_scene(7, shape, 3)
    dets, _ = tc.detection_lists(8, shape, [60, 60, 60], 60)
    cells = np.concatenate([tc.cells_of(cubes[f], dets[f]) for f in range(3)])
    return shape, cells, dets[..., 1].reshape(-1)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [64, 16])
def test_host_twin_equals_oracle_on_noisy_scenes(noisy_cells, A, shift):
    shape, cells, cols = noisy_cells
    slots, n_slots = tc.default_slots(12, 4)
    for ant in (list(range(8)), list(range(12)), [2, 3, 4, 5]):
        table = batch.tdm_hypothesis_table(ant, slots, n_slots, shape[2])
        idx, hyp, decided = hc.oracle(cells[:, ant], cols, table, A, shift)
        assert 1.0 - decided.mean() <= 0.01                  # a condition on the chosen seeds, checked with the oracle alone
        t_idx, t_hyp = host_twin(cells[:, ant], cols, table, A, shift)
        assert np.array_equal(t_idx[decided], idx[decided]) and np.array_equal(t_hyp[decided], hyp[decided])
        assert len(np.unique(hyp)) == n_slots                # every hypothesis wins somewhere
        # the hypothesis given: the deciding call's own index, and the index of any other hypothesis
        g_idx, g_hyp = host_twin(cells[:, ant], cols, table, A, shift, given=t_hyp)
        assert np.array_equal(g_idx, t_idx) and np.array_equal(g_hyp, t_hyp)
        other = (t_hyp + 1) % n_slots
        o_idx, _, o_dec = hc.oracle(cells[:, ant], cols, table, A, shift, given=other)
        g_idx, g_hyp = host_twin(cells[:, ant], cols, table, A, shift, given=other)
        assert np.array_equal(g_idx[o_dec], o_idx[o_dec]) and np.array_equal(g_hyp, other)
        assert 1.0 - o_dec.mean() <= 0.01


# ------------------------------------------------------------------ crafted
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
def test_host_twin_on_crafted_cells(A, shift):
    slots, n_slots = tc.default_slots(12, 4)
    C = 10
    ant = list(range(8))
    table = batch.tdm_hypothesis_table(ant, slots, n_slots, C)
    cols = np.arange(C)
    rng = np.random.default_rng(5)
    # cells non-zero only on slot-0 antennas: every hypothesis sees the same cells bit for bit, an exact tie, h* = 0
    tie = np.zeros((C, 8), dtype=np.complex128)
    tie[:, :4] = rng.standard_normal((C, 4)) + 1j * rng.standard_normal((C, 4))
    idx, hyp = host_twin(tie, cols, table, A, shift)
    assert np.all(hyp == 0) and np.array_equal(idx, tdm_host_twin(tie, cols, table[0], A, shift))
    o_idx, o_hyp, decided = hc.oracle(tie, cols, table, A, shift)
    assert np.all(o_hyp == 0) and np.array_equal(idx[decided], o_idx[decided]) and decided.mean() >= 0.9
    # one NaN cell: every bin of every hypothesis is NaN, the first of both wins
    nan = np.ones((C, 8), dtype=np.complex128)
    nan[:, 6] = np.nan
    idx, hyp = host_twin(nan, cols, table, A, shift)
    assert np.all(idx == 0) and np.all(hyp == 0)
    o_idx, o_hyp, decided = hc.oracle(nan, cols, table, A, shift)
    assert decided.all() and np.all(o_idx == 0) and np.all(o_hyp == 0)
    # hypotheses given out of range are clamped; the values handed in come back untouched
    cells, cc = random_case(9, 40, 8, C)
    given = np.array([-5, -1, 0, 1, 2, 3, 99, 2 ** 31 - 1] * 5)
    g_idx, g_hyp = host_twin(cells, cc, table, A, shift, given=given)
    c_idx, _ = host_twin(cells, cc, table, A, shift, given=np.clip(given, 0, n_slots - 1))
    assert np.array_equal(g_idx, c_idx) and np.array_equal(g_hyp, given.astype(np.int32))
    o_idx, _, o_dec = hc.oracle(cells, cc, table, A, shift, given=given)
    assert np.array_equal(g_idx[o_dec], o_idx[o_dec])


def test_host_twin_on_one_antenna_and_one_bin():
    slots, n_slots = tc.default_slots(12, 4)
    C = 9
    cells, cols = random_case(2, 30, 1, C)
    for ant in ([0], [5], [11]):                             # one antenna: one slot, one distinct hypothesis
        table = batch.tdm_hypothesis_table(ant, slots, n_slots, C)
        for A in (1, 16):
            idx, hyp = host_twin(cells, cols, table, A, 0)
            assert np.all(hyp == 0) and np.all(idx == 0)     # |y_0 W^0| in every bin: the first wins
    # A = 1 with nothing else is refused for longer lists (n_ant <= A), as in the compensated entry
    table = batch.tdm_hypothesis_table([0, 4], slots, n_slots, C)
    with pytest.raises(ValueError):
        host_twin(np.ones((3, 2)), [0, 1, 2], table, 1, 0)
    with pytest.raises(ValueError):                          # H > 8
        host_twin(np.ones((3, 2)), [0, 1, 2], np.ones((9, 2, C)), 16, 0)


# ------------------------------------------------------------------ integers
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("C", [7, 8, 16])
def test_unwrapped_bin_against_brute_force(n, C):
    M = n * C
    window = list(range(-(M // 2), M - M // 2))
    assert len(window) == M
    for c in range(C):
        k = c - C // 2
        for h in range(n):
            want = [q for q in window if (q - (k + h * C)) % M == 0]
            assert len(want) == 1
            got = batch.tdm_unwrapped_bin(c, h, n, C)
            assert isinstance(got, int) and got == want[0] == int(hc.unwrapped_bin(c, h, n, C))
            assert (got - k) % C == 0 and abs((got - k) // C) <= (n + 1) // 2
            assert int(hc.fold_count(c, h, n, C)) == (got - k) // C
        assert batch.tdm_unwrapped_bin(c, 0, n, C) == k      # h = 0: the bin itself
    cols, hyps = np.meshgrid(np.arange(C), np.arange(n))
    assert np.array_equal(batch.tdm_unwrapped_bin(cols, hyps, n, C), hc.unwrapped_bin(cols, hyps, n, C))
    # every bin of the window is reached exactly once
    assert sorted(batch.tdm_unwrapped_bin(cols, hyps, n, C).ravel().tolist()) == window


def test_velocity_rule_keeps_the_bits_of_unfolded_slots():
    n, C, span = 3, 16, 7.25
    vel = np.array([-0.0, 0.0, 1.5, -3.625, np.nan, 2.0 ** -1074])
    c = np.array([8, 8, 11, 3, 9, 8])
    same = hc.unwrapped_velocity(vel, c, np.zeros(6, dtype=int), n, C, span)
    assert same.tobytes() == vel.tobytes()                   # (-0.0 stays -0.0)
    got = hc.unwrapped_velocity(vel, c, np.array([0, 1, 2, 1, 0, 2]), n, C, span)
    m = hc.fold_count(c, np.array([0, 1, 2, 1, 0, 2]), n, C)
    assert m.tolist() == [0, 1, -1, 1, 0, -1]
    assert got[0].tobytes() == vel[0].tobytes() and got[4].tobytes() == vel[4].tobytes()
    assert np.array_equal(got[[1, 2, 3, 5]], vel[[1, 2, 3, 5]] + m[[1, 2, 3, 5]] * span)


# ------------------------------------------------------------------ options
def test_options_are_validated():
    cm = make_cm()
    shape = (12, 16, 8)
    common = dict(ctx=FakeContext(), az_antenna_idxs=list(range(8)), el_antenna_idxs=[8, 9, 10, 11])
    with pytest.raises(ValueError):                          # unwrapping without the compensation
        batch.FramePipeline(cm, 2, shape, tdm_velocity_unwrap=True, **common)
    for bad in ("el", [8, 9, 10, 11], [5], [], "both", 3, [0, 0, 4], [0, 12], [0.5, 4]):
        with pytest.raises(ValueError):                      # inside one slot / no list of antennas
            batch.FramePipeline(cm, 2, shape, tdm_compensation=True, tdm_velocity_unwrap=True, tdm_hypothesis_list=bad, **common)
    with pytest.raises(ValueError):                          # nine slots: more hypotheses than the entry evaluates
        batch.FramePipeline(cm, 2, shape, tdm_compensation=True, tdm_velocity_unwrap=True, tdm_tx_slots=list(range(9)) + [0] * 3,
                            **common)
    p = batch.FramePipeline(cm, 2, shape, tdm_compensation=True, tdm_velocity_unwrap=True, **common)
    assert p.tdm_velocity_unwrap is True and p.tdm_hyp_list == ("az", list(range(8)))
    q = batch.FramePipeline(cm, 2, shape, tdm_compensation=True, tdm_velocity_unwrap=True, tdm_hypothesis_list=[3, 4, -1], **common)
    assert q.tdm_hyp_list == ("list", [3, 4, -1])
    r = batch.FramePipeline(cm, 2, shape, tdm_compensation=True, tdm_velocity_unwrap=True, tdm_hypothesis_list="el",
                            ctx=FakeContext(), az_antenna_idxs=[0, 1], el_antenna_idxs=[3, 7, 11])
    assert r.tdm_hyp_list == ("el", [3, 7, 11])
    off = batch.FramePipeline(cm, 2, shape, tdm_compensation=True, **common)
    assert off.tdm_velocity_unwrap is False and off.tdm_hyp_list is None
    with pytest.raises(ValueError):
        off.tdm_hypotheses()
    from mmwave_radar_processing_amd.processors import PointCloudGenerator
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, list(range(8)), [8, 9, 10, 11], tdm_velocity_unwrap=True)
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, list(range(8)), [8, 9, 10, 11], tdm_compensation=True, tdm_velocity_unwrap=True,
                            tdm_hypothesis_list="el")
    with pytest.raises(ValueError):
        batch.tdm_hypothesis_table([12], [0] * 12, 3, 8)
    with pytest.raises(ValueError):
        batch.tdm_unwrapped_bin(0, 0, 0, 8)
