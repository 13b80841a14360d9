"""TDM-MIMO Doppler phase compensation without a GPU: the ABI, the phase table, the host twin of the float64 stage against the
NumPy oracle (tests/tdm_cases.py), the physics of the compensation on synthetic TDM scenes, the derived bound of the float32
phasor product, and the validation of the options."""
import ctypes
import os
import re

import numpy as np
import pytest

import tdm_cases as tc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib, batch, synth
from mmwave_radar_processing_amd.config_managers import ConfigManager

ENTRIES = ("mmw_angle_argmax_tdm", "mmw_angle_argmax_cells64_tdm", "mmw_diag_angle_argmax_tdm_host")


def host_twin(cells, cols, table, A, shift):
    lib = _lib.load_library()
    cells = np.ascontiguousarray(cells, dtype=np.complex128)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.complex128)
    out = np.full(cells.shape[0], -7, dtype=np.int32)
    _lib.check(lib.mmw_diag_angle_argmax_tdm_host(cells.ctypes.data, cols.ctypes.data, table.ctypes.data, out.ctypes.data,
                                                  cells.shape[0], cells.shape[1], table.shape[1], A, int(shift)))
    return out


# ------------------------------------------------------------------ ABI
def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    lib = _lib.load_library()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), f"{name} is not declared in include/mmwgpu.h"
        assert name in _lib._SIGNATURES and name in _lib.EXPORTED
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name]
    assert len(_lib._SIGNATURES["mmw_angle_argmax_tdm"]) == len(_lib._SIGNATURES["mmw_angle_argmax_exact"]) + 1
    assert re.search(r"#define MMWGPU_ABI_VERSION 7\b", header)
    lib.mmw_abi_version.restype = ctypes.c_int
    assert lib.mmw_abi_version() == 7 == _lib.ABI_VERSION


# ------------------------------------------------------------------ phase table
@pytest.mark.parametrize("C", [8, 9, 10, 128])
def test_phase_table_is_the_formula(C):
    slots, n_slots = tc.default_slots(12, 4)
    ant = [0, 3, 4, 7, 8, 11, -1]
    t = batch.tdm_phase_table(ant, slots, n_slots, C)
    assert t.dtype == np.complex128 and t.shape == (len(ant), C) and t.flags.c_contiguous
    want = tc.phase_formula(ant, slots, n_slots, C)
    assert np.max(np.abs(t - want)) <= 4 * 2.0 ** -53 * 2 * np.pi      # the phase is at most 2 pi: a few roundings of it
    assert np.all(t[:2] == 1.0)                     # slot 0
    assert np.all(t[:, C // 2] == 1.0)              # the zero-Doppler column
    assert t[6].tobytes() == t[5].tobytes()         # -1 is antenna 11
    assert np.all(np.abs(np.abs(t) - 1.0) <= 2.0 ** -52)
    custom = batch.tdm_phase_table([0, 1], [2, 0], 3, C)
    assert np.all(custom[1] == 1.0) and np.allclose(custom[0], tc.phase_formula([0], [2], 3, C)[0], rtol=0, atol=1e-15)


# ------------------------------------------------------------------ host twin == oracle
def random_case(seed, n_rows, n_ant, C):
    rng = np.random.default_rng(seed)
    cells = rng.standard_normal((n_rows, n_ant)) + 1j * rng.standard_normal((n_rows, n_ant))
    cells *= 10.0 ** rng.uniform(-3, 3, (n_rows, 1))
    return cells, rng.integers(0, C, n_rows)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
@pytest.mark.parametrize("n_ant", range(1, 13))
def test_host_twin_equals_oracle_on_random_cells(n_ant, A, shift):
    slots, n_slots = tc.default_slots(12, 4)
    for C in (9, 16):
        cells, cols = random_case(100 * n_ant + A + shift + C, 200, n_ant, C)
        for ant in (list(range(n_ant)), list(range(11, 11 - n_ant, -1))):
            table = batch.tdm_phase_table(ant, slots, n_slots, C)
            want, decided = tc.oracle_argmax(cells, cols, table, A, shift)
            assert decided.mean() >= 0.99
            got = host_twin(cells, cols, table, A, shift)
            assert np.array_equal(got[decided], want[decided])


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("A", [16, 64])
def test_host_twin_on_crafted_cells(A, shift):
    slots, n_slots = tc.default_slots(12, 4)
    C = 10
    ant = list(range(8))
    table = batch.tdm_phase_table(ant, slots, n_slots, C)
    cols = np.arange(C)
    # one non-zero antenna (the first of the list): every bin is y_0 W^0, a tie bit for bit, and the first index wins
    one = np.zeros((C, 8), dtype=np.complex128)
    one[:, 0] = 3.0 - 2.0j
    want, decided = tc.oracle_argmax(one, cols, table, A, shift)
    assert decided.all() and np.all(want == 0)
    assert np.array_equal(host_twin(one, cols, table, A, shift), want)
    # two equal antennas in different transmit slots
    two = np.zeros((C, 8), dtype=np.complex128)
    two[:, 2] = two[:, 5] = 1.5 + 0.25j
    want, decided = tc.oracle_argmax(two, cols, table, A, shift)
    got = host_twin(two, cols, table, A, shift)
    assert decided.sum() >= C - 1 and np.array_equal(got[decided], want[decided])
    # compensation moves the peak: away from the zero-Doppler column the indices differ from the uncompensated ones
    plain, _ = tc.oracle_argmax(two, cols, None, A, shift)
    assert np.any(plain != want) and plain[C // 2] == want[C // 2]
    # a NaN cell: every bin is NaN, the first index wins
    nan = np.ones((C, 8), dtype=np.complex128)
    nan[:, 3] = np.nan
    want, _ = tc.oracle_argmax(nan, cols, table, A, shift)
    assert np.all(want == 0) and np.array_equal(host_twin(nan, cols, table, A, shift), want)


def test_single_slot_list_is_the_uncompensated_answer():
    slots, n_slots = tc.default_slots(12, 4)
    cells, cols = random_case(5, 300, 4, 16)
    table = batch.tdm_phase_table([8, 9, 10, 11], slots, n_slots, 16)
    assert tc.common_phase(table) and not np.all(table == 1.0)
    for shift in (0, 1):
        plain, decided = tc.oracle_argmax(cells, cols, None, 64, shift)
        assert np.array_equal(tc.oracle_argmax(cells, cols, table, 64, shift)[0], plain)
        assert np.array_equal(host_twin(cells, cols, table, 64, shift)[decided], plain[decided])


# ------------------------------------------------------------------ physics
PHYSICS_SEEDS = range(40, 44)


def test_compensation_recovers_the_true_bin_where_the_plain_argmax_misses():
    """4 rx x 3 tx, S = 16, 16 loops, one noiseless target on exact range and Doppler bins, its Doppler column swept over the
    plane: the compensated oracle returns the true bin in EVERY case, the uncompensated one misses in at least half (the
    issue's full-size draw: 76 %; this shape, seeds 40 .. 43 x 16 columns, measured with the oracle alone: see the assert)."""
    num_rx, num_tx, S, loops, A = 4, 3, 16, 16, 64
    slots, n_slots = tc.default_slots(num_rx * num_tx, num_rx)
    az = list(range(8))
    table = batch.tdm_phase_table(az, slots, n_slots, loops)
    hit = miss = total = 0
    for seed in PHYSICS_SEEDS:
        for kd in range(-loops // 2, loops // 2):
            cube, det, true_bin = tc.physics_scene(seed, kd, num_rx, num_tx, S, loops, A=A, shift=True)
            cells = tc.cells_of(cube, [det])[:, az]
            comp, _ = tc.oracle_argmax(cells, [det[1]], table, A, True)
            plain, _ = tc.oracle_argmax(cells, [det[1]], None, A, True)
            total += 1
            hit += int(comp[0] == true_bin)
            miss += int(plain[0] != true_bin)
    print(f"compensated hits {hit}/{total}, uncompensated misses {miss}/{total}")
    assert hit == total
    assert 2 * miss >= total


# ------------------------------------------------------------------ bound of the float32 phasor product
def adversarial_cells():
    f = np.float32
    ends = []
    for e in (-20, 0, 1, 20):
        lo = f(2.0 ** e)
        ends += [lo, np.nextafter(lo, f(np.inf)), np.nextafter(f(2.0 ** (e + 1)), f(0)), np.nextafter(lo, f(0))]
    ends = np.array(ends + [-v for v in ends], dtype=np.float32)
    re, im = np.meshgrid(ends, ends)
    return (re.ravel() + 1j * im.ravel()).astype(np.complex64)


def test_float32_product_error_stays_inside_the_derived_term():
    slots = [0, 1, 2, 5]
    table = batch.tdm_phase_table([0, 1, 2, 3], slots, 6, 4096)        # phases on a fine grid: near every multiple of pi / 2
    p64 = table.ravel()
    ang = np.angle(p64)
    near = np.argsort(np.abs(((ang + np.pi / 4) % (np.pi / 2)) - np.pi / 4))[:400]
    rng = np.random.default_rng(11)
    worst = 0.0
    for x, p in ((adversarial_cells()[:, None], p64[near][None, :]),
                 ((rng.standard_normal(20000) + 1j * rng.standard_normal(20000)).astype(np.complex64) *
                  np.float32(10.0) ** rng.integers(-6, 7, 20000).astype(np.float32), p64[rng.integers(0, p64.size, 20000)])):
        x, p = np.broadcast_arrays(x, p)
        x, p = np.ascontiguousarray(x), np.ascontiguousarray(p)
        p32 = p.astype(np.complex64)
        exact = x.astype(np.complex128) * p
        for fused in (False, True):
            err = np.abs(tc.product_f32(x, p32, fused) - exact)
            ratio = err / tc.product_term(x)
            assert np.all(ratio <= 1.0), f"error {ratio.max():.3f} x the derived term (fused={fused})"
            worst = max(worst, float(ratio.max()))
    print(f"largest float32 product error: {worst:.3f} of the derived term")
    assert worst >= 1.0 / 16.0          # the term is honest: within 16 x of an error that occurs


# ------------------------------------------------------------------ options
class FakeBuffer:
    def __init__(self, n):
        self.nbytes, self.ptr = n, 0

    def free(self):
        pass


class FakeContext:
    handle = None

    def alloc(self, n):
        return FakeBuffer(n)


def make_cm():
    cm = ConfigManager()
    cm.load_cfg_text(synth.synth_cfg_text(16, 8, 3))
    return cm


def test_tdm_tx_slots_are_validated():
    cm = make_cm()
    for bad in ([0] * 11, [0] * 13, [0] * 11 + [-1], [0.5] * 12, 3):
        with pytest.raises(ValueError):
            batch.FramePipeline(cm, 2, (12, 16, 8), ctx=FakeContext(), tdm_compensation=True, tdm_tx_slots=bad)
        with pytest.raises(ValueError):
            batch.FramePipeline(cm, 2, (12, 16, 8), ctx=FakeContext(), tdm_tx_slots=bad)
    from mmwave_radar_processing_amd.processors import PointCloudGenerator
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, [0, 1], [], tdm_compensation=True, tdm_tx_slots=[0] * 5)
    with pytest.raises(ValueError):
        PointCloudGenerator(cm, [0, 1], [], tdm_compensation=True, tdm_tx_slots=[0] * 11 + [-2])
    assert batch.tdm_tx_slots_of(None, 12, 4) == ([0] * 4 + [1] * 4 + [2] * 4, 3)
    assert batch.tdm_tx_slots_of([2, 0, 1], 3, 4) == ([2, 0, 1], 3)
    with pytest.raises(ValueError):
        batch.tdm_tx_slots_of(None, 10, 4)


def test_option_off_constructs_as_before():
    cm = make_cm()
    p = batch.FramePipeline(cm, 2, (12, 16, 8), ctx=FakeContext())
    assert p.tdm_compensation is False and p.tdm_slots is None
    q = batch.FramePipeline(cm, 2, (12, 16, 8), ctx=FakeContext(), tdm_compensation=True)
    assert q.tdm_compensation is True and q.tdm_slots == ([0] * 4 + [1] * 4 + [2] * 4, 3)
    r = batch.FramePipeline(cm, 2, (12, 16, 8), ctx=FakeContext(), tdm_compensation=True, tdm_tx_slots=[0, 1, 2] * 4)
    assert r.tdm_slots == ([0, 1, 2] * 4, 3)


def test_synth_tdm_targets_carries_the_slot_phase():
    """The scene generator's slot phase comes from the chirp timing: de-interleaved, antenna slot k of a target on Doppler bin kd
    leads slot 0 by 2 pi k kd / (num_tx loops), the conjugate of the table's factor."""
    num_rx, num_tx, S, loops, kd = 4, 3, 16, 16, 5
    raw, bins = synth.synth_tdm_targets(0, num_rx, num_tx, S, loops, [(10.0, 4 / S, kd / (num_tx * loops), 0.0)])
    assert raw.shape == (num_rx, S, num_tx * loops) and raw.dtype == np.complex64 and bins.tolist() == [32]
    cells = tc.cells_of(tc.deinterleave(raw, num_tx), [(4, kd + loops // 2)])[0]
    slots, n_slots = tc.default_slots(12, 4)
    table = batch.tdm_phase_table(range(12), slots, n_slots, loops)[:, kd + loops // 2]
    flat = cells * table
    assert np.max(np.abs(flat - flat[0])) <= 1e-5 * abs(flat[0])
    assert np.max(np.abs(cells - cells[0])) > 0.5 * abs(cells[0])
