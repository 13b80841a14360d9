"""The rounding-error bound of the float32 range-Doppler kernels, on adversarial planes, through the C ABI.

    |rd32[cell] - rd64[cell]|  <=  plan[7] * 2^-24 * l1_dev(plane)          (plan[7] = rd_error_ulps, mmw_diag_detect_plan)

is what the screening band of mmw_detect_points (mmw_detect.h) and the certainty test of mmw_angle_argmax_exact are built from.
Inputs, references and the list of kernel families: tests/rd_bound_cases.py (one input family per antenna plane, F = 1;
tests/test_rd_bound_cases_host.py checks builders, checker and budgets without a GPU).  Every case asserts, on every plane,

  * l1: mmw_plane_l1 (and the norms the fused producers leave) against the float64 sum, to the relative error of its own
    summation order (l1_tol_plane / l1_tol_producer below);
  * the bound, with the DEVICE's l1 on the right-hand side -- the inequality exactly as the kernels use it.  The reference is
    numpy's complex128 transform of the float64-windowed cube: its own error is below 1e-14 l1, eight orders of magnitude under
    the smallest budget (48 * 2^-24 = 2.9e-6), so it is not part of the comparison;
  * the kernel family, where mmw_diag_rd_plan reflects the switches in force, and the budget's form everywhere.

Each test prints its worst ratio with the input family and the cell; tools/rd_error_bound.py collects the same figures into
profiles/rd_error_bound.json.
"""
import ctypes
import math

import numpy as np
import pytest

import rd_bound_cases as rb
from mmwave_radar_processing_amd import _lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def gamma(n):
    """Relative error bound of n chained float32 roundings."""
    return n * U / (1 - n * U)


def l1_tol_plane(S, C):
    """k_plane_l1 (mmw_staging.h) adds non-negative terms, so every rounding is a relative error of the final sum and the depth of
    the longest chain bounds it: per term two table values (hann(S), hann(C): 1 each), |re| + |im| (1), the product with hann(C)
    (1) and the row's product with hann(S) (1) = 5; a lane's row chain -- ceil(C / 128) steps of two additions for even C,
    ceil(C / 64) additions for odd C; its chain over rows s = wave, wave + 4, ...: ceil(S / 4) additions; six shuffle steps of
    the wave reduction; two levels over the four waves."""
    row = 2 * math.ceil(C / 128) if C % 2 == 0 else math.ceil(C / 64)
    return gamma(5 + row + math.ceil(S / 4) + 6 + 2)


def l1_tol_producer(S, C):
    """The fused range-Doppler producers (k_rd_fused_256x128, k_rd_mixed_ct) add |re| + |im| of the windowed sample as they form
    it: w = hann(S) hann(C) (two table values + 1), the sample's product with w (1), |re| + |im| and the pair's sum (2) = 6; a
    lane's chain of at most ceil(S C / 2 / 256) steps (two cells per step, workgroups of 256 threads or more); six shuffle steps;
    a sequential sum over at most 16 waves."""
    return gamma(6 + math.ceil(S * C / 512) + 6 + 16)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


class Switches:
    """The MMW_NO_*_RD environment switches and the context options of a case, for the duration of a with block."""

    def __init__(self, ctx, case, monkeypatch):
        self.ctx, self.case, self.mp = ctx, case, monkeypatch

    def __enter__(self):
        for name in rb.ENV_SWITCHES:
            self.mp.delenv(name, raising=False)
        for name, value in self.case.env.items():
            self.mp.setenv(name, value)
        for name, value in self.case.options.items():
            self.ctx.set_option(name, value)
        return self

    def __exit__(self, *exc):
        for name in self.case.options:
            self.ctx.set_option(name, None)
        for name in self.case.env:
            self.mp.delenv(name, raising=False)


def budget(S, C):
    plan = (ctypes.c_int * 8)()
    _lib.check(_lib.load_library().mmw_diag_detect_plan(S, C, _lib.CFAR_CA, 4, 4, 2, 2, 0, 0, 64, plan))
    return plan[7]


def assert_family(case):
    """Which kernel the case exercises: the plan entry where it reflects the switches, the budget's form everywhere."""
    ulps = budget(case.S, case.C)
    if case.plan0 is not None:
        plan = (ctypes.c_int * 8)()
        _lib.check(_lib.load_library().mmw_diag_rd_plan(case.S, case.C, 0, plan))
        assert plan[0] == case.plan0, (rb.case_id(case), plan[0])
    if case.budget == "structured":
        assert ulps == rb.structured_ulps(case.S, case.C)
    elif case.budget == "generic":             # the switches took rd_error_ulps (and range_doppler_impl, which tests the same ones) to the two-kernel path
        assert ulps == rb.generic_ulps(case.S, case.C)
    else:                                       # the run-time plan's terms on top: no compile-time instantiation served the plane
        assert ulps > rb.structured_ulps(case.S, case.C)
    return ulps


def run_rd_and_l1(ctx, cube):
    """(rd32 [V, S, C], l1_dev [V]) of mmw_range_doppler + mmw_plane_l1 on one frame."""
    V, S, C = cube.shape
    d_in, d_rd, d_l1 = ctx.alloc(cube.nbytes), ctx.alloc(cube.nbytes), ctx.alloc(V * 4)
    try:
        d_in.upload(cube)
        d_rd.zero()
        d_l1.zero()
        _lib.check(ctx.lib.mmw_range_doppler(ctx.handle, d_in.ptr, d_rd.ptr, None, 1, V, S, C))
        _lib.check(ctx.lib.mmw_plane_l1(ctx.handle, d_in.ptr, d_l1.ptr, 1, V, S, C))
        return d_rd.download((V, S, C), np.complex64).copy(), d_l1.download((V,), np.float32).copy()
    finally:
        for b in (d_in, d_rd, d_l1):
            b.free()


def assert_bound(what, names, rd32, l1_dev, rd64, l1_64, ulps, l1_tol):
    """The two assertions on every plane; prints and returns the worst ratio."""
    assert np.isfinite(rd32.view(np.float32)).all() and np.isfinite(l1_dev).all(), what
    l1_err = np.abs(l1_dev.astype(np.float64) - l1_64) / l1_64
    ratios, cells = rb.check(rd32, rd64, l1_dev.astype(np.float64), ulps)
    w = int(np.argmax(ratios))
    print(f"\n  {what}: budget {ulps} ulps; worst ratio {ratios[w]:.4f} on {names[w]} at cell {cells[w]}; "
          f"l1 rel err {l1_err.max():.2e} on {names[int(np.argmax(l1_err))]} (tolerance {l1_tol:.2e})")
    print("    " + ", ".join(f"{n} {r:.4f}" for n, r in zip(names, ratios)))
    assert (l1_err <= l1_tol).all(), (what, dict(zip(names, l1_err)), l1_tol)
    assert (ratios <= 1).all(), (what, dict(zip(names, ratios)), cells)
    return float(ratios[w])


@pytest.mark.parametrize("case", rb.CASES, ids=rb.case_id)
def test_rd_error_stays_inside_the_budget(ctx, case, monkeypatch):
    names, cube, rd64, l1_64 = rb.planes_and_reference(case.S, case.C)
    with Switches(ctx, case, monkeypatch):
        ulps = assert_family(case)
        rd32, l1_dev = run_rd_and_l1(ctx, cube)
    assert_bound(rb.case_id(case), names, rd32, l1_dev, rd64, l1_64, ulps, l1_tol_plane(case.S, case.C))


@pytest.mark.parametrize("case", rb.SCALE_CASES, ids=rb.case_id)
def test_bound_and_bits_under_power_of_two_scaling(ctx, case, monkeypatch):
    """The same cube times 2^-20 and 2^20: the bound holds at each scale, and rd32(2^k x) == 2^k rd32(x) bit for bit -- no
    intermediate overflows or goes subnormal at these scales (smallest windowed sample: 2^-12 * 2^-20 * 9e-8 ~ 2e-17; largest
    sum: 2^20 * 5.4e8), and a power-of-two factor commutes with every rounding the budget books (the three-way bfloat16 split
    included: bfloat16 has float32's exponent range).  The norms scale the same way."""
    names, cube, rd64, l1_64 = rb.planes_and_reference(case.S, case.C)
    tol = l1_tol_plane(case.S, case.C)
    with Switches(ctx, case, monkeypatch):
        ulps = assert_family(case)
        base_rd, base_l1 = run_rd_and_l1(ctx, cube)
        for k in (-20, 20):
            f = np.float32(2.0 ** k)
            rd32, l1_dev = run_rd_and_l1(ctx, (cube * f).astype(np.complex64))
            assert_bound(f"{rb.case_id(case)} x 2^{k}", names, rd32, l1_dev, rd64 * 2.0 ** k, l1_64 * 2.0 ** k, ulps, tol)
            np.testing.assert_array_equal(rd32.view(np.uint32), (base_rd * f).view(np.uint32))
            np.testing.assert_array_equal(l1_dev.view(np.uint32), (base_l1 * f).view(np.uint32))


@pytest.mark.parametrize("S,C", [(256, 128), (63, 100)], ids=["256x128", "63x100"])
def test_fused_producers_leave_a_cube_and_norms_inside_the_budget(ctx, S, C, monkeypatch):
    """d_rd / d_l1 as mmw_detect_batch and mmw_detect_points write them (CA-CFAR, window (4, 4) / (2, 2)) on the adversarial
    frame.  The detections are not under test here: a count of -1 (a frame handed back to the float64 path) is acceptable."""
    for name in rb.ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    names, cube, rd64, l1_64 = rb.planes_and_reference(S, C)
    V, n, cap = cube.shape[0], S * C, 256
    ulps = budget(S, C)
    assert ulps == rb.structured_ulps(S, C)
    assert ctx.lib.mmw_detect_points_supported(S, C, _lib.CFAR_CA, 4, 4, 2, 2, 0, 0, 64) == 1
    tol = max(l1_tol_plane(S, C), l1_tol_producer(S, C))        # whichever of the two the call used for its norms
    bufs = [ctx.alloc(b) for b in (cube.nbytes, cube.nbytes, V * 4, n * 8, n, cap * 8, 4)]
    d_in, d_rd, d_l1, d_mag, d_mask, d_dets, d_cnt = bufs
    try:
        d_in.upload(cube)
        for entry in ("mmw_detect_batch", "mmw_detect_points"):
            d_rd.zero()
            d_l1.zero()
            if entry == "mmw_detect_batch":
                _lib.check(ctx.lib.mmw_detect_batch(ctx.handle, d_in.ptr, d_rd.ptr, d_mag.ptr, d_mask.ptr, d_dets.ptr, d_cnt.ptr,
                                                    d_l1.ptr, 1, V, S, C, _lib.CFAR_CA, 4, 4, 2, 2, 8.0, 0, cap), ok_truncated=True)
            else:
                _lib.check(ctx.lib.mmw_detect_points(ctx.handle, d_in.ptr, d_rd.ptr, d_l1.ptr, None, d_dets.ptr, d_cnt.ptr, None, None,
                                                     1, V, S, C, _lib.CFAR_CA, 4, 4, 2, 2, 8.0, 0, cap, None, 0, 1, None, 0, 0, 64,
                                                     None), ok_truncated=True)
            ctx.sync()
            rd32, l1_dev = d_rd.download((V, S, C), np.complex64).copy(), d_l1.download((V,), np.float32).copy()
            count = int(d_cnt.download((1,), np.int32)[0])
            assert count >= -1
            assert_bound(f"{entry} {S}x{C} (count {count})", names, rd32, l1_dev, rd64, l1_64, ulps, tol)
    finally:
        for b in bufs:
            b.free()
