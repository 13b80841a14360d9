"""launch_fft_axis (csrc/mmw_fft_generic.h) at every size, layout and type pair some entry point dispatches, through the C ABI.

Cases, inputs, references and the budget: tests/axis_fft_cases.py (tests/test_axis_fft_cases_host.py checks them without a GPU).
Every case asserts

  * the branch it claims -- kernel, tile, quarter tile -- from axis_fft_cases.expected_kernel with the device's CU count (the
    range-Doppler cases from mmw_diag_rd_plan / the budget's form as well);
  * |got - ref| <= ulps * eps * l1 on every output cell, the budget of the project's counting rule;
  * its guards: every output buffer has guard words before and after it and is filled with an all-ones (NaN) pattern before the
    call, so a cell left unwritten or a store outside the output fails.

Each test prints its worst share of the budget with the cell and, where there is one, the input family of its column.
"""
import ctypes

import numpy as np
import pytest

import axis_fft_cases as ac
import rd_bound_cases as rb
from mmwave_radar_processing_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 256         # bytes on either side of an output


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@pytest.fixture(scope="module")
def num_cu():
    return _lib.device_info(0)["num_cu"]


class Guarded:
    """A device buffer of nbytes between two guards, all of it bytes of 0xFF (a NaN in every float and double)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.buf = ctx.alloc(self.nbytes + 2 * GUARD)
        _lib.check(ctx.lib.mmw_memset(ctx.handle, self.buf.ptr, 0xFF, self.buf.nbytes))
        self.ptr = self.buf.at(GUARD)

    def upload(self, arr):
        self.buf.upload(arr, GUARD)

    def result(self, shape, dtype, written=True):
        """The payload, after checking both guards; written: no cell may still hold the fill pattern."""
        self.ctx.sync()
        for off in (0, GUARD + self.nbytes):
            assert (self.buf.download((GUARD,), np.uint8, off) == 0xFF).all(), "a store outside the output buffer"
        out = self.buf.download(shape, dtype, GUARD).copy()
        assert out.nbytes == self.nbytes
        if written:
            assert not np.isnan(out.view(np.float64 if out.dtype.itemsize % 8 == 0 and out.dtype.kind == "f" else np.float32)).any(), \
                "an output cell was left unwritten (or is NaN)"
        return out

    def free(self):
        self.buf.free()


def device_input(ctx, arr):
    d = ctx.alloc(arr.nbytes)
    d.upload(arr)
    return d


def report(what, ratio, cell, extra=""):
    print(f"\n  {what}: worst share of the budget {ratio:.4f} at cell {cell}{extra}")
    assert ratio <= 1, (what, ratio, cell)
    return ratio


# ------------------------------------------------------------------ mmw_angle_fft
def run_angle(ctx, c, rd):
    mag = bool(c.flags & ac.MAGNITUDE)
    bins = c.S * c.C
    d_in, out = device_input(ctx, rd), Guarded(ctx, c.F * c.A * bins * (4 if mag else 8))
    try:
        _lib.check(ctx.lib.mmw_angle_fft(ctx.handle, d_in.ptr, out.ptr, c.F, c.V, c.S, c.C, c.A, c.flags))
        return out.result((c.F, c.A, bins), np.float32 if mag else np.complex64)
    finally:
        d_in.free()
        out.free()


@pytest.mark.parametrize("c", ac.ANGLE_CASES, ids=lambda c: c.name)
def test_angle_fft_generic(ctx, num_cu, c):
    k = ac.expected_kernel(c.A, False, ac.F32, ac.F32, c.S * c.C, c.F, c.V, num_cu)
    assert (k.kind, k.B, k.quarter) == (c.kind, c.B, c.quarter), (c.name, k)
    kinds, rd, ref, l1 = ac.angle_data(c)
    got = run_angle(ctx, c, rd)
    want = np.abs(ref) if c.flags & ac.MAGNITUDE else ref
    ratio, cell = ac.worst(got, want, l1, ac.angle_ulps(c), ac.EPS32)
    report(f"angle {c.name} ({k.kind} B={k.B}, {ac.angle_ulps(c)} ulps)", ratio, cell, f" ({kinds[cell[0] * c.S * c.C + cell[2]]})")
    if c.V == 2 and not c.flags & ac.NO_WINDOW:
        assert not got.any()                # np.hanning(2) = [0, 0] (include/mmwgpu.h)
    if c.flags & ac.MAGNITUDE:
        # against |complex output| of the same input: the hypot term alone
        cplx = run_angle(ctx, c._replace(flags=c.flags & ~ac.MAGNITUDE), rd)
        r2, cell2 = ac.worst(got, np.abs(cplx.astype(np.complex128)), l1, ac.HYPOT_ULPS, ac.EPS32)
        report(f"angle {c.name} |.| against its complex output", r2, cell2)


def test_angle_stage_of_chain3d(ctx, num_cu):
    """mmw_chain3d with the range-Doppler cube kept: the angle output against the float64 angle transform of that cube as the
    device left it (the cube itself is under test in test_gpu_rd_error_bound.py)."""
    V, S, Cc, F = ac.CHAIN_V, ac.CHAIN_S, ac.CHAIN_C, ac.CHAIN_F
    bins = S * Cc
    cubes = np.stack([rb.build_planes(S, Cc, 610 + f)[1][:V] for f in range(F)])
    d_in = device_input(ctx, cubes)
    try:
        for A in ac.CHAIN_A:
            k = ac.expected_kernel(A, False, ac.F32, ac.F32, bins, F, V, num_cu)
            assert k.kind == ("strided" if A in ac.RADIX else "direct")
            d_rd, out = Guarded(ctx, cubes.nbytes), Guarded(ctx, F * A * bins * 8)
            try:
                _lib.check(ctx.lib.mmw_chain3d(ctx.handle, d_in.ptr, d_rd.ptr, out.ptr, F, V, S, Cc, A, 0))
                got, rd = out.result((F, A, bins), np.complex64), d_rd.result((F, V, bins), np.complex64)
            finally:
                d_rd.free()
                out.free()
            ref, l1 = ac.angle_reference(rd, A, 0)
            ulps = ac.WINDOW_ULPS + ac.axis_ulps(A, V)
            report(f"chain3d A={A} ({k.kind} B={k.B}, {ulps} ulps)", *ac.worst(got, ref, l1, ulps, ac.EPS32))
    finally:
        d_in.free()


# ------------------------------------------------------------------ mmw_range_angle
@pytest.mark.parametrize("c", ac.RANGE_ANGLE_CASES, ids=lambda c: c.name)
def test_range_angle(ctx, num_cu, c):
    n_sel = len(c.rx) if c.rx else c.V
    k1 = ac.expected_kernel(c.S, False, ac.F32, ac.F32, 1, ac.RA_F, c.S, num_cu)
    k2 = ac.expected_kernel(c.A, False, ac.F32, ac.F32, c.S, ac.RA_F, n_sel, num_cu)
    assert k1.kind == ("strided" if c.S in ac.RADIX else "direct") and not k1.quarter and k2.kind == ("strided" if c.A in ac.RADIX else "direct")
    cubes, ref, l1 = ac.range_angle_data(c)
    rx, n_rx = _lib.int_array(c.rx or [])
    d_in, out = device_input(ctx, cubes), Guarded(ctx, ac.RA_F * c.S * c.A * 4)
    try:
        _lib.check(ctx.lib.mmw_range_angle(ctx.handle, d_in.ptr, out.ptr, ac.RA_F, c.V, c.S, ac.RA_C, c.A, c.chirp, rx, n_rx, c.window))
        got = out.result((ac.RA_F, c.S, c.A), np.float32)
    finally:
        d_in.free()
        out.free()
    report(f"range_angle {c.name} ({k1.kind} B={k1.B}, {k2.kind} B={k2.B} quarter={k2.quarter}, {ac.range_angle_ulps(c)} ulps)",
           *ac.worst(got, ref, l1, ac.range_angle_ulps(c), ac.EPS32))


# ------------------------------------------------------------------ mmw_range_profile / _f64
def run_profile(ctx, t, cubes, S, expect_ok=True):
    wide = t == ac.F64
    fn = ctx.lib.mmw_range_profile_f64 if wide else ctx.lib.mmw_range_profile
    d_in, out = device_input(ctx, cubes), Guarded(ctx, ac.RP_F * S * t)
    try:
        status = fn(ctx.handle, d_in.ptr, out.ptr, ac.RP_F, ac.RP_V, S, ac.RP_C, ac.RP_CHIRP)
        if expect_ok:
            _lib.check(status)
        return status, out.result((ac.RP_F, S), np.float64 if wide else np.float32, written=expect_ok)
    finally:
        d_in.free()
        out.free()


@pytest.mark.parametrize("t,S", ac.RP_CASES, ids=lambda v: str(v))
def test_range_profile(ctx, num_cu, t, S):
    k = ac.expected_kernel(S, False, t, ac.F32, 1, ac.RP_F * ac.RP_V, S, num_cu)
    want_b = {385: 8, 769: 4, 1537: 2, 3073: 1, 4096: 1} if t == ac.F32 else {193: 8, 385: 4, 769: 2, 1537: 1, 3073: 1, 4096: 1}
    assert (k.kind, k.B) == (("strided", ac.strided_tile(S, 2 * t)) if S in ac.RADIX else ("direct", want_b[S])) and not k.quarter
    cubes, ref, l1 = ac.range_profile_data(S, t == ac.F64)
    _, got = run_profile(ctx, t, cubes, S)
    report(f"range_profile{'_f64' if t == ac.F64 else ''} S={S} ({k.kind} B={k.B}, {ac.range_profile_ulps(S)} ulps)",
           *ac.worst(got, ref, l1, ac.range_profile_ulps(S), ac.EPS64 if t == ac.F64 else ac.EPS32))


@pytest.mark.parametrize("t", [ac.F32, ac.F64], ids=["f32", "f64"])
def test_range_profile_refuses_4097_samples(ctx, t):
    S = ac.RP_REFUSED
    assert ac.expected_kernel(S, False, t, ac.F32, 1, ac.RP_F * ac.RP_V, S, 256) is None
    status, out = run_profile(ctx, t, np.ones((ac.RP_F, ac.RP_V, S, ac.RP_C), np.complex64), S, expect_ok=False)
    assert status == _lib.MMW_ERR_INVALID and b"not supported" in ctx.lib.mmw_last_error()
    assert (out.view(np.uint8) == 0xFF).all(), "a refused call wrote to its output"


# ------------------------------------------------------------------ mmw_range_doppler_mag64
@pytest.mark.parametrize("S,C", ac.MAG64_SHAPES, ids=lambda v: str(v))
def test_range_doppler_mag64_two_pass(ctx, num_cu, S, C, monkeypatch):
    for name in rb.ENV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if (S, C) in ac.MAG64_NEEDS_SWITCH:
        monkeypatch.setenv("MMW_NO_MIXED_RD", "1")
    plan = (ctypes.c_int * 8)()
    _lib.check(ctx.lib.mmw_diag_rd_plan(S, C, 1, plan))
    assert plan[0] == 3, (S, C, plan[0])
    F, V = ac.MAG64_F, ac.MAG64_V
    k1, k2 = ac.mag64_kernels(S, C, F, num_cu)
    assert k1.kind == ("strided" if S in ac.RADIX else "direct") and k2.kind == ("contig" if C in ac.RADIX else "direct")
    assert max(k1.lds, k2.lds) <= 65536
    if (S, C) == (8, 512):
        assert (k2.B, k2.threads, F * S % k2.B) == (5, 80, 1)          # 16 rows: three tiles of five and a one-row tail
    if C == 1024:
        assert k2.B == 2
    if S == 1024:
        assert k1.B == 4 and k1.lds == 65536
    cubes, ref, l1 = ac.mag64_data(S, C)
    d_in, out = device_input(ctx, cubes), Guarded(ctx, F * S * C * 8)
    try:
        _lib.check(ctx.lib.mmw_range_doppler_mag64(ctx.handle, d_in.ptr, out.ptr, F, V, S, C, ac.MAG64_RX))
        got = out.result((F, S, C), np.float64)
    finally:
        d_in.free()
        out.free()
    report(f"mag64 {S}x{C} ({k1.kind} B={k1.B}, {k2.kind} B={k2.B}, {ac.mag64_ulps(S, C)} ulps)",
           *ac.worst(got, ref, l1, ac.mag64_ulps(S, C), ac.EPS64))


# ------------------------------------------------------------------ mmw_range_doppler, float32, the generic pair
@pytest.mark.parametrize("V,S,C", ac.RD32_SHAPES, ids=lambda v: str(v))
def test_range_doppler_generic_pair(ctx, num_cu, V, S, C, monkeypatch):
    for name, value in ac.RD32_ENV.items():
        monkeypatch.setenv(name, value)
    plan = (ctypes.c_int * 8)()
    _lib.check(ctx.lib.mmw_diag_detect_plan(S, C, _lib.CFAR_CA, 4, 4, 2, 2, 0, 0, 64, plan))
    ulps = rb.generic_ulps(S, C)
    assert plan[7] == ulps                  # rd_error_ulps tests the same switches as range_doppler_impl: the two-kernel path
    k1, k2 = ac.rd32_kernels(V, S, C, num_cu)
    assert k1.kind == ("strided" if S in ac.RADIX else "direct") and k2.kind == ("contig" if C in ac.RADIX else "direct")
    if V == 3 and k2.kind == "contig":
        assert (V * S) % k2.B, "rows must not fill the contiguous tile"
    names, cube, rd64, l1 = rb.planes_and_reference(S, C)
    worst = 0.0
    for sel in (ac.RD32_SUBSETS if V == 3 else (tuple(range(10)),)):
        sel = list(sel)
        d_in, out = device_input(ctx, cube[sel]), Guarded(ctx, V * S * C * 8)
        try:
            _lib.check(ctx.lib.mmw_range_doppler(ctx.handle, d_in.ptr, out.ptr, None, 1, V, S, C))
            got = out.result((V, S, C), np.complex64)
        finally:
            d_in.free()
            out.free()
        ratios, cells = rb.check(got, rd64[sel], l1[sel], ulps)
        w = int(np.argmax(ratios))
        worst = max(worst, report(f"rd32 {S}x{C} planes {sel} ({k1.kind} B={k1.B} quarter={k1.quarter}, {k2.kind} B={k2.B}, {ulps} ulps)",
                                  float(ratios[w]), cells[w], f" ({names[sel[w]]})"))
