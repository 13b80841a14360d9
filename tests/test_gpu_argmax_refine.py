"""The float64 refinement of mmw_angle_argmax_exact on built detection lists, through the C ABI, route by route.

Inputs and references: tests/refine_cases.py (every evaluation is flagged by construction; tests/test_refine_cases_host.py
checks the builders without a GPU).  Per case the cube is uploaded once, d_rd and d_l1 come from mmw_range_doppler and
mmw_plane_l1 (the sequence of FramePipeline.point_clouds for the stand-alone path), and mmw_angle_argmax_exact runs once per
route setting (context options, removed again afterwards):

    dense    MMW_ARGMAX_DENSE_MIN = 1          k_cells64<128> + k_argmax64_list up to dense_cap, the direct kernels beyond
    direct   MMW_ARGMAX_DENSE_MIN = 2^30       k_argmax_refine_part + _finish
    whole    ... and MMW_REFINE_SPLIT = 0      k_argmax_refine_whole
    mixed    ... and MMW_REFINE_SPLIT = 3      three entries part + finish, the rest whole

Asserted in this order: MMW_OK; n_refined == evaluations (else the message names P_TONE); indices == the oracle's on every
non-excluded evaluation; unlisted slots of d_idx still hold the sentinel; all routes of a case identical everywhere.

Value level (mmw_rd_cells64_at): the complex128 cells of both routes against np.longdouble direct sums of the windowed
float32 cube, error normalised by the cell's L1w = sum |w_s w_c x|, asserted against the a-priori bounds
refine_cases.gamma_dense / gamma_direct (derivations in their docstrings; u = 2^-53):

    dense   |err| <= (77 + 8 ceil(S / 64)) u L1w
    direct  |err| <= (20 + per / 256 + parts) u L1w,   per = the slice length, parts = refine_parts(n_frames)

P_TONE = 1e5 (refine_cases.py): measured on an MI355X, 1e3 is the smallest power of ten at which every plane and antenna
list reports n_refined == evaluations (10 and 100 do not); the cases use 100 x that.

The measured maxima (kernel, and np.fft.fft2 in complex128 on the same cells as the yardstick) are printed; DESIGN.md 4.6
records them.
"""
import numpy as np
import pytest

import refine_cases as rc
from mmwave_radar_processing_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROUTES = {
    "dense": {"MMW_ARGMAX_DENSE_MIN": 1},
    "direct": {"MMW_ARGMAX_DENSE_MIN": 1 << 30},
    "whole": {"MMW_ARGMAX_DENSE_MIN": 1 << 30, "MMW_REFINE_SPLIT": 0},
    "mixed": {"MMW_ARGMAX_DENSE_MIN": 1 << 30, "MMW_REFINE_SPLIT": 3},
}


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


class Resident:
    """A case's cube, detection list, range-Doppler cube and plane norms on the device."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        c = case
        n = c.F * c.V * c.S * c.C * 8
        slots = c.F * max(c.cap, 1)
        self.bufs = dict(cube=ctx.alloc(n), rd=ctx.alloc(n), l1=ctx.alloc(c.F * c.V * 4), dets=ctx.alloc(slots * 8),
                         counts=ctx.alloc(c.F * 4), idx=ctx.alloc(slots * 4))
        b = self.bufs
        b["cube"].upload(c.cube)
        b["dets"].upload(c.dets)
        b["counts"].upload(c.counts)
        _lib.check(ctx.lib.mmw_range_doppler(ctx.handle, b["cube"].ptr, b["rd"].ptr, None, c.F, c.V, c.S, c.C))
        _lib.check(ctx.lib.mmw_plane_l1(ctx.handle, b["cube"].ptr, b["l1"].ptr, c.F, c.V, c.S, c.C))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self.bufs.values():
            buf.free()

    def argmax(self, ants, shift, options):
        """(return code, n_refined, idx [F][cap]) of one mmw_angle_argmax_exact call under the given context options."""
        c, b, ctx = self.case, self.bufs, self.ctx
        b["idx"].upload(np.full((c.F, max(c.cap, 1)), SENTINEL, dtype=np.int32))
        arr, n_ant = _lib.int_array(ants)
        n_ref = _lib.C.c_int(-1)
        try:
            for name, value in options.items():
                ctx.set_option(name, value)
            rc_ = ctx.lib.mmw_angle_argmax_exact(ctx.handle, b["cube"].ptr, b["l1"].ptr, b["rd"].ptr, b["dets"].ptr, b["counts"].ptr,
                                                 b["idx"].ptr, c.F, c.V, c.S, c.C, c.cap, arr, n_ant, rc.A_BINS, int(shift),
                                                 _lib.C.byref(n_ref))
        finally:
            for name in options:
                ctx.set_option(name, None)
        return rc_, n_ref.value, b["idx"].download((c.F, max(c.cap, 1)), np.int32)

    def cells(self, ants, route):
        """(return code, cells [F][cap][n_ant] complex128, NaN where nothing was written) of mmw_rd_cells64_at."""
        c, ctx = self.case, self.ctx
        arr, n_ant = _lib.int_array(ants)
        fill = np.full((c.F, max(c.cap, 1), n_ant), np.nan + 1j * np.nan, dtype=np.complex128)
        d_out = ctx.alloc(fill.nbytes)
        try:
            d_out.upload(fill)
            rc_ = ctx.lib.mmw_rd_cells64_at(ctx.handle, self.bufs["cube"].ptr, self.bufs["dets"].ptr, self.bufs["counts"].ptr, d_out.ptr,
                                            c.F, c.V, c.S, c.C, c.cap, arr, n_ant, route)
            return rc_, d_out.download(fill.shape, np.complex128)
        finally:
            d_out.free()


def check_indices(res, ants, shift, routes):
    """Assertions 1-5 of the module docstring for one antenna list; returns {route: idx}."""
    c = res.case
    want, excl, _ = c.expected(tuple(ants), int(shift))
    listed = want >= 0
    got = {}
    for route in routes:
        tag = f"{c.name} {route} ants {list(ants)} shift {shift}"
        rc_, n_ref, idx = res.argmax(ants, shift, ROUTES[route] if route != "default" else {})
        assert rc_ == _lib.MMW_OK, tag
        assert n_ref == c.n_evals, f"{tag}: {n_ref} of {c.n_evals} evaluations flagged with P_TONE = {c.P:g}"
        cmp = listed & ~excl
        bad = np.argwhere(cmp & (idx != want))
        assert len(bad) == 0, f"{tag}: {len(bad)} indices differ from the oracle's, first (f, det) {bad[0]}: {idx[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        assert np.all(idx[~listed] == SENTINEL), f"{tag}: a slot beyond min(counts, cap) was written"
        got[route] = idx
    first = routes[0]
    for route in routes[1:]:
        diff = listed & (got[route] != got[first])
        if np.any(diff & excl):
            print(f"{c.name}: {route} and {first} differ on {np.count_nonzero(diff & excl)} excluded evaluations")
        assert not np.any(diff & ~excl), f"{c.name}: {route} and {first} disagree"
    return got


ALL_ROUTES = ("dense", "direct", "whole", "mixed")


@pytest.mark.parametrize("S", rc.DENSE_S + (830,))
def test_planes_of_128_chirps(ctx, S):
    """8 and 63 (one pass, lanes past the plane), 64, 100 (ragged second pass, not a power of two), 256, 512 (8 passes), 829
    (the last plane the LDS takes) through k_cells64; 830 has no dense kernel and takes the direct route under every setting."""
    case = rc.case(f"plane_{S}x128")
    with Resident(ctx, case) as res:
        check_indices(res, (0, 1, 2, 3), 1, ALL_ROUTES)
        check_indices(res, (3, 0, 2), 0, ("dense", "direct"))


@pytest.mark.parametrize("plane", ["256x128", "100x128"])
@pytest.mark.parametrize("layout", ["corners", "duplicates", "n256", "n257", "n513", "n700", "tail", "overcap", "alternating"])
def test_detection_layouts(ctx, layout, plane):
    """Corners of the plane and the Doppler wrap, a cell listed five times, 256 / 257 / 513 / 700 flagged cells in one frame
    (one full chunk, a second chunk, three chunks and a second pass of the detection scan), a list longer than dense_cap whose
    tail the direct kernels take in the same call, counts beyond cap, empty frames between full ones."""
    case = rc.case(f"{layout}_{plane}")
    with Resident(ctx, case) as res:
        check_indices(res, (0, 1, 2, 3), 1, ("dense", "direct", "mixed") if case.n_evals <= 300 else ("dense", "direct"))


def test_dense_min_threshold(ctx):
    """F = 4 and the default dense_min = 8 F = 32: calls with 31 and with 32 flagged evaluations under the default options
    (by the code the direct and the dense route; which one ran cannot be seen from outside, both must be right) give the
    oracle's indices, the forced routes' indices, and each other's on the 31 shared detections."""
    c31, c32 = rc.case("thr31_64x128"), rc.case("thr32_64x128")
    np.testing.assert_array_equal(c31.cube, c32.cube)
    shared = c31.expected((0, 1, 2, 3), 1)[0] >= 0
    assert np.count_nonzero(shared) == 31 and c32.n_evals == 32
    np.testing.assert_array_equal(c31.dets[shared], c32.dets[shared])
    with Resident(ctx, c31) as r31, Resident(ctx, c32) as r32:
        i31 = check_indices(r31, (0, 1, 2, 3), 1, ("default", "dense", "direct"))["default"]
        i32 = check_indices(r32, (0, 1, 2, 3), 1, ("default", "dense", "direct"))["default"]
    np.testing.assert_array_equal(i31[shared], i32[shared])


@pytest.mark.parametrize("name", list(rc.ANT_LISTS))
def test_antenna_lists(ctx, name):
    """Lengths that are no multiple of REFINE_NA = 4, 9 to 32 antennas (V = 32), a repeated antenna, descending order; with
    and without the fftshift of the angle axis."""
    case = rc.case("ants_64x128")
    with Resident(ctx, case) as res:
        for shift in (1, 0):
            check_indices(res, rc.ANT_LISTS[name], shift, ("dense", "direct", "whole"))


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in rc.DIRECT_PLANES])
def test_direct_only_planes(ctx, plane):
    """No dense kernel (C != 128): C > 256 (ds = 0 with a carry), C = 256 (dc = 0), planes smaller than one slice of 256
    cells (empty slices), all-zero windows (S = 2, C = 2); split + finish, whole-plane, and both in one call."""
    case = rc.case(f"direct_{plane}")
    with Resident(ctx, case) as res:
        check_indices(res, (0, 1, 2, 3), 1, ("direct", "whole", "mixed", "dense"))
        check_indices(res, (2, 0, 1), 0, ("direct", "whole"))


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in rc.PARTS_PLANES])
@pytest.mark.parametrize("F", rc.PARTS_STEPS)
def test_frame_counts_around_the_slice_steps(ctx, F, plane):
    """refine_parts(n_frames) halves the slices per plane at 3750 / 7500 / 15000 frames: both sides of every step, on the
    direct-only planes whose cubes stay small at 15001 frames (8 x 10, 127 x 2, 2 x 5: one slice holds the plane) and on
    20 x 56, whose slice length and number of slices that hold cells change with the slice count (256 x 5, 512 x 3, 768 x 2):
    there the cells themselves are compared as well.  63 x 100, 254 x 50, 16 x 320 and 32 x 256 are left out of this sweep:
    their cubes would take 1.5 to 6 GB at 15001 frames."""
    case = rc.case(f"parts_{F}_{plane}")
    with Resident(ctx, case) as res:
        check_indices(res, (0, 1, 2, 3), 1, ("direct", "whole", "mixed"))
        if plane == "20x56":
            check_values(res, _lib.CELLS64_DIRECT, rc.gamma_direct(case.S, case.C, case.F), [(0, 0), (0, 1), (1, 0), (F - 1, 0), (F - 1, 1)])


# ---- value level ------------------------------------------------------------------------------------------------------------
def check_values(res, route, gamma, picks):
    """picks: (f, det) slots to compare (<= 64)."""
    c = res.case
    ants = (0, 1, 2, 3)
    rc_, cells = res.cells(ants, route)
    assert rc_ == _lib.MMW_OK, c.name
    listed = np.zeros(cells.shape[:2], dtype=bool)
    for f in range(c.F):
        listed[f, :c.listed(f)] = True
    assert not np.any(np.isnan(cells[listed])), f"{c.name}: a listed cell was not written"
    assert np.all(np.isnan(cells[~listed])), f"{c.name}: a slot beyond min(counts, cap) was written"
    worst_k = worst_np = 0.0
    for f in sorted({f for f, _ in picks}):
        dets = [d for ff, d in picks if ff == f]
        want, l1 = rc.longdouble_cells(c.cube[f], c.dets[f, dets], ants)
        got = cells[f, dets].astype(np.clongdouble)
        ref_np = c.rd(f)[list(ants)][:, c.dets[f, dets, 0], c.dets[f, dets, 1]].T.astype(np.clongdouble)
        worst_k = max(worst_k, float(np.max(np.abs(got - want) / (rc.U * l1[None, :]))))
        worst_np = max(worst_np, float(np.max(np.abs(ref_np - want) / (rc.U * l1[None, :]))))
    print(f"{c.name} route {route}: max |err| / (2^-53 L1w) kernel {worst_k:.3f} (bound {gamma}), numpy fft2 {worst_np:.3f}")
    assert worst_k <= gamma, f"{c.name}: cell error {worst_k:.3f} u L1w exceeds the derived bound {gamma}"


def spread(case, f, n):
    """n listed slots of frame f: the first ones (corners), both sides of the 256-cell chunk border, the last ones."""
    m = case.listed(f)
    want = list(range(min(m, n // 2))) + [d for d in (254, 255, 256, 257) if d < m] + list(range(max(0, m - n // 4), m))
    return [(f, d) for d in sorted(set(want))][:n]


@pytest.mark.parametrize("plane", ["8x128", "63x128", "100x128", "256x128", "512x128"])
def test_dense_cell_values(ctx, plane):
    case = rc.case(f"value_{plane}")
    with Resident(ctx, case) as res:
        check_values(res, _lib.CELLS64_DENSE, rc.gamma_dense(case.S), spread(case, 0, 48) + spread(case, 1, 12))
        if plane == "100x128":        # the same cells through the direct slices
            check_values(res, _lib.CELLS64_DIRECT, rc.gamma_direct(case.S, case.C, case.F), spread(case, 0, 24))


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in rc.DIRECT_PLANES])
def test_direct_cell_values(ctx, plane):
    case = rc.case(f"direct_{plane}")
    with Resident(ctx, case) as res:
        rc_, _ = res.cells((0, 1), _lib.CELLS64_DENSE)
        assert rc_ == _lib.MMW_ERR_UNSUPPORTED
        if min(case.S, case.C) == 2:      # np.hanning(2) = [0, 0]: L1w = 0 and every cell is exactly zero
            rc_, cells = res.cells((0, 1, 2, 3), _lib.CELLS64_DIRECT)
            assert rc_ == _lib.MMW_OK
            for f in range(case.F):
                assert np.all(cells[f, :case.listed(f)] == 0)
            return
        check_values(res, _lib.CELLS64_DIRECT, rc.gamma_direct(case.S, case.C, case.F), spread(case, 0, 24) + spread(case, 2, 5))
