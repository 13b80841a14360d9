"""k_cells64_mixed<C>, the dense float64 cell kernel of the chirp counts other than 128, through the C ABI.

Inputs and references: tests/cells64_mixed_cases.py on top of tests/refine_cases.py (every evaluation flagged by construction;
tests/test_cells64_mixed_host.py checks builders, plan and bound without a GPU).

Value level: mmw_rd_cells64_at(route = MMW_CELLS64_DENSE_MIXED) against np.longdouble direct sums of the windowed float32 cube,
error normalised by the cell's L1w = sum |w_s w_c x| and asserted against the a-priori bound gamma_mixed(S, C) (derivation in
its docstring; u = 2^-53).  The measured maxima are printed beside np.fft.fft2's; DESIGN.md 4.6 records them.

Index level: mmw_angle_argmax_exact with MMW_ARGMAX_DENSE_MIXED = 1, MMW_ARGMAX_DENSE_MIN = 1 (k_cells64_mixed + k_argmax64_list
up to dense_cap, the direct kernels beyond) against MMW_ARGMAX_DENSE_MIXED = 0 (the direct kernels): MMW_OK; n_refined ==
evaluations; indices == the oracle's on every non-excluded evaluation; the sentinel survives in unlisted slots; both agree.

Fixtures: FramePipeline.point_clouds() and PointCloudGenerator.process on the frames of tests/golden/os_pc_np2.npz (the
reference's OS-CFAR 2-D and sequential-detector point clouds on 12 x 63 x 100 and 12 x 63 x 70, margins >= 1e-9 stored with
them) under the worst-case bound, once with MMW_ARGMAX_DENSE_MIXED = 1 and MMW_ARGMAX_DENSE_MIN = 1 (every flagged evaluation
through k_cells64_mixed; the count of refined evaluations is asserted to be above zero) and once with MMW_ARGMAX_DENSE_MIXED = 0
(the direct sums): detections identical, points within 1e-9 range_max, the two settings identical.
"""
import json
import os

import numpy as np
import pytest

import cells64_mixed_cases as mc
import refine_cases as rc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib, synth

pytestmark = pytest.mark.gpu
SENTINEL = -7
ROUTES = {
    "mixed": {"MMW_ARGMAX_DENSE_MIXED": 1, "MMW_ARGMAX_DENSE_MIN": 1},
    "direct": {"MMW_ARGMAX_DENSE_MIXED": 0, "MMW_ARGMAX_DENSE_MIN": 1},
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


def spread(case, f, n):
    """n listed slots of frame f: the first ones (corners), both sides of the 256-cell chunk border, the last ones."""
    m = case.listed(f)
    want = list(range(min(m, n // 2))) + [d for d in (254, 255, 256, 257) if d < m] + list(range(max(0, m - n // 4), m))
    return [(f, d) for d in sorted(set(want))][:n]


_refs = {}


def longdouble_reference(c, f, dets, ants):
    """np.longdouble sums of a case's picked cells: computed once per (case, frame, picks), shared by the routes compared."""
    key = (c.name, f, tuple(dets), tuple(ants))
    if key not in _refs:
        _refs[key] = rc.longdouble_cells(c.cube[f], c.dets[f, list(dets)], ants)
    return _refs[key]


def check_values(res, route, gamma, picks):
    """picks: (f, det) slots to compare (<= 64); returns the cells of the route."""
    c = res.case
    ants = (0, 1, 2, 3)
    rc_, cells = res.cells(ants, route)
    assert rc_ == _lib.MMW_OK, f"{c.name} route {route}: {rc_}"
    listed = np.zeros(cells.shape[:2], dtype=bool)
    for f in range(c.F):
        listed[f, :c.listed(f)] = True
    assert not np.any(np.isnan(cells[listed])), f"{c.name}: a listed cell was not written"
    assert np.all(np.isnan(cells[~listed])), f"{c.name}: a slot beyond min(counts, cap) was written"
    worst_k = worst_np = 0.0
    for f in sorted({f for f, _ in picks}):
        dets = [d for ff, d in picks if ff == f]
        want, l1 = longdouble_reference(c, f, dets, ants)
        got = cells[f, dets].astype(np.clongdouble)
        ref_np = c.rd(f)[list(ants)][:, c.dets[f, dets, 0], c.dets[f, dets, 1]].T.astype(np.clongdouble)
        worst_k = max(worst_k, float(np.max(np.abs(got - want) / (rc.U * l1[None, :]))))
        worst_np = max(worst_np, float(np.max(np.abs(ref_np - want) / (rc.U * l1[None, :]))))
    print(f"{c.name} route {route}: max |err| / (2^-53 L1w) kernel {worst_k:.3f} (bound {gamma}), numpy fft2 {worst_np:.3f}")
    assert worst_k <= gamma, f"{c.name}: cell error {worst_k:.3f} u L1w exceeds the derived bound {gamma}"
    return cells


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in mc.VALUE_PLANES])
def test_mixed_cell_values(ctx, plane):
    """Fails where the route does not exist (MMW_ERR_INVALID for route 2)."""
    case = mc.case(f"value_{plane}")
    picks = spread(case, 0, 48) + spread(case, 1, 12)
    with Resident(ctx, case) as res:
        check_values(res, _lib.CELLS64_DENSE_MIXED, mc.gamma_mixed(case.S, case.C), picks)
        if plane == "63x128":         # the same plane through k_cells64<128>: each within its own bound of the same sums
            check_values(res, _lib.CELLS64_DENSE, rc.gamma_dense(case.S), picks)
        if plane == "63x100":         # ... and through the direct slices
            check_values(res, _lib.CELLS64_DIRECT, rc.gamma_direct(case.S, case.C, case.F), picks)


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in mc.UNSUPPORTED_PLANES])
def test_unsupported_planes(ctx, plane):
    case = mc.case(f"unsupported_{plane}")
    with Resident(ctx, case) as res:
        rc_, cells = res.cells((0, 1, 2, 3), _lib.CELLS64_DENSE_MIXED)
        assert rc_ == _lib.MMW_ERR_UNSUPPORTED
        assert np.all(np.isnan(cells)), "an unsupported plane was written to"


def check_indices(res, ants, shift):
    c = res.case
    want, excl, _ = c.expected(tuple(ants), int(shift))
    listed = want >= 0
    got = {}
    for route, options in ROUTES.items():
        tag = f"{c.name} {route} ants {list(ants)} shift {shift}"
        rc_, n_ref, idx = res.argmax(ants, shift, options)
        assert rc_ == _lib.MMW_OK, tag
        assert n_ref == c.n_evals, f"{tag}: {n_ref} of {c.n_evals} evaluations flagged with P_TONE = {c.P:g}"
        cmp = listed & ~excl
        bad = np.argwhere(cmp & (idx != want))
        assert len(bad) == 0, f"{tag}: {len(bad)} indices differ from the oracle's, first (f, det) {bad[0]}: {idx[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        assert np.all(idx[~listed] == SENTINEL), f"{tag}: a slot beyond min(counts, cap) was written"
        got[route] = idx
    diff = listed & (got["mixed"] != got["direct"])
    assert not np.any(diff & ~excl), f"{c.name}: the mixed and the direct route disagree"
    return got


@pytest.mark.parametrize("plane", [f"{S}x{C}" for S, C in mc.INDEX_PLANES])
@pytest.mark.parametrize("layout", list(mc.LAYOUTS))
def test_detection_layouts(ctx, layout, plane):
    """Corners of the plane and both sides of the Doppler wrap, a cell listed five times, 256 / 257 flagged cells in one frame
    (a second chunk), a list longer than dense_cap whose tail the direct kernels take in the same call, counts beyond cap, an
    empty frame between full ones; antenna lists (0, 1, 2, 3) with the fftshift and (3, 0, 2) without."""
    case = mc.case(f"{layout}_{plane}")
    with Resident(ctx, case) as res:
        check_indices(res, (0, 1, 2, 3), 1)
        check_indices(res, (3, 0, 2), 0)


def test_zero_windows(ctx):
    """S = 2: np.hanning(2) = [0, 0], every cell is exactly zero and every index 0."""
    case = mc.case("zero_2x10")
    with Resident(ctx, case) as res:
        rc_, cells = res.cells((0, 1, 2, 3), _lib.CELLS64_DENSE_MIXED)
        assert rc_ == _lib.MMW_OK
        for f in range(case.F):
            assert np.all(cells[f, :case.listed(f)] == 0)
            assert np.all(np.isnan(cells[f, case.listed(f):]))
        got = check_indices(res, (0, 1, 2, 3), 1)
        for idx in got.values():
            assert np.all(idx[idx != SENTINEL] == 0)


# ---- the reference's point clouds on shipped shapes ---------------------------------------------------------------------------
OS_PC_CASES = (("6843_RadVel_ods_10Hz.cfg", (12, 63, 100)), ("6843_RadVel_ods_20Hz.cfg", (12, 63, 70)))
YAML_OS2D = {"num_train": [5, 5], "num_guard": [3, 2], "rho": 0.7, "alpha": 2}
YAML_SEQ = dict(rng_cfar_type="os_cfar_1d", rng_cfar_params={"num_train": 5, "num_guard": 3, "rho": 0.6, "alpha": 2},
                vel_cfar_type="os_cfar_1d", vel_cfar_params={"num_train": 5, "num_guard": 2, "rho": 0.7, "alpha": 3})
AZ, EL = list(range(8)), [8, 9, 10, 11]


@pytest.mark.parametrize("cfg,shape", OS_PC_CASES, ids=[c for c, _ in OS_PC_CASES])
def test_reference_point_clouds_on_shipped_shapes(monkeypatch, cfg, shape):
    from mmwave_radar_processing_amd.batch import FramePipeline
    from mmwave_radar_processing_amd.config_managers import ConfigManager
    from mmwave_radar_processing_amd.detectors import OsCFAR2D
    from mmwave_radar_processing_amd.processors import PointCloudGenerator
    from mmwave_radar_processing_amd.processors.range_doppler_detection.range_doppler_detector_sequential import RangeDopplerDetectorSequential
    g = np.load(os.path.join(ROOT, "tests", "golden", "os_pc_np2.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "cfg_scalars.json")) as fh:
        entry = json.load(fh)[cfg]
    cm = ConfigManager()
    cm.load_cfg_text("\n".join(entry["lines"]))
    tol = 1e-9 * entry["expect"]["range_max_m"]
    tag = "x".join(str(x) for x in shape)
    seeds = [int(s) for s in g["seeds"]]
    assert all(float(g[f"{tag}_s{s}_min_margin"]) >= 1e-9 for s in seeds)
    cubes = np.stack([synth.synth_cube(s, shape) for s in seeds])
    monkeypatch.setenv("MMW_ARGMAX_BOUND_DIV", "1")
    got = {}
    refined = {}
    for mixed in ("1", "0"):
        monkeypatch.setenv("MMW_ARGMAX_DENSE_MIXED", mixed)
        if mixed == "1":        # every flagged evaluation through k_cells64_mixed (the default threshold of 8 per frame would leave
            monkeypatch.setenv("MMW_ARGMAX_DENSE_MIN", "1")     # these frames, a few flagged evaluations each, to the direct sums)
        else:
            monkeypatch.delenv("MMW_ARGMAX_DENSE_MIN", raising=False)
        pipes = {"os": FramePipeline(cm, len(seeds), shape, cfar=OsCFAR2D((5, 5), (3, 2), rho=0.7, alpha=2.0), az_antenna_idxs=AZ,
                                     el_antenna_idxs=EL),
                 "seq": FramePipeline(cm, len(seeds), shape, sequential=RangeDopplerDetectorSequential(cm, **YAML_SEQ),
                                      az_antenna_idxs=AZ, el_antenna_idxs=EL)}
        gens = {"os": PointCloudGenerator(cm, az_antenna_idxs=AZ, el_antenna_idxs=EL, detector_type="range_doppler_detector_2d",
                                          detector_params={"cfar_type": "os_cfar_2d", "cfar_params": dict(YAML_OS2D)}),
                "seq": PointCloudGenerator(cm, az_antenna_idxs=AZ, el_antenna_idxs=EL, detector_type="range_doppler_detector_sequential",
                                           detector_params=dict(YAML_SEQ))}
        for key, pipe in pipes.items():
            pipe.load(cubes)
            pcs = pipe.point_clouds()
            refined[(mixed, key)] = pipe.n_refined
            for f, s in enumerate(seeds):
                want_d, want_pc = g[f"{tag}_s{s}_{key}_dets"].reshape(-1, 2), g[f"{tag}_s{s}_{key}_pc"].reshape(-1, 4)
                np.testing.assert_array_equal(pipe.dets[f], want_d, err_msg=f"{tag} {key} seed {s} mixed {mixed}")
                np.testing.assert_allclose(pcs[f], want_pc, rtol=0, atol=tol, err_msg=f"{tag} {key} seed {s} mixed {mixed}")
                single = gens[key].process(cubes[f])
                np.testing.assert_array_equal(np.asarray(gens[key].detector.dets).reshape(-1, 2), want_d)
                np.testing.assert_allclose(single, want_pc, rtol=0, atol=tol, err_msg=f"{tag} {key} seed {s} mixed {mixed} (single frame)")
                got[(mixed, key, f)] = (pcs[f], single)
    # the float64 path had work to do, the same under both settings: with MMW_ARGMAX_DENSE_MIN = 1 all of it went through the kernel
    print(f"{tag}: evaluations refined {refined}")
    assert refined[("1", "os")] == refined[("0", "os")] > 0 and refined[("1", "seq")] == refined[("0", "seq")]
    for (mixed, key, f), (pc, single) in got.items():
        if mixed == "1":
            np.testing.assert_array_equal(pc, got[("0", key, f)][0])
            np.testing.assert_array_equal(single, got[("0", key, f)][1])
