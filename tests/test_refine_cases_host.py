"""Host side of the refinement tests (no GPU): tests/refine_cases.py builds what tests/test_gpu_argmax_refine.py relies on.

The builders are seeded; every case keeps its excluded share (float64 margin below 1e-9) within 1 %; every listed detection
lies inside the plane and outside the strong component's 3 x 3 neighbourhood, and the windowed strong component really stays
inside that neighbourhood; the special cells each layout is named after are there; the oracle's complex128 cells equal
np.longdouble direct sums of the windowed cube within gamma_numpy (the yardstick the GPU value tests print beside the
kernels' errors); and the ABI lists the read-out entry."""
import os
import re

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib


def test_builders_are_seeded_and_reproducible():
    for name in ("corners_100x128", "direct_8x10", "thr32_64x128"):
        a = rc.case(name)
        seed, shape, cap, counts, layout = rc._SPECS[name]
        b = rc.Case(name, seed, shape, cap, counts, layout)
        assert a is rc.case(name) and a is not b and seed == int(seed)
        np.testing.assert_array_equal(a.cube, b.cube)
        np.testing.assert_array_equal(a.dets, b.dets)
        assert a.cube.dtype == np.complex64 and a.dets.dtype == np.int32 and a.counts.dtype == np.int32
        assert np.all(np.isfinite(a.cube.view(np.float32)))
    assert not np.array_equal(rc.case("corners_100x128").cube[0], rc.case("duplicates_100x128").cube[0])
    # a different amplitude moves only the strong component
    lo, hi = rc.make_cube(7, 1, 2, 16, 12, 10.0), rc.make_cube(7, 1, 2, 16, 12, 1000.0)
    assert np.abs(hi).max() > 50 * np.abs(lo).max()


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_case_is_well_formed_and_meets_the_exclusion_cap(name):
    c = rc.case(name)
    assert 4 <= c.V <= 32 and c.dets.shape == (c.F, c.cap, 2)
    ok = rc.allowed_cells(c.S, c.C)
    for f in range(c.F):
        n = c.listed(f)
        r, d = c.dets[f, :n, 0], c.dets[f, :n, 1]
        assert np.all((r >= 0) & (r < c.S) & (d >= 0) & (d < c.C)), "a detection outside the plane"
        assert np.all(ok[r, d]), "a detection inside the strong component's 3 x 3 neighbourhood"
        assert np.all(c.dets[f, n:] == -12345)
    lists = list(rc.ANT_LISTS.values()) if name == "ants_64x128" else [(0, 1, 2, 3), (3, 0, 2), (2, 0, 1)]
    for ants in lists:
        for shift in (1, 0):
            idx, excl, worst = c.expected(tuple(ants), shift)
            assert np.count_nonzero(idx >= 0) == c.n_evals
            assert np.count_nonzero(excl) <= rc.MAX_EXCLUDED_SHARE * c.n_evals, f"{name} {ants} {shift}: choose another seed"
            assert worst >= rc.MARGIN_MIN
            if len(ants) == 1:
                assert not excl.any() and np.all(idx[idx >= 0] == 0)
            if min(c.S, c.C) == 2:                  # np.hanning(2) = [0, 0]: all-zero spectra, index 0, nothing excluded
                assert not excl.any() and np.all(idx[idx >= 0] == 0)


def test_layouts_hold_the_cells_they_are_named_after():
    for plane in ("256x128", "100x128"):
        S, C = (int(v) for v in plane.split("x"))
        c = rc.case(f"corners_{plane}")
        have = {tuple(x) for x in c.dets[0, :c.listed(0)]}
        assert {(r, d) for r in (0, S - 1) for d in (0, 63, 64, 127)} <= have
        c = rc.case(f"duplicates_{plane}")
        cells, n = np.unique(c.dets[0, :c.listed(0)], axis=0, return_counts=True)
        assert n.max() >= 5
        assert [rc.case(f"{n}_{plane}").listed(0) for n in ("n256", "n257", "n513")] == [256, 257, 513]
        c = rc.case(f"n700_{plane}")
        assert c.counts.tolist() == [0, 700, 0] and c.n_evals <= 256 * c.F
        c = rc.case(f"tail_{plane}")
        assert c.n_evals > min(c.F * c.cap, 256 * c.F)
        c = rc.case(f"overcap_{plane}")
        assert c.counts[0] == c.cap + 7 and c.listed(0) == c.cap
        c = rc.case(f"alternating_{plane}")
        assert c.counts.tolist() == [24, 0, 24, 0]
    a, b = rc.case("thr31_64x128"), rc.case("thr32_64x128")
    assert (a.n_evals, b.n_evals) == (31, 32) == (8 * a.F - 1, 8 * a.F)
    assert sorted(len(v) for v in rc.ANT_LISTS.values()) == [1, 3, 4, 5, 5, 6, 8, 9, 16, 32]
    steps = [F for F in range(1, 20000) if rc.refine_parts(F) != rc.refine_parts(F + 1)]
    assert sorted(rc.PARTS_STEPS) == sorted(steps + [F + 1 for F in steps])
    # the slicing of k_argmax_refine_part on the sweep's planes: (slice length, slices that hold cells) per slice count
    def slicing(S, C, F):
        parts = rc.refine_parts(F)
        per = -(-(-(-(S * C) // parts)) // 256) * 256
        return parts, per, -(-(S * C) // per)
    assert [slicing(20, 56, F) for F in rc.PARTS_STEPS] == [(16, 256, 5), (8, 256, 5), (8, 256, 5), (4, 512, 3), (4, 512, 3), (2, 768, 2)]
    assert {slicing(S, C, F)[1:] for S, C in rc.PARTS_PLANES[:3] for F in rc.PARTS_STEPS} == {(256, 1)}
    for S, C in rc.PARTS_PLANES:
        assert rc.case(f"parts_15001_{S}x{C}").cube.nbytes < 600 << 20
    # the limits of the dense kernel's LDS, as csrc/mmw_cells64.h computes them
    lds = lambda S: (64 * 137 + S) * 16 + (S + 128) * 8 + 256 * 8 + 64
    assert lds(829) <= 160 * 1024 - 512 < lds(830)


@pytest.mark.parametrize("S,C", [(8, 10), (63, 100), (100, 128), (16, 320)])
def test_strong_component_stays_in_its_neighbourhood(S, C):
    """hann * g is a raised cosine: without noise, and before the float32 rounding of the samples, every cell outside the
    3 x 3 neighbourhood is zero to rounding (1e-12 of the peak); a plain tone of the same bin is not (the reason for g)."""
    r0, k0 = rc.tone_of(S, C)
    s, c = np.arange(S)[:, None], np.arange(C)[None, :]
    tone = np.exp(2j * np.pi * (r0 * s / S + k0 * c / C))
    w = np.hanning(S)[:, None] * np.hanning(C)[None, :]
    spec = np.fft.fftshift(np.fft.fft2(w * tone * rc.taper(S)[:, None] * rc.taper(C)[None, :]), axes=1)
    peak = np.abs(spec).max()
    assert np.unravel_index(np.argmax(np.abs(spec)), spec.shape) == (r0, rc.doppler_index(k0, C))
    assert np.abs(spec[rc.allowed_cells(S, C)]).max() <= 1e-12 * peak
    plain = np.fft.fftshift(np.fft.fft2(w * tone), axes=1)
    assert np.abs(plain[rc.allowed_cells(S, C)]).max() >= 1e-4 * np.abs(plain).max()
    assert rc.taper(S).max() <= 4.1 and rc.taper(S).min() >= 0.0


@pytest.mark.parametrize("name", ["direct_8x10", "direct_63x100"])
def test_oracle_cells_equal_longdouble_direct_sums(name):
    c = rc.case(name)
    ants = (0, 1, 2, 3)
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 here"
    dets = c.dets[0, :6]
    want, l1 = rc.longdouble_cells(c.cube[0], dets, ants)
    got = c.rd(0)[list(ants)][:, dets[:, 0], dets[:, 1]].T
    ratio = float(np.max(np.abs(got.astype(np.clongdouble) - want) / (rc.U * l1[None, :])))
    gamma = rc.gamma_numpy(c.S, c.C)
    print(f"{name}: np.fft.fft2 complex128 against longdouble sums: max |err| / (2^-53 L1w) = {ratio:.3f}, bound {gamma}")
    assert ratio <= gamma
    assert float(np.max(np.abs(want))) < 1e-3 * float(l1.min())        # the cells are small beside L1w: the sums cancel


def test_error_bound_formulas():
    assert [rc.gamma_dense(S) for S in (8, 64, 65, 100, 256, 512, 829)] == [85, 85, 93, 93, 109, 141, 181]
    assert rc.gamma_direct(256, 128, 3) == 12 + 8 + 6 + 2 + 16 and rc.gamma_direct(8, 10, 3) == 12 + 1 + 8 + 16
    assert rc.gamma_direct(8, 10, 15001) == 12 + 1 + 8 + 2
    assert rc.gamma_numpy(8, 10) == 4 + 3 * 6 + 6 + 9 and rc.gamma_numpy(63, 100) == 4 + (7 + 7 + 11) + (6 + 6 + 9 + 9)


def test_header_and_ctypes_table_list_the_read_out_entry():
    text = open(os.path.join(ROOT, "include", "mmwgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint mmw_rd_cells64_at\s*\((.*?)\);", code, flags=re.S)
    assert decl, "mmw_rd_cells64_at is not declared in mmwgpu.h"
    assert "mmw_rd_cells64_at" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_rd_cells64_at"]) == decl.group(1).count(",") + 1 == 13
    assert "point_cloud_generator.py" in text[text.index("mmw_rd_cells64_at:"):text.index("#define MMW_CELLS64_DENSE")]
    for name, value in (("MMW_CELLS64_DENSE", _lib.CELLS64_DENSE), ("MMW_CELLS64_DIRECT", _lib.CELLS64_DIRECT)):
        assert int(re.search(rf"#define {name}\s+(\d+)", code).group(1)) == value
    lib = _lib.load_library()
    assert hasattr(lib, "mmw_rd_cells64_at")
    assert lib.mmw_abi_version() == _lib.ABI_VERSION == 7           # an added entry changes no existing signature
    # argument checks that need no device
    assert lib.mmw_rd_cells64_at(None, None, None, None, None, 1, 1, 8, 8, 1, None, 0, 0) == _lib.MMW_ERR_INVALID
