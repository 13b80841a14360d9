"""Host side of the dense float64 cell kernel for planes of any chirp count (no GPU): the plan predicate
mmw_diag_cells64_plan over every shipped cube shape, the header and the bindings of the new read-out route, the case builders
of tests/cells64_mixed_cases.py, and its a-priori error bound gamma_mixed against a float64 NumPy model of the kernel's
operation order."""
import json
import os
import re

import numpy as np
import pytest

import cells64_mixed_cases as mc
import refine_cases as rc
from conftest import ROOT
from mmwave_radar_processing_amd import _lib


def plan(S, C):
    lib = _lib.load_library()
    out = (_lib.C.c_int * 8)()
    assert lib.mmw_diag_cells64_plan(S, C, out) == _lib.MMW_OK
    return list(out)


def shipped_shapes():
    with open(os.path.join(ROOT, "tests", "golden", "cfg_scalars.json")) as fh:
        cfgs = json.load(fh)
    return sorted({(c["expect"]["num_samples"], c["expect"]["loops"]) for c in cfgs.values()})


def test_plan_over_the_shipped_shapes():
    shapes = shipped_shapes()
    assert {C for _, C in shapes} >= set(mc.MUST_COVER), "the shipped chirp counts changed: revisit MUST_COVER"
    for S, C in shapes:
        p = plan(S, C)
        if C in mc.MUST_COVER:
            R1, R2 = mc.FACTORS[C]
            assert p[0] == mc.KIND_MIXED, f"{S} x {C}: no dense kernel"
            assert p[1] * p[2] == C and (p[1], p[2]) == (R1, R2)
            assert p[3] == mc.rows_per_pass(C) and p[3] % 8 == 0 and p[3] * p[2] <= mc.NT
            assert p[4] == mc.lds_bytes(S, C) <= mc.LDS_MAX
            assert p[5] == 256 and p[6] == mc.pitch(C) and p[6] % 2 == 1 and p[6] > C and p[7] == 1
        elif C == 128:
            assert p[0] == (mc.KIND_128 if S <= 829 else mc.KIND_NONE), f"{S} x {C}"
        else:
            assert C in mc.NOT_COVERED and p == [0] * 8, f"{S} x {C}"


def test_plan_pins():
    # 128 chirps: k_cells64<128> under exactly its own condition (829 samples is the last plane its LDS takes)
    for S in (256, 829):
        p = plan(S, 128)
        assert p[:4] == [mc.KIND_128, 16, 8, 64] and p[5] == 256 and p[6] == 137 and p[7] == 1
        assert p[4] == (64 * 137 + S) * 16 + (S + 128) * 8 + 256 * 8 + 64
    assert plan(830, 128)[0] == mc.KIND_NONE and plan(830, 128)[7] == 1         # (the mixed kernel keeps 32 rows per pass)
    # no instantiation: 320 chirps, the prime 127, 115 = 5 * 23, 11
    for S, C in ((16, 320), (63, 127), (63, 115), (8, 11)):
        assert plan(S, C) == [0] * 8
    # the test-only instantiations
    for S, C in ((8, 10), (16, 15), (20, 56)):
        assert plan(S, C)[:3] == [mc.KIND_MIXED, *mc.FACTORS[C]]
    # tables beyond 160 KiB - 512 B: none
    big = next(S for S in range(1, 65536) if mc.lds_bytes(S, 100) > mc.LDS_MAX)
    assert plan(big - 1, 100)[0] == mc.KIND_MIXED and plan(big, 100) == [0] * 8
    lib = _lib.load_library()
    assert lib.mmw_diag_cells64_plan(0, 100, (_lib.C.c_int * 8)()) == _lib.MMW_ERR_INVALID
    assert lib.mmw_diag_cells64_plan(63, 100, None) == _lib.MMW_ERR_INVALID


def test_header_and_bindings():
    with open(os.path.join(ROOT, "include", "mmwgpu.h")) as fh:
        text = fh.read()
    m = re.search(r"^#define\s+MMW_CELLS64_DENSE_MIXED\s+(\d+)\s*$", text, flags=re.M)
    assert m and int(m.group(1)) == _lib.CELLS64_DENSE_MIXED == 2
    assert text.index("#define MMW_CELLS64_DIRECT") < m.start()
    assert (_lib.CELLS64_DENSE, _lib.CELLS64_DIRECT) == (0, 1)
    assert re.search(r"\bint mmw_diag_cells64_plan\s*\(int S, int C, int plan\[8\]\);", text)
    assert "mmw_diag_cells64_plan:" in text
    assert "mmw_diag_cells64_plan" in _lib.EXPORTED and len(_lib._SIGNATURES["mmw_diag_cells64_plan"]) == 3
    lib = _lib.load_library()
    assert hasattr(lib, "mmw_diag_cells64_plan")
    assert lib.mmw_abi_version() == 7
    # the route is validated before anything touches a device
    assert lib.mmw_rd_cells64_at(None, None, None, None, None, 1, 1, 8, 8, 1, None, 0, 2) == _lib.MMW_ERR_INVALID


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_builders(name):
    c = mc.case(name)
    seed, shape, cap, counts, layout = mc._SPECS[name]
    assert (c.F, c.V, c.S, c.C) == shape and c.F <= 4 and c.V == 4 and c.cap == cap and c.dets.shape == (c.F, c.cap, 2)
    np.testing.assert_array_equal(c.counts, counts)
    ok = rc.allowed_cells(c.S, c.C)
    for f in range(c.F):
        n = c.listed(f)
        assert n == min(counts[f], cap)
        r, d = c.dets[f, :n, 0], c.dets[f, :n, 1]
        assert np.all((r >= 0) & (r < c.S) & (d >= 0) & (d < c.C)), "a detection outside the plane"
        assert np.all(ok[r, d]), "a detection inside the strong component's 3 x 3 neighbourhood"
        assert np.all(c.dets[f, n:] == -12345)
    assert c.n_evals == sum(min(n, cap) for n in counts)
    # all-flagged construction: the strong component is there (planes of 5 x 5 cells and more) ...
    assert (c.tone is None) == (min(c.S, c.C) < 5)
    if c.tone is not None:
        assert np.abs(c.cube).max() > 0.5 * c.P
    if name.startswith("unsupported"):
        return
    # ... and the exclusion rule leaves the case its evaluations
    for ants, shift in (((0, 1, 2, 3), 1), ((3, 0, 2), 0)):
        idx, excl, worst = c.expected(ants, shift)
        assert np.count_nonzero(idx >= 0) == c.n_evals
        assert np.count_nonzero(excl) <= rc.MAX_EXCLUDED_SHARE * c.n_evals, f"{name} {ants} {shift}: choose another seed"
        assert worst >= rc.MARGIN_MIN
        if c.S == 2:
            assert not excl.any() and np.all(idx[idx >= 0] == 0)


def test_layout_cells():
    for S, C in mc.INDEX_PLANES:
        c = mc.case(f"corners_{S}x{C}")
        want = {(r, d) for r in (0, S - 1) for d in (0, C // 2 - 1, C // 2, C - 1)}       # both sides of the Doppler wrap
        for f in range(c.F):
            assert want <= {tuple(x) for x in c.dets[f, :c.listed(f)]}
        c = mc.case(f"duplicates_{S}x{C}")
        for f in range(c.F):
            cells, n = np.unique(c.dets[f, :c.listed(f)], axis=0, return_counts=True)
            assert n.max() >= 5
        assert mc.case(f"n256_{S}x{C}").listed(0) == 256 and mc.case(f"n257_{S}x{C}").listed(0) == 257
        t = mc.case(f"tail_{S}x{C}")
        assert t.n_evals > min(t.F * t.cap, 256 * t.F)                                     # beyond dense_cap
        o = mc.case(f"overcap_{S}x{C}")
        assert o.counts[0] > o.cap and o.listed(0) == o.cap
        a = mc.case(f"alternating_{S}x{C}")
        assert list(a.counts) == [24, 0, 24, 0]


def test_factor_table_and_bound_terms():
    for C, (R1, R2) in mc.FACTORS.items():
        assert R1 * R2 == C and 2 <= R2 <= 16 and R1 <= 10
    assert [mc.gamma_regdft(R) for R in (1, 2, 3, 4, 5, 7, 8, 9, 10, 14, 16)] == [0, 1, 5, 10, 6, 7, 15, 14, 7, 8, 20]
    # 63 x 100: 10 x 10, 48 rows per pass (6 per lane), two passes
    assert mc.gamma_mixed(63, 100) == 4 + 7 + 4 + 7 + 21 + 2 + 12 + 3
    # 63 x 128 through the mixed kernel: 8 x 16, 32 rows per pass (4 per lane), two passes
    assert mc.gamma_mixed(63, 128) == 4 + 15 + 4 + 20 + 13 + 2 + 8 + 3


@pytest.mark.parametrize("plane", [(8, 10), (20, 56)])
def test_bound_against_a_float64_model_of_the_operation_order(plane):
    """The NumPy model (same levels, same partial sums, same recurrence) against np.longdouble direct sums: within gamma_mixed,
    and the model itself equals the oracle's cells to rounding."""
    S, C = plane
    c = mc.case(f"value_{S}x{C}")
    ants = (0, 1, 2, 3)
    cells = c.dets[0, :64]
    want, l1 = rc.longdouble_cells(c.cube[0], cells, ants)
    worst = 0.0
    for j, a in enumerate(ants):
        got = mc.model_cells(c.cube[0, a], cells).astype(np.clongdouble)
        worst = max(worst, float(np.max(np.abs(got - want[:, j]) / (rc.U * l1[j]))))
    gamma = mc.gamma_mixed(S, C)
    print(f"{S} x {C}: float64 model max |err| / (2^-53 L1w) {worst:.3f} (bound {gamma})")
    assert 0 < worst <= gamma
