"""The inputs and constants of tests/capon_cases.py, checked without a GPU.

1. oracle_np.capon_spectrum (float64, np.linalg.solve) against a 50-digit mpmath evaluation of the same definition on
   every conditioned case: the oracle's relative error is at most C_ORACLE * cond2 * 2**-53 per bin, so the bound the
   device is held to in test_gpu_capon.py (C_KERNEL + C_ORACLE) really leaves C_KERNEL to the device.
2. The conditioned cases span cond2 from below 1e3 to above 1e9.
3. The second-pass shapes cross the grid cap of k_capon_sweep for every CU count, and the families cover the T, V, K and
   R values they claim.
"""
import numpy as np
import pytest

import capon_cases as cc
from oracle import oracle_np as O

mp = pytest.importorskip("mpmath")


def capon_mp(Xvk, thetas, delta):
    """P(theta) of one bin, [V][K] complex64 -> list of mpf: X X^H / K + delta tr / V I, inverse, 1 / Re(a^H R^-1 a)."""
    V, K = Xvk.shape
    X = mp.matrix(V, K)
    for v in range(V):
        for k in range(K):
            X[v, k] = mp.mpc(float(Xvk[v, k].real), float(Xvk[v, k].imag))       # complex64 -> mpf is exact
    Rm = X * X.H / K
    tr = sum(Rm[v, v].real for v in range(V))
    load = mp.mpf(delta) * tr / V
    for v in range(V):
        Rm[v, v] += load
    Ri = mp.inverse(Rm)
    out = []
    for th in thetas:
        ph = -mp.pi * mp.sin(mp.mpf(float(th)))
        a = mp.matrix([mp.expj(ph * v) for v in range(V)])
        out.append(1 / (a.H * Ri * a)[0, 0].real)
    return out


def test_oracle_error_scales_with_the_condition_number():
    worst = 0.0
    with mp.workdps(50):
        for name, X, th, delta, terms in cc.conditioned_cases():
            F, V, R, K = X.shape
            for f in range(F):
                P = O.capon_spectrum(X[f], th, delta)
                for r in range(R):
                    ref = capon_mp(X[f, :, r, :], th, delta)
                    err = max(float(abs(mp.mpf(float(P[r, t])) - ref[t]) / ref[t]) for t in range(len(th)))
                    ratio = err / (terms["cond2"][f, r] * 2.0 ** -53)
                    print(f"{name} bin {r}: cond2 {terms['cond2'][f, r]:.2e}, oracle error {err:.2e}, ratio {ratio:.3f}")
                    worst = max(worst, ratio)
                    assert ratio <= cc.C_ORACLE, (name, r)
    print(f"largest ratio {worst:.3f}, C_ORACLE {cc.C_ORACLE}")


def test_conditioned_cases_span_the_condition_numbers():
    conds = np.concatenate([t["cond2"].ravel() for _, _, _, _, t in cc.conditioned_cases()])
    assert conds.min() < 1e3 and conds.max() > 1e9
    decades = set(np.floor(np.log10(conds)).astype(int))
    assert len(decades) >= 6, sorted(decades)
    for name, X, th, delta, t in cc.conditioned_cases():
        F, V, R, K = X.shape
        assert X.dtype == np.complex64 and R <= 4 and t["cond2"].shape == (F, R)
        assert delta > 0 or K >= 4 * V, name                       # delta = 0 with K < V is singular by definition
        if "scales" in t:
            c = t["cond2"][0]
            assert np.all(np.abs(c - c[0]) <= 1e-9 * c[0])          # scaling the bin leaves its conditioning alone
            tiny, huge = np.finfo(np.float32).tiny, np.finfo(np.float32).max
            P = O.capon_spectrum(X[0], th, delta)
            assert P.min() >= 8 * tiny and P.max() <= huge / 8       # the float32 output stays normal and finite
            for r, s in enumerate(t["scales"]):
                np.testing.assert_allclose(P[r], s * s * P[0], rtol=1e-12)


@pytest.mark.parametrize("num_cu", [64, 256, 304])
def test_second_pass_shapes_cross_the_grid_cap(num_cu):
    c = cc.grid_cap_bins(num_cu)
    assert c == 16 * num_cu
    table = cc.second_pass_table(num_cu)
    assert 10 <= len(table) <= 12
    shapes, vks = {}, {}
    for name, F, R, V, K, T in table:
        assert F * R > c, name
        if name.startswith("r1_three_trips"):
            assert R == 1 and F * R > 2 * c
        assert F * V * R * K * 8 <= 80 << 20 or num_cu > 256, name
        shapes[name.split("_V")[0]] = shapes.get(name.split("_V")[0], 0) + 1
        vks[(V, K)] = vks.get((V, K), 0) + 1
    assert len(shapes) == 5 and min(shapes.values()) >= 2
    assert set(vks) == set(cc.VK_VALUES) and min(vks.values()) >= 2
    assert {T for *_, T in table} == set(cc.T_VALUES)
    # the advance of the kernel, replayed: step_f / step_r per shape, and that a wrap (nr >= R) really happens somewhere
    kinds = set()
    for name, F, R, V, K, T in table:
        step_f, step_r = divmod(c, R)
        wraps = any((b % R) + step_r >= R for b in range(min(c, F * R - c)))
        kinds.add((min(step_f, 2), step_r != 0, wraps))
    assert {(0, True, True), (1, True, True), (2, False, False), (2, True, True)} <= kinds, kinds


def test_second_pass_case_is_reproducible_and_small():
    name, F, R, V, K, T = cc.second_pass_table(4)[0]            # the builders at a toy CU count
    a = cc.second_pass_case(4, name)
    b = cc.second_pass_case(4, name)
    assert a[1].dtype == np.complex64 and a[1].shape == (F, V, R, K) and len(a[2]) == T
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert len(list(cc.second_pass_shapes(4))) == len(cc.second_pass_table(4))


def test_edge_shapes_cover_their_lists():
    cases = list(cc.edge_shapes())
    assert 10 <= len(cases) <= 14
    assert {x.shape[1] for _, x, *_ in cases} == set(cc.EDGE_V)
    assert {x.shape[3] for _, x, *_ in cases} == set(cc.EDGE_K)
    assert {x.shape[2] for _, x, *_ in cases} == set(cc.EDGE_R)
    assert {len(th) for _, _, th, *_ in cases} >= {1, 64, 192, 193, 200}
    for name, X, th, delta, t in cases:
        assert t["cond2"].max() < 1e5, name


def test_poison_cases_poison_what_they_say():
    num_cu = 4
    c = cc.grid_cap_bins(num_cu)
    cases = list(cc.poison_cases(num_cu))
    ants = set()
    for name, X, th, delta, t in cases:
        F, V, R, K = X.shape
        bad = np.argwhere(~np.isfinite(X))
        assert len(bad) == len(t["poison"]) >= 2
        kinds = set()
        for (f, v, r, k, val, orig), where in zip(sorted(t["poison"], key=lambda p: (p[0], p[2])), bad):
            assert (f, v, r, k) == tuple(where) and k == K - 1 and np.isfinite(orig)
            kinds.add("nan" if np.isnan(val) else "inf")
            ants.add("first" if v == 0 else "last" if v == V - 1 else "other")
        assert kinds == {"nan", "inf"}
        trips = {(f * R + r) // c for f, _, r, *_ in t["poison"]}
        assert 0 in trips and max(trips) >= 1, name              # first trip and a later one
    assert ants == {"first", "last"}
    assert any(X.shape[3] % 32 for _, X, *_ in cases)            # the last snapshot sits in a tail chunk
    assert any(X.shape[1] < 16 and t["poison"][0][1] == 0 for _, X, _, _, t in cases)      # padding lanes re-read it
