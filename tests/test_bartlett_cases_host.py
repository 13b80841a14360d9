"""The cases of tests/bartlett_cases.py are adversarial, checked without a GPU: the planted turns are where the docstring says,
the exact references agree with ``oracle.bartlett_response``, a float32-reduction mutant fails at the large spans and passes at
the small one, the scaled operands stay inside the normal float32 range (the condition of the bit-for-bit scaling identity), and
the impulse list holds both sides of every K-split part boundary."""
import numpy as np
import pytest

import bartlett_cases as bc

SHAPES = {"masked": bc.MASKED, "fast": bc.FAST}


@pytest.fixture(scope="module")
def cases():
    return {(sh, sp): bc.dyadic_case(SHAPES[sh], sp) for sh in SHAPES for sp in bc.SPANS}


def mutant_ratio(c):
    return bc.worst_ratio(bc.response(c["X"], bc.steering_f32_mutant(c["P"], c["dirs"], c["lam"])), c["ref"])


# ------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("span", list(bc.SPANS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_planted_turns_occur_in_every_frame(cases, shape, span):
    c = cases[shape, span]
    N, one = bc.turn_units(c["Pi"], c["Di"]), 1 << 14
    assert np.abs(c["Pi"]).max() <= bc.SPANS[span] and np.abs(c["Di"]).max() <= 1024
    for f in range(len(N)):
        assert not N[f, 0].any()                                            # exactly 0 against every direction
        assert N[f, 1, 0] > 0 and N[f, 1, 0] % one == 0                     # a positive integer
        assert N[f, 2, 0] < 0 and N[f, 2, 0] % one == 0                     # a negative integer
        assert N[f, 3, 0] > one and N[f, 3, 0] % one == one // 2            # n + 1/2, n > 0
        assert N[f, 4, 0] < -one and N[f, 4, 0] % one == one // 2           # n + 1/2, n < 0
        if span in bc.LARGE_SPANS:                                          # beyond 2^11 turns with the 2^-14 bit set
            assert N[f, 5, 1] > 1 << 25 and N[f, 5, 1] & 1
            assert N[f, 6, 1] < -(1 << 25) and N[f, 6, 1] & 1
        else:                                                               # (3 * 0.05 m / lambda = 38 turns: out of reach)
            assert np.abs(N[f]).max() < 1 << 25
    # the device's float64 expression, (d / lambda) . p summed in its order, rounds nowhere on this grid
    dl = c["dirs"] * (1.0 / c["lam"])
    turns = dl[0][None, None, :] * c["P"][:, 0, :, None] + dl[1][None, None, :] * c["P"][:, 1, :, None] \
        + dl[2][None, None, :] * c["P"][:, 2, :, None]
    assert np.array_equal(turns, N * bc.TURN_UNIT)


@pytest.mark.parametrize("span", list(bc.SPANS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_reference_agrees_with_the_oracle(cases, shape, span):
    c = cases[shape, span]
    assert bc.worst_ratio(bc.oracle_response(c["X"], c["P"], c["dirs"], c["lam"]), c["ref"]) <= 1e-9


@pytest.mark.parametrize("span", list(bc.SPANS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_float32_reduction_mutant_fails_at_large_spans_only(cases, shape, span):
    ratio = mutant_ratio(cases[shape, span])
    print(f"{shape} {span}: float32-reduction mutant at {ratio:.2e} of the peak")
    if span in bc.LARGE_SPANS:
        assert ratio >= 4 * bc.SPEC_TOL
    else:
        assert ratio <= bc.SPEC_TOL


@pytest.mark.parametrize("shape", list(SHAPES))
def test_mutant_fails_on_unit_vectors_too(shape):
    ratio = mutant_ratio(bc.unit_case(SHAPES[shape]))
    print(f"{shape} unit vectors, 77 GHz, +-4 m: mutant at {ratio:.2e} of the peak")
    assert ratio >= 4 * bc.SPEC_TOL


# ------------------------------------------------------------------------------------------------------------ B
def test_split_is_exact_and_three_pieces_suffice():
    v = bc.parts(bc.scaling_case()["X"])
    p1, p2, p3 = bc.split3(v)
    assert np.array_equal(p1.astype(np.float64) + p2 + p3, v.astype(np.float64))
    assert not (p3.view(np.uint32) & np.uint32(0xFFFF)).any()              # the third piece is a bfloat16
    one = bc.parts(bc.ones_mantissa_case()["X"])
    assert set(np.abs(one).view(np.uint32).tolist()) == {0x3F7FFFFF}
    q = bc.split3(np.abs(one))
    assert [float(p[0]) for p in q] == [1 - 2.0 ** -8, 2.0 ** -8 - 2.0 ** -16, 2.0 ** -16 - 2.0 ** -24]     # every piece full


def test_scaled_operands_and_outputs_stay_normal():
    """Multiplying by 2^k is exact, and commutes with every rounding of the pipeline, while nothing leaves the normal range:
    no piece of the split of X 2^k or of W (as float64 rounds it: the device forms its own), no partial sum and no output.  A
    product of two third pieces may still fall below the normal range at k = -30; it is 2^-40 of the sum it joins, which no
    rounding sees."""
    c = bc.scaling_case()
    W = bc.steering_exact(c["Pi"], c["Di"]).astype(np.complex64)
    wp = np.abs(np.concatenate(bc.split3(bc.parts(W))))
    w_min = wp[wp > 0].min()
    S, E = c["X"].shape[1:]
    for k in bc.SCALE_K:
        Xk = bc.scaled(c["X"], k)
        assert np.array_equal(bc.parts(Xk).astype(np.float64), np.ldexp(bc.parts(c["X"]).astype(np.float64), k))
        xp = np.abs(np.concatenate(bc.split3(bc.parts(Xk))))
        x_min = xp[xp > 0].min()
        assert bc.F32_TINY <= x_min and bc.F32_TINY <= w_min
        assert 2.0 * S * E * float(xp.max()) * float(wp.max()) <= bc.F32_MAX        # any partial sum, the FFT's included
        out = np.abs(bc.parts(c["ref"] * 2.0 ** k))
        assert bc.F32_TINY <= out.min() and out.max() <= bc.F32_MAX


# ------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("E", bc.IMPULSE_E)
def test_impulse_list_holds_both_sides_of_every_part_boundary(E):
    e0 = {e for _, e in bc.index_list(E)}
    assert len(bc.index_list(E)) <= 15 * 2 and {0, 7, 8, 15, 16, 31, 32, 63, 64, 127, E - 2, E - 1} <= e0
    for F in range(1, bc.GEMM_FRAMES_PER_CALL + 1):
        ksplit, kc = bc.plan(bc.MI355X_CUS, F, bc.IMPULSE_S, E, bc.IMPULSE_T)
        assert ksplit == 4 and kc == bc.KC[E]
    bounds = bc.part_boundaries(E)
    assert len(bounds) == 3
    for b in bounds:
        assert b - 1 in e0 and b in e0, b
    # more frames than that and the planner stops splitting K as finely: the reason for calls of at most two frames
    assert bc.plan(bc.MI355X_CUS, 15, bc.IMPULSE_S, 512, bc.IMPULSE_T)[0] < bc.plan(bc.MI355X_CUS, 2, bc.IMPULSE_S, 512, bc.IMPULSE_T)[0]


@pytest.mark.parametrize("E", bc.IMPULSE_E)
@pytest.mark.parametrize("which", ["index", "row"])
def test_impulse_reference_agrees_with_the_oracle(E, which):
    cells = bc.index_list(E) if which == "index" else bc.row_list(E)
    c = bc.impulse_case(E, cells)
    assert all(np.count_nonzero(c["X"][f]) == 1 and c["X"][f, s0, e0] == 1 for f, (s0, e0) in enumerate(cells))
    assert bc.worst_ratio(bc.oracle_response(c["X"], c["P"], c["dirs"], c["lam"]), c["ref"]) <= 1e-9
    # a neighbouring k read in place of e0 moves the result by the order of the peak: every index is its own test
    for f, (s0, e0) in enumerate(cells):
        wrong = c["ref"][f] / bc.steering_exact(c["Pi"], c["Di"])[f, e0] * bc.steering_exact(c["Pi"], c["Di"])[f, e0 - 1 if e0 else 1]
        assert np.abs(wrong - c["ref"][f]).max() > 100 * bc.SPEC_TOL * np.abs(c["ref"][f]).max()


# ------------------------------------------------------------------------------------------------------------ D
def test_k_split_of_the_batch_shapes_does_not_depend_on_the_frame_count_at_256_cus():
    """What lets the GEMM paths be compared bit for bit between a 5-frame and a 1-frame call on an MI355X (the GPU test asks
    the planner's restatement with the device's own CU count, and compares at the bar where the two plans differ)."""
    for shape in (bc.MASKED, bc.FAST):
        assert bc.plan(bc.MI355X_CUS, 1, *shape) == bc.plan(bc.MI355X_CUS, 5, *shape)
    assert bc.plan(bc.MI355X_CUS, 1, *bc.MASKED)[0] == 1 and bc.plan(bc.MI355X_CUS, 1, *bc.FAST)[0] == 2
    assert bc.plan(64, 1, *bc.FAST) != bc.plan(64, 40, *bc.FAST)            # on a smaller part the claim of the issue holds
