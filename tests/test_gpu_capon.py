"""mmw_capon (k_capon_sweep) straight through the C ABI: past the first trip of its capped grid, and on its numerics.

Inputs: tests/capon_cases.py (tests/test_capon_cases_host.py checks them and the oracle's own error without a GPU).

| test                          | what would make it fail                                                                 |
|-------------------------------|-----------------------------------------------------------------------------------------|
| second pass, bit-exact        | any bin of a later trip computed from other snapshots than a lone first-trip call reads: |
|                               | the (frame, bin) advance, the `more` branch, a prefetch slot handed over wrongly        |
| second pass, oracle           | the same, and all bins at once, at the numerics bound                                    |
| numerics bound                | an error that grows faster than (C_KERNEL + C_ORACLE) cond2 2^-53 beside float32 rounding |
| scale invariance              | denormal flush, overflow of the trace, a reciprocal that loses bits far from 1           |
| poison isolation              | a NaN / Inf reaching another bin through the shared prefetch slots or the LDS strips     |
| angle-table cache             | a stale or mis-keyed device table of exp(-j pi sin theta)                                 |
| arguments                     | an entry that launches on shapes capon() cannot index, or writes on a refused call       |
"""
import ctypes as C
import functools

import numpy as np
import pytest

import capon_cases as cc
from mmwave_radar_processing_amd import _lib
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

SECOND_PASS_NAMES = [row[0] for row in cc.second_pass_table(256)]        # the names do not depend on the CU count
CONDITIONED = list(cc.conditioned_cases())
EDGES = list(cc.edge_shapes())
REFUSED = (_lib.MMW_ERR_INVALID, _lib.MMW_ERR_UNSUPPORTED)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@functools.lru_cache(maxsize=None)
def num_cu():
    return _lib.device_info(0)["num_cu"]


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run_capon(ctx, X, th, delta):
    F, V, R, K = X.shape
    th = np.ascontiguousarray(th, dtype=np.float64)
    T = len(th)
    d_x, d_p = ctx.alloc(X.nbytes), ctx.alloc(F * R * T * 4)
    try:
        d_x.upload(X)
        d_p.upload(np.full(F * R * T, -7.0, np.float32))            # every output must be written
        _lib.check(ctx.lib.mmw_capon(ctx.handle, d_x.ptr, dptr(th), d_p.ptr, F, V, R, K, T, float(delta)))
        return d_p.download((F, R, T), np.float32)
    finally:
        d_x.free()
        d_p.free()


_batches = {}


def second_pass_batch(ctx, name):
    """The case's inputs (rebuilt: tens of MB) and the batch's device result (kept: the two tests of a case share it)."""
    case = cc.second_pass_case(num_cu(), name)
    if name not in _batches:
        _batches[name] = run_capon(ctx, case[1], case[2], case[3])
    return case, _batches[name]


def oracle(X, th, delta):
    return np.stack([O.capon_spectrum(X[f], th, delta) for f in range(X.shape[0])])


def assert_within_bound(P, ref, cond, label):
    """|P - ref| <= (2^-23 + (C_KERNEL + C_ORACLE) cond2 2^-53) |ref| elementwise; prints the observed figures first."""
    err = np.abs(P.astype(np.float64) - ref) / np.abs(ref)
    worst = err.max(axis=-1)
    lit = worst / (cond * 2.0 ** -53)
    seen = worst > 2.0 ** -24                      # bins whose error is more than the rounding of the float32 output
    i = np.unravel_index(np.argmax(worst / cc.bound(cond)), worst.shape)
    print(f"{label}: cond2 {cond.min():.2e}..{cond.max():.2e}, worst error {worst.max():.3e}, tightest bin: error {worst[i]:.3e} "
          f"of bound {cc.bound(cond[i]):.3e}; largest error / (cond2 2^-53) among the {int(seen.sum())} bins with error > 2^-24: "
          + (f"{lit[seen].max():.3g}" if seen.any() else "none (float32 rounding only)"))
    assert np.all(np.isfinite(P)), label
    assert np.all(err <= cc.bound(cond)[..., None]), label


def sampled_bins(F, R, c, seed):
    """About 24 bins: the first and last of each trip, both sides of frame boundaries, a few random ones."""
    n = F * R
    bins = []
    for t0 in range(0, n, c):
        bins += [t0, min(t0 + c, n) - 1]
    frames = sorted({1, 2, F - 1, c // R, c // R + 1, (2 * c) // R + 1} & set(range(1, F)))
    for f in frames:
        bins += [f * R - 1, f * R]
    bins += [c + 1, c + 2, c + 3, n - 2]
    rng = np.random.default_rng(seed)
    bins += list(rng.integers(0, n, 6)) + list(rng.integers(c, n, 4))
    out = []
    for b in bins:
        if 0 <= b < n and b not in out:
            out.append(int(b))
    return out[:28]


@pytest.mark.parametrize("name", SECOND_PASS_NAMES)
def test_second_pass_equals_single_bin_calls(ctx, name):
    """A bin of a later trip must be the very numbers a lone call computes for it: a single-bin call (n_frames = 1,
    R = 1) is always a first trip, reads its chunks through the first fetches and hands nothing over.  No tolerance."""
    (_, X, th, delta, _), P = second_pass_batch(ctx, name)
    F, V, R, K = X.shape
    c = cc.grid_cap_bins(num_cu())
    assert F * R > c                                   # the precondition: some wave takes a second bin
    bins = sampled_bins(F, R, c, len(name))
    assert any(b >= c for b in bins)
    for b in bins:
        f, r = divmod(b, R)
        alone = run_capon(ctx, np.ascontiguousarray(X[f:f + 1, :, r:r + 1, :]), th, delta)
        assert np.array_equal(alone[0, 0], P[f, r]), f"{name}: bin {b} (frame {f}, range bin {r}, trip {b // c})"


@pytest.mark.parametrize("name", SECOND_PASS_NAMES)
def test_second_pass_against_the_oracle(ctx, name):
    (_, X, th, delta, _), P = second_pass_batch(ctx, name)
    assert_within_bound(P, oracle(X, th, delta), cc.cond2(X, delta), name)
    _batches.pop(name, None)


@pytest.mark.parametrize("case", CONDITIONED + EDGES, ids=[c[0] for c in CONDITIONED + EDGES])
def test_numerics_bound(ctx, case):
    name, X, th, delta, terms = case
    assert_within_bound(run_capon(ctx, X, th, delta), oracle(X, th, delta), terms["cond2"], name)


def test_scale_invariance(ctx):
    """P(s X) = s^2 P(X) for s ~ 1e-20 and ~ 1e+15 (exact products in complex64, capon_cases.conditioned_cases): every
    intermediate of the kernel scales by a power of s, so only the two float32 roundings of the outputs differ."""
    name, X, th, delta, terms = next(c for c in CONDITIONED if "scales" in c[4])
    P = run_capon(ctx, X, th, delta)[0].astype(np.float64)
    assert np.all(np.isfinite(P)) and np.all(P >= np.finfo(np.float32).tiny)
    for r, s in enumerate(terms["scales"]):
        want = s * s * P[0]
        dev = np.max(np.abs(P[r] - want) / want)
        print(f"scale {s:.4e}: P(sX) against s^2 P(X) {dev:.3e} (bound {2.0 ** -22:.3e})")
        assert dev <= 2.0 ** -22, s


@pytest.mark.parametrize("index", [0, 1, 2])
def test_poison_stays_in_its_bin(ctx, index):
    name, X, th, delta, terms = list(cc.poison_cases(num_cu()))[index]
    F, V, R, K = X.shape
    clean = X.copy()
    bad = np.zeros((F, R), bool)
    for f, v, r, k, val, orig in terms["poison"]:
        clean[f, v, r, k] = orig
        bad[f, r] = True
    assert np.all(np.isfinite(clean)) and bad.sum() == len(terms["poison"])
    P, Pc = run_capon(ctx, X, th, delta), run_capon(ctx, clean, th, delta)
    assert np.all(np.isfinite(Pc))
    assert np.array_equal(P[~bad], Pc[~bad]), name                 # every other bin: bit for bit what it was
    assert not np.any(np.isfinite(P[bad])), name                   # the poisoned bins: never a finite number


def test_angle_table_cache():
    """The device table of exp(-j pi sin theta) is keyed on the caller's grid (memcmp): A, B (same T, other values), A,
    another T, A, and A with -0.0 for +0.0 (another key, the same numbers) each equal a fresh context's result."""
    rng = np.random.default_rng(77)
    X = (rng.standard_normal((1, 6, 3, 20)) + 1j * rng.standard_normal((1, 6, 3, 20))).astype(np.complex64)
    A = np.linspace(-1.0, 1.0, 71)
    assert A[35] == 0.0 and not np.signbit(A[35])
    A_neg = A.copy()
    A_neg[35] = -0.0
    assert A_neg.tobytes() != A.tobytes()
    B = np.linspace(-1.3, 0.9, 71)
    Cg = np.linspace(-1.2, 1.2, 200)

    def fresh(grid):
        c = _lib.Context(0)
        try:
            return run_capon(c, X, grid, 1e-2)
        finally:
            c.close()

    want = {k: fresh(g) for k, g in (("A", A), ("B", B), ("C", Cg))}
    assert not np.array_equal(want["A"], want["B"])
    c = _lib.Context(0)
    try:
        for k, g in (("A", A), ("B", B), ("A", A), ("C", Cg), ("A", A), ("A", A_neg), ("A", A), ("B", B)):
            assert np.array_equal(run_capon(c, X, g, 1e-2), want[k]), k
    finally:
        c.close()


def test_arguments(ctx):
    """Refused calls return MMW_ERR_INVALID / MMW_ERR_UNSUPPORTED and leave d_out alone (capon() indexes 16-wide strips
    and divides by V and K); n_frames = 0 is MMW_OK and writes nothing."""
    F, V, R, K, T = 2, 4, 3, 8, 5
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((F, 17, R, K)) + 1j * rng.standard_normal((F, 17, R, K))).astype(np.complex64)     # room for V = 17
    th = np.linspace(-1, 1, T)
    sentinel = np.full(F * R * 17, -123.0, np.float32)
    d_x, d_p = ctx.alloc(X.nbytes), ctx.alloc(sentinel.nbytes)
    L, h = ctx.lib, ctx.handle
    try:
        d_x.upload(X)
        d_p.upload(sentinel)

        def call(ctxh=h, x=d_x.ptr, t=dptr(th), p=d_p.ptr, f=F, v=V, r=R, k=K, nt=T, delta=1e-2):
            st = L.mmw_capon(ctxh, x, t, p, f, v, r, k, nt, delta)
            ctx.sync()
            return st

        refused = dict(null_ctx=dict(ctxh=None), null_x=dict(x=None), null_thetas=dict(t=None), null_out=dict(p=None),
                       v17=dict(v=17), v0=dict(v=0), v_negative=dict(v=-1), k0=dict(k=0), t0=dict(nt=0), r0=dict(r=0),
                       frames_negative=dict(f=-1), delta_negative=dict(delta=-1e-3), delta_nan=dict(delta=float("nan")),
                       delta_inf=dict(delta=float("inf")))
        for what, kw in refused.items():
            assert call(**kw) in REFUSED, what
            np.testing.assert_array_equal(d_p.download(sentinel.shape, np.float32), sentinel, err_msg=what)
        assert call(f=0) == _lib.MMW_OK
        np.testing.assert_array_equal(d_p.download(sentinel.shape, np.float32), sentinel)
        # and the accepted extremes write exactly their F * R * T outputs: V = 16, V = 1, delta = 0
        for v, delta in ((16, 1e-2), (1, 1e-2), (4, 0.0)):
            Xv = np.ascontiguousarray(X[:, :v])
            d_x.upload(Xv)
            assert call(v=v, delta=delta) == _lib.MMW_OK
            got = d_p.download(sentinel.shape, np.float32)
            np.testing.assert_array_equal(got[F * R * T:], sentinel[F * R * T:])
            assert_within_bound(got[:F * R * T].reshape(F, R, T), oracle(Xv, th, delta), cc.cond2(Xv, delta),
                                f"V={v}, delta={delta}")
            d_p.upload(sentinel)
    finally:
        d_x.free()
        d_p.free()
