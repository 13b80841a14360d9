"""The sequential detector's kernels straight through the C ABI on crafted profiles, row lists and shapes.

Inputs and references: tests/seq_cases.py (tests/test_seq_cases_host.py asserts, without a GPU, that the profiles hold cells that
EQUAL their threshold, that no case is vacuous and that the route-agreement scenes keep every cell clear of its threshold).

| entry                 | kernel                     | what is crafted                                                            |
|-----------------------|----------------------------|----------------------------------------------------------------------------|
| mmw_seq_rows          | k_seq_rows                 | float64 profiles with ties and non-finite cells, S = 1 .. 3072 (and 3073)  |
| mmw_seq_detect        | k_seq_detect               | row lists of every pass length on cubes of every column / group layout     |
| mmw_seq_detect_plane  | k_cfar1d_gated, list branch| the same lists                                                             |
| mmw_cfar1d_rows       | k_cfar1d_gated, list branch| float64 planes with ties and non-finite cells under six lists              |

Decisions are compared bit for bit (assert_array_equal) with cfar_cases.ref_cfar1d on the float64 rows the device itself formed
(d_rowmag of the row kernel, d_mag64 of the full-plane route); the rows are compared with the complex128 oracle under the bound
of seq_cases.value_bound.  Measured worst |row - oracle| / bound per shape (row kernel, full plane) is printed by
test_rows_stay_within_the_direct_sum_bound.
"""
import functools

import numpy as np
import pytest

import cfar_cases as cc
import seq_cases as sc
from mmwave_radar_processing_amd import _lib

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s)) for s in sc.SHAPES]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.default_context()
    c.set_option("MMW_SEQ_FULL_PLANE", 0)            # mmw_seq_route then answers for the shape alone
    yield c
    c.set_option("MMW_SEQ_FULL_PLANE", None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


POISON_BITS = _bits(np.array([sc.MAG_POISON]))[0]


# ----------------------------------------------------------------------------------------------------------- mmw_seq_rows
def run_seq_rows(ctx, bufs, prof, kind, T, G, scale, k):
    F, S = prof.shape
    d_prof, d_rows, d_nrows = bufs
    d_prof.upload(prof)
    d_rows.upload(np.full(F * S + sc.GUARD_WORDS, sc.ROW_POISON, np.int32))
    d_nrows.upload(np.full(F + sc.GUARD_WORDS, sc.ROW_POISON, np.int32))
    rc = ctx.lib.mmw_seq_rows(ctx.handle, d_prof.ptr, d_rows.ptr, d_nrows.ptr, F, S, kind, T, G, float(scale), int(k))
    rows = d_rows.download((F * S + sc.GUARD_WORDS,), np.int32)
    nrows = d_nrows.download((F + sc.GUARD_WORDS,), np.int32)
    assert np.all(rows[F * S:] == sc.ROW_POISON) and np.all(nrows[F:] == sc.ROW_POISON), "guard words written"
    return rc, rows[:F * S].reshape(F, S), nrows[:F]


@pytest.mark.parametrize("S", sc.ROWS_S)
def test_seq_rows_on_crafted_profiles(ctx, S):
    F = 4
    bufs = [ctx.alloc(F * S * 8), ctx.alloc((F * S + sc.GUARD_WORDS) * 4), ctx.alloc((F + sc.GUARD_WORDS) * 4)]
    selected = 0
    try:
        for T, G, kind, k, scale in sc.rows_cases(S):
            prof = sc.profile_frames(S, T, G)
            _, mask = sc.rows_reference(prof, kind, T, G, scale, k)
            rc, rows, nrows = run_seq_rows(ctx, bufs, prof, kind, T, G, scale, k)
            _lib.check(rc)
            tag = f"S {S} T {T} G {G} {cc.KIND_NAMES[kind]} k {k} scale {scale!r}"
            for f in range(F):
                want = np.flatnonzero(mask[f])
                assert nrows[f] == len(want), f"{tag} frame {f}"
                np.testing.assert_array_equal(rows[f, :len(want)], want, err_msg=f"{tag} frame {f}")
                assert np.all(rows[f, len(want):] == sc.ROW_POISON), f"{tag} frame {f}: written behind the list"
                selected += len(want)
            if sc.rows_case_is_empty(S, T, G, kind):
                assert not nrows.any(), tag
    finally:
        for b in bufs:
            b.free()
    assert selected > 0 or S == 1


def test_seq_rows_refuses_a_profile_longer_than_3072(ctx):
    F, S = 2, 3073
    bufs = [ctx.alloc(F * S * 8), ctx.alloc((F * S + sc.GUARD_WORDS) * 4), ctx.alloc((F + sc.GUARD_WORDS) * 4)]
    try:
        prof = np.stack([cc.quantised(S, 6, 1), cc.constant(S)])
        rc, rows, nrows = run_seq_rows(ctx, bufs, prof, cc.CA, 4, 2, 1.0, 0)
        assert rc == _lib.MMW_ERR_INVALID
        assert np.all(nrows == sc.ROW_POISON) and np.all(rows == sc.ROW_POISON)
        rc, rows, nrows = run_seq_rows(ctx, bufs, prof[:, :3072].copy(), cc.CA, 4, 2, 1.0, 0)       # and the limit itself is served
        assert rc == _lib.MMW_OK and nrows[0] == sc.rows_reference(prof[:1, :3072], cc.CA, 4, 2, 1.0, 0)[1].sum() > 0
    finally:
        for b in bufs:
            b.free()


# ----------------------------------------------------------------------------------------------------------- the two routes
class Detector:
    """Device buffers of one cube batch [F][V][S][C]; run() calls one route with poisoned outputs and guard words behind them."""

    def __init__(self, ctx, cubes, max_cap):
        self.ctx, self.shape = ctx, cubes.shape
        F, V, S, C = cubes.shape
        self.n_mag = F * S * C + C + sc.GUARD_WORDS          # one row of slack and a guard behind the float64 rows
        self.bufs = dict(cubes=ctx.alloc(cubes.nbytes), rows=ctx.alloc(F * S * 4), nrows=ctx.alloc(F * 4),
                         dets=ctx.alloc((F * max_cap * 2 + sc.GUARD_WORDS) * 4), counts=ctx.alloc((F + sc.GUARD_WORDS) * 4),
                         mag=ctx.alloc(self.n_mag * 8), mask=ctx.alloc(F * S * C))
        self.max_cap = max_cap
        self.load(cubes)

    def load(self, cubes):
        self.bufs["cubes"].upload(np.ascontiguousarray(cubes, np.complex64))

    def free(self):
        for b in self.bufs.values():
            b.free()

    def run(self, route, rows, nrows, kind, T, G, scale, k, cap, shape=None, expect=_lib.MMW_OK):
        """(dets [F][cap][2], counts [F], mags [F][S][C]): for the row kernel mags[f][j] is the row of list entry j (MAG_POISON
        behind the list), for the full plane mags[f][r] is range row r."""
        b, L, h = self.bufs, self.ctx.lib, self.ctx.handle
        F, V, S, C = self.shape if shape is None else shape
        assert cap <= self.max_cap
        n_dets = F * cap * 2
        b["rows"].upload(np.ascontiguousarray(rows, np.int32))
        b["nrows"].upload(np.ascontiguousarray(nrows, np.int32))
        b["dets"].upload(np.full(n_dets + sc.GUARD_WORDS, sc.DET_POISON, np.int32))
        b["counts"].upload(np.full(F + sc.GUARD_WORDS, sc.DET_POISON, np.int32))
        if shape is None:
            b["mag"].upload(np.full(self.n_mag, sc.MAG_POISON))
        args = (F, V, S, C, kind, T, G, float(scale), int(k), cap)
        if route == sc.ROW_KERNEL:
            rc = L.mmw_seq_detect(h, b["cubes"].ptr, b["rows"].ptr, b["nrows"].ptr, b["dets"].ptr, b["counts"].ptr, *args,
                                  b["mag"].ptr)
        else:
            rc = L.mmw_seq_detect_plane(h, b["cubes"].ptr, b["rows"].ptr, b["nrows"].ptr, b["mag"].ptr, b["mask"].ptr,
                                        b["dets"].ptr, b["counts"].ptr, *args)
        assert rc == expect, (rc, L.mmw_last_error())
        dets = b["dets"].download((n_dets + sc.GUARD_WORDS,), np.int32)
        counts = b["counts"].download((F + sc.GUARD_WORDS,), np.int32)
        assert np.all(dets[n_dets:] == sc.DET_POISON) and np.all(counts[F:] == sc.DET_POISON), "guard words written"
        if shape is not None:
            return dets[:n_dets].reshape(F, cap, 2), counts[:F], None
        mags = b["mag"].download((self.n_mag,), np.float64)
        assert np.all(_bits(mags[F * S * C:]) == POISON_BITS), "float64 rows written behind the buffer"
        return dets[:n_dets].reshape(F, cap, 2), counts[:F], mags[:F * S * C].reshape(F, S, C)


def device_rows(route, mags, f, lst, n=None):
    """The float64 rows of list lst of frame f as the route keeps them; for the row kernel the rows behind the list (of n
    entries when the list handed over was longer or malformed) must hold their poison."""
    n = len(lst) if n is None else n
    if route == sc.ROW_KERNEL:
        assert np.all(_bits(mags[f, n:]) == POISON_BITS), f"frame {f}: rows written behind the list"
        return mags[f, :len(lst)]
    return mags[f, np.asarray(lst, int)]


def assert_lists(dets, counts, want, cap, tag):
    for f, w in enumerate(want):
        assert counts[f] == len(w), f"{tag} frame {f}: count {counts[f]}, expected {len(w)}"
        n = min(cap, len(w))
        np.testing.assert_array_equal(dets[f, :n], w[:n], err_msg=f"{tag} frame {f}")
        assert np.all(dets[f, n:] == sc.DET_POISON), f"{tag} frame {f}: written behind the list"


def check_decisions(det, route, cubes, lists, kind, T, G, scale, k, cap, tag):
    """Section (a): run the lists, rebuild the expected detections from the device's own rows.  Returns (dets, counts, mags,
    detections in all)."""
    F, V, S, C = cubes.shape
    rows, nrows = sc.pack_lists(lists, S, F)
    dets, counts, mags = det.run(route, rows, nrows, kind, T, G, scale, k, cap)
    want, close = [], 0
    for f in range(F):
        lst = lists[f] if f < len(lists) else []
        w, c = sc.expected_dets(lst, device_rows(route, mags, f, lst), kind, T, G, scale, k)
        want.append(w)
        close += c
    assert close == 0, f"{tag}: {close} cells within 4 ulp of their threshold; choose another seed"
    assert_lists(dets, counts, want, cap, tag)
    return dets, counts, mags, sum(len(w) for w in want)


@functools.lru_cache(maxsize=None)
def oracle_planes(shape):
    return np.stack([sc.oracle_plane(c) for c in sc.cube_batch(shape)])


@pytest.mark.parametrize("route", [sc.ROW_KERNEL, sc.FULL_PLANE], ids=["rows", "plane"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=SHAPE_IDS)
def test_decisions_order_and_counts_on_crafted_lists(ctx, shape, route):
    """(a): every kind with two windows on the six lists, then on lists of RB - 1, RB and 2 RB rows."""
    V, S, C = shape
    cubes = sc.cube_batch(shape)
    assert ctx.lib.mmw_seq_route(ctx.handle, S, C) == 0
    cap = max(len(x) for x in sc.shape_lists(shape) + sc.pass_lists(shape)) * C       # every cell of the longest list
    det = Detector(ctx, cubes, cap)
    total = 0
    try:
        for lists in (sc.shape_lists(shape), sc.pass_lists(shape)):
            if not lists:
                continue
            for T, G in sc.DET_WINDOWS:
                for kind, k in sc.det_kinds(T):
                    tag = f"{shape} {'rows' if route == sc.ROW_KERNEL else 'plane'} {cc.KIND_NAMES[kind]} T {T} G {G} lengths " \
                          f"{[len(x) for x in lists]}"
                    total += check_decisions(det, route, cubes, lists, kind, T, G, sc.DET_SCALE, k, cap, tag)[3]
    finally:
        det.free()
    assert total > 0 or C <= 3                           # C = 1: no window fits; C = 3: hann(3) = (0, 1, 0), a flat Doppler row


@pytest.mark.parametrize("shape", sc.SHAPES, ids=SHAPE_IDS)
def test_rows_stay_within_the_direct_sum_bound(ctx, shape):
    """(b): |device row - oracle row| <= seq_cases.value_bound on every listed row, for both routes.  Measured on an MI355X: the
    worst ratio to the bound is 0.028 for the row kernel (2x12x3) and 0.034 for the full plane (1x9x1); 0.002 at 1x1024x512."""
    V, S, C = shape
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    rows, nrows = sc.pack_lists(lists, S)
    want = oracle_planes(shape)
    det = Detector(ctx, cubes, 16)
    worst = {}
    try:
        for route in (sc.ROW_KERNEL, sc.FULL_PLANE):
            mags = det.run(route, rows, nrows, cc.CA, 1, 0, sc.DET_SCALE, 0, 16)[2]
            worst[route] = 0.0
            for f, lst in enumerate(lists):
                if len(lst):
                    err = np.abs(device_rows(route, mags, f, lst) - want[f][lst]).max()
                    worst[route] = max(worst[route], err / sc.value_bound(cubes[f]))
    finally:
        det.free()
    print(f"{shape}: worst |row - oracle| / bound: row kernel {worst[sc.ROW_KERNEL]:.4f}, full plane {worst[sc.FULL_PLANE]:.4f}")
    assert worst[sc.ROW_KERNEL] <= 1.0 and worst[sc.FULL_PLANE] <= 1.0, worst


@pytest.mark.parametrize("shape", sc.ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_routes_return_the_oracle_list(ctx, shape):
    """(c): the oracle's thresholds on the oracle's plane; test_seq_cases_host.py holds the margin that makes this exact."""
    V, S, C = shape
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    rows, nrows = sc.pack_lists(lists, S)
    planes = oracle_planes(shape)
    cap = S * C
    det = Detector(ctx, cubes, cap)
    try:
        for T, G in sc.DET_WINDOWS:
            for kind, k in sc.det_kinds(T):
                want = [sc.expected_dets(lst, planes[f][lst], kind, T, G, sc.DET_SCALE, k)[0] for f, lst in enumerate(lists)]
                for route in (sc.ROW_KERNEL, sc.FULL_PLANE):
                    dets, counts, _ = det.run(route, rows, nrows, kind, T, G, sc.DET_SCALE, k, cap)
                    assert_lists(dets, counts, want, cap, f"{shape} route {route} {cc.KIND_NAMES[kind]} T {T}")
    finally:
        det.free()


@pytest.mark.parametrize("route", [sc.ROW_KERNEL, sc.FULL_PLANE], ids=["rows", "plane"])
def test_capacity_keeps_counts_exact_and_the_rest_untouched(ctx, route):
    """(d): cap 0, count - 1, count and count + 3 for a frame of known count; run() checks the guard words."""
    shape = (2, 24, 100)
    V, S, C = shape
    cubes = sc.cube_batch(shape)[:2]
    lists = [np.arange(S), np.arange(1, S, 2)]
    det = Detector(ctx, cubes, S * C)
    try:
        _, counts, _, _ = check_decisions(det, route, cubes, lists, cc.CA, 4, 2, sc.DET_SCALE, 0, S * C, "full capacity")
        count = int(counts[0])
        assert count > 3 and counts[1] > 3
        for cap in (0, count - 1, count, count + 3):
            _, c2, _, _ = check_decisions(det, route, cubes, lists, cc.CA, 4, 2, sc.DET_SCALE, 0, cap, f"cap {cap}")
            np.testing.assert_array_equal(c2, counts)
    finally:
        det.free()


@pytest.mark.parametrize("route", [sc.ROW_KERNEL, sc.FULL_PLANE], ids=["rows", "plane"])
def test_list_lengths_out_of_range_and_entries_that_name_no_row(ctx, route):
    """(e) nrows = -1 is length 0 and nrows = S + 5 is length S; section 4: entries outside [0, S) give nothing."""
    shape = (2, 24, 100)
    V, S, C = shape
    cubes = sc.cube_batch(shape)
    cap = S * C
    kind, T, G, k = cc.OS, 4, 2, 4
    det = Detector(ctx, cubes, cap)
    try:
        good = [np.zeros(0, int), np.arange(S), np.array([3]), np.array([3]), np.zeros(0, int), np.array([2, 5])]
        d0, c0, m0, n0 = check_decisions(det, route, cubes, good, kind, T, G, sc.DET_SCALE, k, cap, "clean lists")
        assert c0[1] > 0 and c0[2] > 0 and c0[5] > 0
        rows, nrows = sc.pack_lists(good, S)
        rows[0] = np.arange(S)                           # S valid entries behind a negative length
        nrows[0], nrows[1] = -1, S + 5
        rows[2, :2], nrows[2] = [-1, 3], 2
        rows[3, :2], nrows[3] = [3, S], 2
        rows[4, :1], nrows[4] = [S + 7], 1
        rows[5, :4], nrows[5] = [-2 ** 31, 2, 5, 2 ** 31 - 1], 4
        d1, c1, m1 = det.run(route, rows, nrows, kind, T, G, sc.DET_SCALE, k, cap)
        np.testing.assert_array_equal(c1, c0)
        np.testing.assert_array_equal(d1, d0)
        if route == sc.FULL_PLANE:
            np.testing.assert_array_equal(m1, m0)
        else:                                            # the rows of the entries that name a row, at their list positions
            np.testing.assert_array_equal(m1[1], m0[1])
            np.testing.assert_array_equal(m1[2, 1], m0[2, 0])
            np.testing.assert_array_equal(m1[3, 0], m0[3, 0])
            np.testing.assert_array_equal(m1[5, 1:3], m0[5, :2])
            for f, n in enumerate(nrows.clip(0, S)):
                assert np.all(_bits(m1[f, n:]) == POISON_BITS), f"frame {f}: rows written behind the list"
    finally:
        det.free()


@pytest.mark.parametrize("route", [sc.ROW_KERNEL, sc.FULL_PLANE], ids=["rows", "plane"])
def test_only_antenna_0_is_read(ctx, route):
    """(f): NaN and both infinities in antennas 1 .. V - 1 change nothing."""
    shape = (3, 32, 128)
    V, S, C = shape
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    cap = S * C
    det = Detector(ctx, cubes, cap)
    try:
        d0, c0, m0, n0 = check_decisions(det, route, cubes, lists, cc.GO, 4, 2, sc.DET_SCALE, 0, cap, "clean cube")
        assert n0 > 0
        dirty = cubes.copy()
        dirty[:, 1, ::3, ::5] = np.nan
        dirty[:, 1, 1::3, 1::5] = np.inf
        dirty[:, 2, ::2] = -np.inf + 1j * np.nan
        dirty[:, 2, 1::2] = np.inf
        det.load(dirty)
        d1, c1, m1, _ = check_decisions(det, route, dirty, lists, cc.GO, 4, 2, sc.DET_SCALE, 0, cap, "dirty antennas")
        np.testing.assert_array_equal(c1, c0)
        np.testing.assert_array_equal(d1, d0)
        np.testing.assert_array_equal(_bits(m1), _bits(m0))
    finally:
        det.free()


@pytest.mark.parametrize("plant", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("route", [sc.ROW_KERNEL, sc.FULL_PLANE], ids=["rows", "plane"])
def test_a_non_finite_sample_in_antenna_0(ctx, route, plant):
    """(g): one NaN (one +Inf) sample in antenna 0 of frame 3: decisions follow the device's own rows for every kind, the other
    frames of the call are as without it."""
    shape = (2, 24, 100)
    V, S, C = shape
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    cap = S * C
    det = Detector(ctx, cubes, cap)
    try:
        clean = {kind: check_decisions(det, route, cubes, lists, kind, 4, 2, sc.DET_SCALE, k, cap, "clean")
                 for kind, k in sc.det_kinds(4)}
        dirty = cubes.copy()
        dirty[3, 0, 7, 11] = plant
        det.load(dirty)
        for kind, k in sc.det_kinds(4):
            d1, c1, m1, _ = check_decisions(det, route, dirty, lists, kind, 4, 2, sc.DET_SCALE, k, cap,
                                            f"{cc.KIND_NAMES[kind]} with {plant}")
            d0, c0, m0, _ = clean[kind]
            assert not np.all(np.isfinite(device_rows(route, m1, 3, lists[3])))
            others = [f for f in range(sc.N_FRAMES) if f != 3]
            np.testing.assert_array_equal(c1[others], c0[others])
            np.testing.assert_array_equal(d1[others], d0[others])
            np.testing.assert_array_equal(_bits(m1[others]), _bits(m0[others]))
    finally:
        det.free()


def test_a_shape_beyond_the_lds_is_refused_and_the_next_call_served(ctx):
    """(h): mmw_seq_route and MMW_ERR_UNSUPPORTED of mmw_seq_detect above 160 KiB (nothing launched: the buffers are those of a
    small shape), then a good call."""
    for _, S, C in sc.SHAPES:
        assert ctx.lib.mmw_seq_route(ctx.handle, S, C) == 0, (S, C)
    assert ctx.lib.mmw_seq_route(ctx.handle, *sc.UNSERVED) == 1
    shape = (2, 12, 3)
    V, S, C = shape
    cubes, lists = sc.cube_batch(shape), sc.shape_lists(shape)
    det = Detector(ctx, cubes, 8)
    try:
        rows, nrows = sc.pack_lists([[0]], S, 1)
        dets, counts, _ = det.run(sc.ROW_KERNEL, rows, nrows, cc.CA, 1, 0, sc.DET_SCALE, 0, 8, shape=(1, 1) + sc.UNSERVED,
                                  expect=_lib.MMW_ERR_UNSUPPORTED)
        assert np.all(dets == sc.DET_POISON) and np.all(counts == sc.DET_POISON)
        assert b"mmw_seq_detect_plane" in ctx.lib.mmw_last_error()
        check_decisions(det, sc.ROW_KERNEL, cubes, lists, cc.CA, 1, 0, sc.DET_SCALE, 0, 8, "after the refusal")
    finally:
        det.free()


# ----------------------------------------------------------------------------------------------------------- mmw_cfar1d_rows
@pytest.mark.parametrize("kind", [cc.CA, cc.OS, cc.GO, cc.SO], ids=lambda k: cc.KIND_NAMES[k])
@pytest.mark.parametrize("shape", sc.PLANE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_list_search_on_crafted_planes(ctx, shape, kind):
    """Section 3: mask, detections and counts bit-exact row by row; unlisted rows are written 0 over a mask poisoned with 7."""
    R, D = shape
    T, G = sc.PLANE_WINDOW
    k = 4 if kind == cc.OS else 0
    lists = sc.plane_lists(R)
    rows, nrows = sc.pack_lists(lists, R)
    F = len(lists)
    fired = 0
    for name, planes in sc.planes_for_lists(shape).items():
        for scale in (1.0, cc.JUST_BELOW_ONE):
            mask_ref = sc.plane_reference(planes, lists, kind, scale)
            want = [np.argwhere(m).astype(np.int32) for m in mask_ref]
            n_max = max(len(w) for w in want)
            for cap in (R * D, n_max // 2):
                n_dets = F * cap * 2
                bufs = [ctx.alloc(planes.nbytes), ctx.alloc(rows.nbytes), ctx.alloc(nrows.nbytes), ctx.alloc(F * R * D + sc.GUARD_WORDS),
                        ctx.alloc((n_dets + sc.GUARD_WORDS) * 4), ctx.alloc(F * 4)]
                try:
                    bufs[0].upload(planes)
                    bufs[1].upload(rows)
                    bufs[2].upload(nrows)
                    bufs[3].upload(np.full(F * R * D + sc.GUARD_WORDS, 7, np.uint8))
                    bufs[4].upload(np.full(n_dets + sc.GUARD_WORDS, sc.DET_POISON, np.int32))
                    _lib.check(ctx.lib.mmw_cfar1d_rows(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                                                       bufs[5].ptr, F, R, D, kind, T, G, float(scale), k, cap))
                    mask = bufs[3].download((F * R * D + sc.GUARD_WORDS,), np.uint8)
                    dets = bufs[4].download((n_dets + sc.GUARD_WORDS,), np.int32)
                    counts = bufs[5].download((F,), np.int32)
                finally:
                    for b in bufs:
                        b.free()
                tag = f"{name} {shape} {cc.KIND_NAMES[kind]} scale {scale!r} cap {cap}"
                assert np.all(mask[F * R * D:] == 7) and np.all(dets[n_dets:] == sc.DET_POISON), tag + ": guard written"
                np.testing.assert_array_equal(mask[:F * R * D].reshape(F, R, D), mask_ref, err_msg=tag)
                assert_lists(dets[:n_dets].reshape(F, cap, 2), counts, want, cap, tag)
                fired += int(mask_ref.sum())
    assert fired > 0
